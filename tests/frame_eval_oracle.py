"""NumPy restatement of mvp_frame_confusion_f32 / mvp_label_histogram_u16 / mvp_label_histogram_i64 (include/mvp_hip.h), built on
tests/resize_oracle.py's prepare_labels.  TEST INFRASTRUCTURE: held to Pillow, to the reference's Evaluator and to the weight arithmetic
of compute_label_weights.py by tests/test_frame_eval_cpu.py through tests/golden/frame_eval.npz, and the library is held to it.
Also the seeded inputs of that fixture (fixture_inputs), shared by its generator and the tests."""
import numpy as np

from tests import resize_oracle as RO

EVAL_CLASS_IDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]


def first_argmax(logit):
    """logit (Nf,C,h,w) float32 -> (Nf,h,w) int64: the first maximum by strict `>` from class 0 (no NaN: outside the contract)"""
    logit = np.asarray(logit, np.float32)
    am = np.zeros(logit.shape[:1] + logit.shape[2:], np.int64)
    mx = logit[:, 0].copy()
    for c in range(1, logit.shape[1]):
        win = logit[:, c] > mx
        am[win] = c
        mx[win] = logit[:, c][win]
    return am


def frame_confusion(logit, labels, picked, size=None, mapping=None, ignore_value=-100, out=None):
    """-> (mat (C,C) int64 [label][argmax] over the pixels whose mapped label lies in [0,C), added to `out`; pred (Nf,h,w) int64).
    labels None: (None, pred)."""
    pred = first_argmax(logit)
    if labels is None:
        return None, pred
    C = logit.shape[1]
    lab = RO.prepare_labels(labels, picked, size=size, mapping=mapping, ignore_value=ignore_value)
    assert lab.shape == pred.shape, (lab.shape, pred.shape)
    keep = (lab >= 0) & (lab < C)
    mat = np.zeros((C, C), np.int64) if out is None else np.array(out, np.int64)
    np.add.at(mat, (lab[keep], pred[keep]), 1)
    return mat, pred


def label_histogram(labels, nbins, picked=None, size=None, mapping=None, out=None):
    """labels (Ftot,H,W) uint16 (read through picked / size / mapping; a raw id past the mapping counts nowhere) or int64 of any shape
    -> (nbins,) int64 counts of the values in [0,nbins), added to `out`"""
    labels = np.asarray(labels)
    if labels.dtype == np.uint16:
        picked = np.arange(len(labels)) if picked is None else picked
        v = RO.prepare_labels(labels, picked, size=size, mapping=mapping, ignore_value=-1).ravel()
    else:
        v = labels.astype(np.int64).ravel()
    hist = np.zeros(nbins, np.int64) if out is None else np.array(out, np.int64)
    v = v[(v >= 0) & (v < nbins)]
    return hist + np.bincount(v, minlength=nbins)[:nbins]


def label_log_weights(hist, class_ids=None):
    """compute_label_weights.py:27-29 / :45-47 on integer counts: float32 counts [at class_ids] / their float32 sum -> 1 / log(1.2 + w)"""
    w = np.asarray(hist).astype(np.float64).astype(np.float32)
    if class_ids is not None:
        w = w[list(class_ids)]
    w = w / np.sum(w)
    return 1 / np.log(1.2 + w)


# ---- the fixture's inputs, from the seed -------------------------------------------------------------------------------------------------
FIX_STORE = (5, 23, 31)   # Ftot, H, W
FIX_SIZE = (7, 5)         # PIL's (w, h): 23 x 31 -> 5 x 7, a non-integer ratio on both axes
FIX_PICKED = [4, 0, 0, 2, 3]
FIX_C = 20
FIX_T = 41                # raw ids 0..47 in the store: 41..47 lie past the mapping


def fixture_inputs():
    """-> dict: labels (5,23,31) uint16 raw ids in [0,48) with frame 3 made of ids that map to -100 only (the reference's Evaluator
    returns early on such a frame); mapping (41,) int64, the nyu40 -> benchmark class table (-100 elsewhere); picked; logit (5,20,5,7)
    float32 with planted exact ties; seg_label_3d: three per-scene int64 arrays of nyu40 ids with some -100."""
    rs = np.random.RandomState(31)
    Ftot, H, W = FIX_STORE
    labels = rs.randint(0, 48, (Ftot, H, W)).astype(np.uint16)
    often = rs.random_sample((Ftot, H, W)) < 0.7  # most pixels carry a benchmark class
    labels[often] = np.array(EVAL_CLASS_IDS, np.uint16)[rs.randint(0, 20, int(often.sum()))]
    mapping = np.full(FIX_T, -100, np.int64)
    mapping[EVAL_CLASS_IDS] = np.arange(20)
    unmapped = np.array([i for i in range(48) if i >= FIX_T or mapping[i] < 0], np.uint16)
    labels[3] = unmapped[rs.randint(0, len(unmapped), (H, W))]
    w, h = FIX_SIZE
    logit = rs.standard_normal((len(FIX_PICKED), FIX_C, h, w)).astype(np.float32)
    logit[0, 7, :, 1] = logit[0, 3, :, 1] = 9.0    # a tie of classes 3 and 7 above the rest: 3 wins
    logit[1, :, 2, :] = 0.5                        # all classes equal: 0 wins
    logit[2, 19, 0, :] = logit[2, 18, 0, :] = 8.0  # the last two classes
    scenes = [rs.randint(0, 41, n).astype(np.int64) for n in (300, 1, 777)]
    scenes[0][::7] = -100
    return {'labels': labels, 'mapping': mapping, 'picked': np.array(FIX_PICKED, np.int64), 'logit': logit, 'seg_label_3d': scenes}

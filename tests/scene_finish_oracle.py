"""NumPy restatement of what mvp_ensemble_softmax_f32, mvp_label_confusion_i64 and mvp_pack_cloud_f32 compute (test infrastructure, never
imported by the product): the ensemble of mvpnet/ensemble.py:45-49 in the float32 arithmetic pinned in include/mvp_hip.h and in float64,
the evaluator's confusion matrix (mvpnet/evaluate_3d.py:25-40) and the 3D baselines' padded batches."""
import numpy as np

from tests import scene_ragged_oracle as RO

FIXTURE = dict(n=512, C=20, M=4, seed=7, scale=3.0)  # tests/golden/scene_finish.npz (make_scene_finish_golden.py)
EVAL_CLASS_IDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]


def fixture_inputs():
    """-> logits (M,n,C) float32, gt (n,) int64 raw ids with ignored (-100) and non-evaluation ids (0, 13, 40, 255) among them."""
    P = FIXTURE
    rs = np.random.RandomState(P['seed'])
    logits = (rs.randn(P['M'], P['n'], P['C']) * P['scale']).astype(np.float32)
    gt = rs.choice(np.array(EVAL_CLASS_IDS + [-100, 0, 13, 40, 255], np.int64), P['n'])
    return logits, gt


def ensemble(logits):
    """logits (M,n,C) float32 -> (prob32 (n,C) float32, label32, prob64 (n,C) float64, label64).  prob32 is the pinned expression: per
    model max, exp(x - max), the sum in class order, a division; the models added in order; the first maximum.  numpy.exp on float32 is
    not the device's expf bit for bit: prob32 shows where float32 arithmetic lands, prob64 is the yardstick."""
    logits = np.asarray(logits)
    assert logits.ndim == 3 and logits.dtype == np.float32
    M, n, C = logits.shape
    P32, P64 = None, None
    with np.errstate(invalid='ignore', over='ignore'):
        for m in range(M):
            x = logits[m]
            e = np.exp(x - np.max(x, axis=1, keepdims=True)).astype(np.float32)
            s = e[:, 0].copy()
            for c in range(1, C):
                s = (s + e[:, c]).astype(np.float32)
            p = (e / s[:, None]).astype(np.float32)
            P32 = p if P32 is None else (P32 + p).astype(np.float32)
            x64 = x.astype(np.float64)
            e64 = np.exp(x64 - np.max(x64, axis=1, keepdims=True))
            p64 = e64 / e64.sum(1, keepdims=True)
            P64 = p64 if P64 is None else P64 + p64
    return P32, np.argmax(P32, axis=1).astype(np.int64), P64, np.argmax(P64, axis=1).astype(np.int64)


def prob_bar(M, C):
    """|P - P64| bound: per model expf within 2 ulp, C - 1 additions, one division and the rounding of x - mx, all on values <= 1."""
    return M * (C + 8) * 2.0 ** -24


def decided(P64, bar):
    """rows whose two largest float64 probabilities differ by more than twice the bar"""
    top = np.sort(P64, axis=1)[:, ::-1]
    return (top[:, 0] - top[:, 1]) > 2 * bar if P64.shape[1] > 1 else np.ones(len(P64), bool)


def lut_of(labels):
    """value -> position table of an evaluator's labels (-1: not a label)"""
    labels = np.asarray(labels, np.int64)
    lut = np.full(int(labels.max()) + 1, -1, np.int32)
    lut[labels] = np.arange(len(labels), dtype=np.int32)
    return lut


def label_confusion(pred, gt, C, pred_lut=None, gt_lut=None):
    """-> (C,C) int64: += 1 at [position(gt)][position(pred)] where both are positions."""
    def position(v, lut):
        v = np.asarray(v, np.int64).reshape(-1)
        if lut is None:
            return np.where((v >= 0) & (v < C), v, -1)
        lut = np.asarray(lut)
        inside = (v >= 0) & (v < len(lut))
        q = np.where(inside, lut[np.clip(v, 0, len(lut) - 1)], -1).astype(np.int64)
        return np.where((q >= 0) & (q < C), q, -1)
    row, col = position(gt, gt_lut), position(pred, pred_lut)
    both = (row >= 0) & (col >= 0)
    return np.bincount(row[both] * C + col[both], minlength=C * C).reshape(C, C).astype(np.int64)


def pack_cloud(points, index, offsets, slot_base, out_len, colors=None, feature=None, seed=0):
    """-> (points_flat, feature_flat or None) float32: chunk c as a (3, out_len[c]) matrix at 3 * slot_base[c] and a (Cf, out_len[c]) matrix
    at Cf * slot_base[c]; floats no chunk covers stay NaN.  A slot's member is scene_ragged_oracle.pad_slots' for points and features alike."""
    points = np.asarray(points, np.float32)
    assert colors is None or feature is None
    src = None
    if colors is not None:
        src = np.asarray(colors, np.uint8).astype(np.float32) / np.float32(255.0)
    if feature is not None:
        src = np.asarray(feature, np.float32)
    slots = int(max(b + n for b, n in zip(slot_base, out_len))) if len(out_len) else 0
    out_p = np.full(3 * slots, np.nan, np.float32)
    out_f = None if src is None else np.full(src.shape[1] * slots, np.nan, np.float32)
    for c in range(len(out_len)):
        members = np.asarray(index[offsets[c]:offsets[c + 1]])
        choice = members[RO.pad_slots(len(members), out_len[c], seed, c)]
        out_p[3 * slot_base[c]:3 * (slot_base[c] + out_len[c])] = points[choice].T.reshape(-1)
        if src is not None:
            Cf = src.shape[1]
            out_f[Cf * slot_base[c]:Cf * (slot_base[c] + out_len[c])] = src[choice].T.reshape(-1)
    return out_p, out_f

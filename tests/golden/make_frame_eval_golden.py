"""Writes tests/golden/frame_eval.npz: the seeded inputs of tests/frame_eval_oracle.py::fixture_inputs and what PILLOW, the REFERENCE's
Evaluator and the arithmetic of its compute_label_weights.py give on them.

    python -m tests.golden.make_frame_eval_golden /path/to/the/reference/checkout

  labels (5,23,31) uint16, mapping (41,) int64, picked (5,) int64, logit (5,20,5,7) float32: the inputs (frame 3 maps to -100 only).
  nearest (5,5,7) uint16: `Image.fromarray(labels[picked[i]]).resize((7, 5), Image.NEAREST)` of the "I;16" images.
  confusion (20,20) int32: the matrix of the reference's `Evaluator(CLASS_NAMES)` (mvpnet/evaluate_3d.py, sklearn's confusion_matrix
      inside), fed as mvpnet/test_2d.py:113-118 feeds it: `torch.argmax(1)` of the logits and the mapped Pillow labels, batch_update per
      frame (a raw id past the mapping raises in the reference's loader; here it is ignored, -100).
  hist_2d (20,) int64, weights_2d (20,) float32: compute_2d_weights' loop over ALL five store frames at (7, 5) -- np.bincount(label[label
      != -100], minlength=20) summed in float64 -- and its last three lines.
  seg_label_3d (1078,) int64 with scene_offsets_3d (4,): three scenes of nyu40 ids (some -100); hist_3d (41,) int64, weights_3d (20,)
      float32: compute_3d_weights' loop (np.bincount(label, minlength=41) needs non-negative labels: the -100 are dropped first, as the
      device histogram drops them) and its last lines with VALID_CLASS_IDS.
The file is written with fixed zip time stamps: it regenerates byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

from tests import frame_eval_oracle as FO

HERE = os.path.dirname(os.path.abspath(__file__))


def save_npz(path, arrays):
    """np.savez_compressed with the members' time stamps fixed (numpy stamps them with the clock)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main(reference_root):
    import torch
    from PIL import Image
    sys.path.insert(0, reference_root)
    from mvpnet.evaluate_3d import Evaluator, CLASS_NAMES, EVAL_CLASS_IDS
    assert list(EVAL_CLASS_IDS) == FO.EVAL_CLASS_IDS
    fx = FO.fixture_inputs()
    labels, mapping, picked, logit = fx['labels'], fx['mapping'], fx['picked'], fx['logit']
    T = len(mapping)

    def loader_label(frame):  # scannet_2d.py:156, :167-168
        im = Image.fromarray(frame)
        assert im.mode == 'I;16', im.mode
        raw = np.asarray(im.resize(FO.FIX_SIZE, Image.NEAREST))
        return raw, np.where(raw < T, mapping[np.minimum(raw, T - 1)], -100).astype(np.int64)

    nearest = np.stack([loader_label(labels[r])[0] for r in picked])
    assert nearest.dtype == np.uint16 and nearest.shape == (len(picked), FO.FIX_SIZE[1], FO.FIX_SIZE[0])
    gt = np.stack([loader_label(labels[r])[1] for r in picked])
    pred = torch.from_numpy(logit).argmax(1).cpu().numpy()
    ev = Evaluator(CLASS_NAMES)
    ev.batch_update(pred, gt.copy())  # (the reference rewrites -100 in place)
    cm = ev.confusion_matrix
    assert cm.sum() > 0 and (cm == np.round(cm)).all() and (gt[4] < 0).all()

    label_weights = np.zeros(20)
    for frame in labels:  # compute_2d_weights, every frame of the small store
        label = loader_label(frame)[1].flatten()
        label_weights += np.bincount(label[label != -100], minlength=20)
    hist_2d = label_weights.astype(np.int64)
    label_weights = label_weights.astype(np.float32)
    label_weights = label_weights / np.sum(label_weights)
    weights_2d = 1 / np.log(1.2 + label_weights)

    label_weights = np.zeros(41)
    for label in fx['seg_label_3d']:  # compute_3d_weights
        label_weights += np.bincount(label[label >= 0], minlength=41)
    hist_3d = label_weights.astype(np.int64)
    label_weights = label_weights.astype(np.float32)[EVAL_CLASS_IDS]
    label_weights = label_weights / np.sum(label_weights)
    weights_3d = 1 / np.log(1.2 + label_weights)
    assert weights_2d.dtype == np.float32 and weights_3d.dtype == np.float32 and weights_3d.shape == (20,)

    offsets = np.concatenate([[0], np.cumsum([len(s) for s in fx['seg_label_3d']])]).astype(np.int64)
    path = os.path.join(HERE, 'frame_eval.npz')
    save_npz(path, {'labels': labels, 'mapping': mapping, 'picked': picked, 'logit': logit, 'nearest': nearest, 'confusion': cm.astype(np.int32),
                    'hist_2d': hist_2d, 'weights_2d': weights_2d, 'seg_label_3d': np.concatenate(fx['seg_label_3d']), 'scene_offsets_3d': offsets,
                    'hist_3d': hist_3d, 'weights_3d': weights_3d})
    print('wrote', path, os.path.getsize(path), 'bytes; pairs counted', int(cm.sum()), 'of', gt.size)


if __name__ == '__main__':
    main(sys.argv[1])

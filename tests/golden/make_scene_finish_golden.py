"""Writes tests/golden/scene_finish.npz: what the REFERENCE's scene finish gives on the seeded inputs of tests/scene_finish_oracle.py
(n = 512, C = 20, M = 4) -- the labels of the expression of mvpnet/ensemble.py:45-49 (the sum of scipy.special.softmax over the models,
argmax) and the confusion matrix that the reference's Evaluator class (mvpnet/evaluate_3d.py, sklearn's confusion_matrix inside) holds
after two updates: the ensemble's labels mapped to raw ids against the raw ground truth with labels = EVAL_CLASS_IDS, and the same pair
once more with the predictions rolled by one point.  Expected results only; the inputs come from the seed.

    python -m tests.golden.make_scene_finish_golden /path/to/the/reference/checkout
"""
import os
import sys

import numpy as np

from tests import scene_finish_oracle as FO


def main(reference_root):
    import scipy.special
    sys.path.insert(0, reference_root)
    from mvpnet.evaluate_3d import Evaluator, CLASS_NAMES, EVAL_CLASS_IDS
    assert list(EVAL_CLASS_IDS) == FO.EVAL_CLASS_IDS
    logits, gt = FO.fixture_inputs()
    prob = sum(scipy.special.softmax(logits[m], axis=1) for m in range(len(logits)))
    label = prob.argmax(1)
    scannet_to_nyu40 = np.array(EVAL_CLASS_IDS + [0])  # ensemble.py:9
    raw = scannet_to_nyu40[label]
    ev = Evaluator(CLASS_NAMES, EVAL_CLASS_IDS)
    ev.update(raw.copy(), gt.copy())           # (the reference rewrites -100 in place)
    ev.update(np.roll(raw, 1), gt.copy())
    cm = ev.confusion_matrix
    assert cm.sum() > 0 and (cm == np.round(cm)).all()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'scene_finish.npz')
    np.savez_compressed(path, label=label.astype(np.int16), confusion=cm.astype(np.int32))
    print('wrote', path, os.path.getsize(path), 'bytes; pairs counted', int(cm.sum()), 'of', 2 * len(gt))


if __name__ == '__main__':
    main(sys.argv[1])

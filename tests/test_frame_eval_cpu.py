"""Stage one's test, validation and class weights without a GPU: the NumPy oracle (tests/frame_eval_oracle.py) against Pillow, the
reference's Evaluator and the arithmetic of compute_label_weights.py (tests/golden/frame_eval.npz), metric.label_log_weights against the
same, and the argument checks and declarations of mvp_frame_confusion_f32 / mvp_label_histogram_u16 / mvp_label_histogram_i64.  No
kernel runs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import frame_eval_oracle as FO
from tests import resize_oracle as RO
from tests.conftest import GOLDEN, ROOT

NAMES = (('mvp_frame_confusion_f32', 22), ('mvp_label_histogram_u16', 15), ('mvp_label_histogram_i64', 5))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'frame_eval.npz'))


def same_bits(got, exp):
    return got.dtype == np.float32 and exp.dtype == np.float32 and got.shape == exp.shape and np.array_equal(got.view(np.uint32), exp.view(np.uint32))


# ---- the oracle is the reference -------------------------------------------------------------------------------------------------------
def test_fixture_inputs_come_from_the_seed(golden):
    fx = FO.fixture_inputs()
    for k in ('labels', 'mapping', 'picked', 'logit'):
        assert fx[k].dtype == golden[k].dtype and np.array_equal(fx[k], golden[k]), k
    assert np.array_equal(np.concatenate(fx['seg_label_3d']), golden['seg_label_3d'])
    assert np.array_equal(np.cumsum([0] + [len(s) for s in fx['seg_label_3d']]), golden['scene_offsets_3d'])


def test_oracle_labels_equal_pillow(golden):
    got = RO.prepare_labels(golden['labels'], golden['picked'], size=FO.FIX_SIZE)
    assert np.array_equal(got, golden['nearest'].astype(np.int64))
    assert int(golden['labels'].max()) >= FO.FIX_T  # ids past the mapping are in the store


def test_oracle_confusion_equals_the_reference_evaluator(golden):
    mat, pred = FO.frame_confusion(golden['logit'], golden['labels'], golden['picked'], size=FO.FIX_SIZE, mapping=golden['mapping'])
    assert mat.dtype == np.int64 and np.array_equal(mat, golden['confusion'].astype(np.int64)) and int(mat.sum()) > 100
    # the planted ties: the first maximum, torch.argmax's answer (the fixture's predictions are torch's)
    assert (pred[0, :, 1] == 3).all() and (pred[1, 2, :] == 0).all() and (pred[2, 0, :] == 18).all()
    assert np.array_equal(pred, torch.from_numpy(golden['logit']).argmax(1).numpy())
    # the frame that maps to -100 only adds nothing
    alone, _ = FO.frame_confusion(golden['logit'][4:], golden['labels'], golden['picked'][4:], size=FO.FIX_SIZE, mapping=golden['mapping'])
    assert int(alone.sum()) == 0


def test_oracle_histograms_equal_the_reference_counts(golden):
    h2 = FO.label_histogram(golden['labels'], 20, size=FO.FIX_SIZE, mapping=golden['mapping'])
    assert h2.dtype == np.int64 and np.array_equal(h2, golden['hist_2d'])
    h3 = FO.label_histogram(golden['seg_label_3d'], 41)
    assert np.array_equal(h3, golden['hist_3d']) and int(h3.sum()) < len(golden['seg_label_3d'])  # (the -100 dropped)
    off = golden['scene_offsets_3d']
    acc = None
    for a, b in zip(off[:-1], off[1:]):
        acc = FO.label_histogram(golden['seg_label_3d'][a:b], 41, out=acc)
    assert np.array_equal(acc, golden['hist_3d'])
    raw = FO.label_histogram(golden['labels'], 65536, picked=[1, 1])
    assert np.array_equal(raw, 2 * np.bincount(golden['labels'][1].ravel(), minlength=65536))


def test_oracle_weights_equal_the_reference_arithmetic(golden):
    assert same_bits(FO.label_log_weights(golden['hist_2d']), golden['weights_2d'])
    assert same_bits(FO.label_log_weights(golden['hist_3d'], FO.EVAL_CLASS_IDS), golden['weights_3d'])


# ---- the product's host arithmetic ---------------------------------------------------------------------------------------------------------
def test_label_log_weights_equals_the_fixture(golden):
    from mvpnet_amd import metric as M
    assert list(M.EVAL_CLASS_IDS) == FO.EVAL_CLASS_IDS
    assert same_bits(M.label_log_weights(golden['hist_2d']), golden['weights_2d'])
    assert same_bits(M.label_log_weights(torch.from_numpy(golden['hist_2d'])), golden['weights_2d'])
    assert same_bits(M.label_log_weights(torch.from_numpy(golden['hist_3d']), M.EVAL_CLASS_IDS), golden['weights_3d'])
    w = M.label_log_weights(golden['hist_2d'])
    assert (w > 0).all() and np.isfinite(w).all() and w.shape == (20,)
    # what np.savetxt writes is what config.build_loss_2d reads back
    assert torch.as_tensor(w).dtype == torch.float32


def test_summary_from_confusion_on_the_host(golden):
    """the expressions of the two meters: acc = trace / sum in Python floats, IoU in float32 tensors"""
    from mvpnet_amd import metric as M
    mat = torch.from_numpy(golden['confusion'].astype(np.int64))
    got = M.summary_from_confusion(mat)
    assert got['seg_acc'] == float(mat.diagonal().sum()) / int(mat.sum())
    iou = M.SegIoU(20)
    iou.mat = mat
    assert got['seg_iou'] == iou.global_avg or (np.isnan(got['seg_iou']) and np.isnan(iou.global_avg))
    assert np.isnan(M.summary_from_confusion(torch.zeros((3, 3), dtype=torch.int64))['seg_acc'])


def test_update_frames_needs_class_indices():
    from mvpnet_amd import metric as M
    logit = torch.zeros((1, 20, 2, 2))
    with pytest.raises(ValueError):
        M.DeviceEvaluator(M.CLASS_NAMES, M.EVAL_CLASS_IDS).update_frames(logit, None, None)
    with pytest.raises(ValueError):
        M.DeviceEvaluator(M.CLASS_NAMES[:3]).update_frames(logit, None, None)


def test_ops_refuse_host_tensors():
    import mvpnet_amd.ops as ops
    with pytest.raises(RuntimeError):
        ops.frame_confusion(torch.zeros(1, 3, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint16), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        ops.label_histogram(torch.zeros(2, 8, 8, dtype=torch.uint16), 20)
    with pytest.raises(RuntimeError):
        ops.label_histogram(torch.zeros(5, dtype=torch.int64), 41)


# ---- the library: declarations and argument checks ---------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    from mvpnet_amd import _lib
    lib = _lib.lib()
    with open(os.path.join(ROOT, 'include', 'mvp_hip.h')) as f:
        header = f.read()
    for name, count in NAMES:
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name]) == count and name in _lib.EXPORTS and hasattr(lib, name)
        decl = re.search(r'\bint ' + name + r'\(([^;]*)\);', header)
        assert decl is not None, name
        assert len(decl.group(1).split(',')) == count, name  # the header's parameter list and the ctypes signature agree
    assert '#define MVP_HISTOGRAM_MAX_BINS 65536' in header
    import mvpnet_amd.ops as ops
    from mvpnet_amd import metric, mvpnet2d, scene
    from mvpnet_amd.ops import frame_eval
    assert frame_eval.MAX_BINS == 65536
    for fn in (ops.frame_confusion, ops.label_histogram, metric.DeviceEvaluator.update_frames, metric.label_log_weights, metric.summary_from_confusion,
               mvpnet2d.test_frames_2d, mvpnet2d.validate_2d, scene.label_weights_2d, scene.label_weights_3d):
        assert callable(fn)


def test_argument_errors_do_not_launch():
    """Precondition failures return MVP_E* before any HIP call (safe without a GPU)."""
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    EINVAL, EUNSUPPORTED, ENULL = -1, -2, -3

    def conf(Nf=2, C=20, h=4, w=6, ld=None, labels=d, Ftot=3, H=8, W=6, picked=d, yi=d, xi=None, mapping=d, T=41, mat=d, pred=None, logit=d):
        ld = (C * h * w, h * w, w, 1) if ld is None else ld
        return lib.mvp_frame_confusion_f32(logit, Nf, C, h, w, *ld, labels, Ftot, H, W, picked, yi, xi, mapping, T, -100, mat, pred, None)

    assert conf(logit=None) == ENULL and conf(picked=None) == ENULL
    assert conf(labels=None, mat=None, pred=None) == ENULL           # an unlabelled split needs pred
    assert conf(logit=None, C=0) == ENULL                             # a null pointer outranks an invalid size
    for bad in (dict(Nf=0), dict(C=0), dict(h=0, yi=d), dict(w=0, xi=d), dict(Ftot=0), dict(H=0), dict(W=0, xi=d), dict(T=-1)):
        assert conf(**bad) == EINVAL, bad
    assert conf(yi=None) == EINVAL and conf(xi=d) == EINVAL           # a table exactly for a changed axis
    assert conf(h=8, yi=d) == EINVAL and conf(w=3, xi=None) == EINVAL
    assert conf(labels=None) == EINVAL and conf(mat=None, pred=d) == EINVAL  # labels and mat go together
    assert conf(C=1 << 16) == EUNSUPPORTED
    assert conf(H=1 << 16, W=1 << 15, xi=d) == EUNSUPPORTED and conf(h=1 << 16, w=1 << 15, xi=d) == EUNSUPPORTED
    assert conf(H=1 << 31) == EUNSUPPORTED
    assert conf(ld=(0, 1 << 30, 1, 1)) == EUNSUPPORTED and conf(ld=(0, 1 << 26, 1 << 28, 1)) == EUNSUPPORTED  # a logit frame spans < 2^30 elements
    assert conf(ld=(480, -1, 6, 1)) == EINVAL

    def hist(labels=d, Ftot=3, H=8, W=6, picked=d, Nf=2, h=4, w=6, yi=d, xi=None, mapping=d, T=41, nbins=20, out=d):
        return lib.mvp_label_histogram_u16(labels, Ftot, H, W, picked, Nf, h, w, yi, xi, mapping, T, nbins, out, None)

    for name in ('labels', 'picked', 'out'):
        assert hist(**{name: None}) == ENULL, name
    assert hist(out=None, nbins=0) == ENULL
    for bad in (dict(Nf=0), dict(nbins=0), dict(h=0), dict(w=0, xi=d), dict(Ftot=0), dict(H=0), dict(W=0, xi=d), dict(T=-1), dict(yi=None), dict(xi=d)):
        assert hist(**bad) == EINVAL, bad
    assert hist(nbins=65537) == EUNSUPPORTED and hist(H=1 << 16, W=1 << 15, xi=d) == EUNSUPPORTED

    assert lib.mvp_label_histogram_i64(None, 5, 41, d, None) == ENULL and lib.mvp_label_histogram_i64(d, 5, 41, None, None) == ENULL
    assert lib.mvp_label_histogram_i64(d, -1, 41, d, None) == EINVAL and lib.mvp_label_histogram_i64(d, 5, 0, d, None) == EINVAL
    assert lib.mvp_label_histogram_i64(d, 5, 65537, d, None) == EUNSUPPORTED and lib.mvp_label_histogram_i64(d, 1 << 40, 41, d, None) == EUNSUPPORTED
    assert lib.mvp_label_histogram_i64(d, 0, 41, d, None) == 0          # nothing to do: no launch

"""The scene finish without a GPU: the NumPy oracle of mvp_ensemble_softmax_f32 / mvp_label_confusion_i64 pinned against the libraries
the reference calls (scipy.special.softmax, sklearn's confusion_matrix) and against the committed reference fixture
(tests/golden/make_scene_finish_golden.py), the three new entry points in the signature table and the library, and their argument checks
(which return before any launch)."""
import ctypes

import numpy as np
import pytest

from tests import scene_finish_oracle as FO


def test_ensemble_oracle_equals_scipy_softmax_summed():
    softmax = pytest.importorskip('scipy.special').softmax
    logits, _ = FO.fixture_inputs()
    P32, l32, P64, l64 = FO.ensemble(logits)
    ref = sum(softmax(logits[m], axis=1) for m in range(len(logits)))       # float32, as ensemble.py:45-49 on saved float32 logits
    ref64 = sum(softmax(logits[m].astype(np.float64), axis=1) for m in range(len(logits)))
    bar = FO.prob_bar(*logits.shape[::2])
    assert np.abs(ref64 - P64).max() < 1e-14
    print('float32 oracle against float64: %.3e, scipy float32: %.3e, bar %.3e' % (np.abs(P32 - P64).max(), np.abs(ref - P64).max(), bar))
    assert np.abs(P32 - P64).max() <= bar and np.abs(ref - P64).max() <= bar
    ok = FO.decided(P64, bar)
    assert ok.mean() >= 0.99
    assert np.array_equal(l64, ref64.argmax(1)) and np.array_equal(l32[ok], ref.argmax(1)[ok]) and np.array_equal(l32[ok], l64[ok])


def test_ensemble_oracle_special_rows():
    x = np.zeros((2, 5, 4), np.float32)
    x[:, 0] = [1.0, 3.0, 3.0, 0.0]           # an exact tie in every model: the first maximum
    x[:, 1] = 2.5                            # an all-equal row
    x[0, 2, 3] = np.nan                      # one NaN
    x[:, 3] = [0.0, 1.0, 2.0, 5.0]
    x[1, 4, 1] = np.inf
    P32, l32, P64, l64 = FO.ensemble(x)
    assert l32.tolist() == [1, 0, 0, 3, 0] and l64.tolist() == l32.tolist()
    assert np.isnan(P32[2]).all() and np.isnan(P32[4]).all() and np.allclose(P32[1], 0.5)


def test_confusion_oracle_equals_sklearn():
    CM = pytest.importorskip('sklearn.metrics').confusion_matrix
    logits, gt = FO.fixture_inputs()
    ids = np.array(FO.EVAL_CLASS_IDS + [0])
    pred = ids[FO.ensemble(logits)[3]]
    pred[::17] = 0                                        # "no prediction" mapped to raw id 0
    rewritten = gt.copy()
    rewritten[rewritten == -100] = 20                     # evaluate_3d.py:32
    exp = CM(rewritten, pred, labels=FO.EVAL_CLASS_IDS)
    lut = FO.lut_of(FO.EVAL_CLASS_IDS)
    got = FO.label_confusion(pred, gt, 20, lut, lut)
    assert got.dtype == np.int64 and np.array_equal(got, exp) and 0 < got.sum() < len(gt)
    # without tables: positions are the values
    pos_pred, pos_gt = np.where(lut[np.clip(pred, 0, 39)] >= 0, lut[np.clip(pred, 0, 39)], 20), np.where((gt >= 0) & (gt < 40), lut[np.clip(gt, 0, 39)], -100)
    assert np.array_equal(FO.label_confusion(pos_pred, pos_gt, 20), exp)


def test_oracle_against_the_reference_fixture(golden):
    g = golden('scene_finish')
    P = FO.FIXTURE
    logits, gt = FO.fixture_inputs()
    assert logits.shape == (P['M'], P['n'], P['C']) and g['label'].shape == (P['n'],) and g['confusion'].shape == (P['C'], P['C'])
    P32, l32, P64, l64 = FO.ensemble(logits)
    ok = FO.decided(P64, FO.prob_bar(P['M'], P['C']))
    ref_label = g['label'].astype(np.int64)
    assert ok.mean() >= 0.99 and np.array_equal(l32[ok], ref_label[ok]) and np.array_equal(l64[ok], ref_label[ok])
    raw = np.array(FO.EVAL_CLASS_IDS + [0])[ref_label]
    lut = FO.lut_of(FO.EVAL_CLASS_IDS)
    cm = FO.label_confusion(raw, gt, P['C'], lut, lut) + FO.label_confusion(np.roll(raw, 1), gt, P['C'], lut, lut)
    assert np.array_equal(cm, g['confusion'].astype(np.int64))
    # the host evaluator of this build holds the same matrix
    from mvpnet_amd.metric import Evaluator, CLASS_NAMES
    ev = Evaluator(CLASS_NAMES, FO.EVAL_CLASS_IDS)
    ev.batch_update([raw, np.roll(raw, 1)], [gt, gt])
    assert np.array_equal(ev.confusion_matrix, g['confusion'])


def test_pack_cloud_oracle_extends_the_pack_oracle():
    from tests import scene_ragged_oracle as RO
    rs = np.random.RandomState(1)
    pts, col = rs.standard_normal((300, 3)).astype(np.float32), rs.randint(0, 256, (300, 3)).astype(np.uint8)
    lengths, out_len, slot_base = [1, 40, 64], [8, 64, 64], [128, 0, 64]
    index = np.concatenate([np.sort(rs.choice(300, n, replace=False)) for n in lengths]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    p, f = FO.pack_cloud(pts, index, offsets, slot_base, out_len, colors=col, seed=5)
    assert np.array_equal(p.view(np.uint32), RO.pack_chunks(pts, index, offsets, [3 * s for s in slot_base], out_len, seed=5).view(np.uint32))
    src = index[offsets[1]:offsets[2]][RO.pad_slots(40, 64, 5, 1)]
    assert np.array_equal(f[:3 * 64].reshape(3, 64), (col[src].astype(np.float32) / np.float32(255)).T) and f.dtype == np.float32
    assert FO.pack_cloud(pts, index, offsets, slot_base, out_len)[1] is None


def test_symbols_are_declared_and_exported():
    from mvpnet_amd import _lib
    lib = _lib.lib()
    for name, count in (('mvp_pack_cloud_f32', 18), ('mvp_ensemble_softmax_f32', 9), ('mvp_label_confusion_i64', 10)):
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name]) == count and name in _lib.EXPORTS and hasattr(lib, name)
    import mvpnet_amd.ops as ops
    from mvpnet_amd import metric, scene
    assert callable(ops.pack_cloud) and callable(ops.ensemble_softmax) and callable(ops.label_confusion)
    assert callable(scene.infer_scene_3d) and callable(scene.ensemble_scene) and callable(metric.DeviceEvaluator)


def test_argument_errors_do_not_launch():
    """Precondition failures return MVP_E* before any HIP call (safe without a GPU)."""
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)

    def ensemble(M=4, n=300, C=20, ld=None, table=None, prob=d, label=d):
        table = (ctypes.c_void_p * 9)(*([16] * 9)) if table is None else table
        ld_r, ld_c = (C, 1) if ld is None else ld
        return lib.mvp_ensemble_softmax_f32(table, M, n, C, ld_r, ld_c, prob, label, None)

    assert ensemble(C=0) == -1 and ensemble(n=-1) == -1 and ensemble(M=0) == -1 and ensemble(ld=(-20, 1)) == -1 and ensemble(ld=(20, -1)) == -1
    assert ensemble(M=9) == -2 and ensemble(C=65) == -2 and ensemble(n=1 << 31) == -2    # MVP_EUNSUPPORTED
    assert lib.mvp_ensemble_softmax_f32(None, 4, 300, 20, 20, 1, d, d, None) == -3 and ensemble(label=None) == -3
    holes = (ctypes.c_void_p * 9)(16, 16, None, 16, 16, 16, 16, 16, 16)
    assert ensemble(table=holes) == -3 and ensemble(M=2, table=holes, n=0) == 0             # (only the first M entries are looked at)
    assert ensemble(C=0, label=None) == -3                                                  # a null pointer outranks an invalid size
    assert ensemble(prob=None, n=0) == 0 and ensemble(n=0) == 0                             # prob is optional; nothing to do: no launch

    def confusion(n=300, C=20, Lp=40, Lg=40, pred=d, gt=d, plut=d, glut=d, mat=d):
        return lib.mvp_label_confusion_i64(pred, gt, n, C, plut, Lp, glut, Lg, mat, None)

    assert confusion(C=0) == -1 and confusion(n=-1) == -1 and confusion(Lp=-1) == -1
    assert confusion(plut=None) == -1 and confusion(Lg=0) == -1                             # a table comes with its length
    assert confusion(C=32769) == -2
    for name in ('pred', 'gt', 'mat'):
        assert confusion(**{name: None}) == -3, name
    assert confusion(C=0, mat=None) == -3
    assert confusion(n=0) == 0 and confusion(n=0, plut=None, Lp=0, glut=None, Lg=0) == 0

    one = (ctypes.c_int64 * 2)(3, 0)
    wide = (ctypes.c_int64 * 2)(8, 0)

    def pack(n=100, total=50, C=1, Cf=3, out_slots=64, lengths=one, out_len=wide, **ptrs):
        p = dict(points=d, colors=d, feature=None, index=d, offsets=d, slot_base=d, dev_out_len=d, out_points=d, out_feature=d)
        p.update(ptrs)
        return lib.mvp_pack_cloud_f32(p['points'], p['colors'], p['feature'], Cf, n, p['index'], total, p['offsets'], C, p['slot_base'],
                                      p['dev_out_len'], lengths, out_len, 0, p['out_points'], p['out_feature'], out_slots, None)

    assert pack(n=-1) == -1 and pack(n=0) == -1 and pack(total=0) == -1 and pack(C=-1) == -1 and pack(out_slots=-1) == -1
    assert pack(lengths=wide, out_len=one) == -1                                            # N_c >= n_c
    assert pack(lengths=(ctypes.c_int64 * 2)(0, 0)) == -1                                   # n_c >= 1
    assert pack(Cf=4) == -1 and pack(feature=d) == -1                                       # colours are 3 channels; one source at most
    assert pack(colors=None, feature=d, Cf=0) == -1
    assert pack(colors=None, feature=d, Cf=9) == -2 and pack(n=1 << 31) == -2             # MVP_EUNSUPPORTED
    assert pack(out_len=(ctypes.c_int64 * 2)(1 << 31, 0)) == -2
    for name in ('points', 'index', 'offsets', 'slot_base', 'dev_out_len', 'out_points', 'out_feature'):
        assert pack(**{name: None}) == -3, name
    assert pack(lengths=None) == -3 and pack(out_len=None) == -3 and pack(n=0, points=None) == -3
    assert pack(C=0) == 0 and pack(C=0, colors=None, out_feature=None, Cf=0) == 0          # no chunks: no launch; the feature is optional


def test_no_cpu_fallback_and_refusals():
    import torch
    import mvpnet_amd.ops as ops
    from mvpnet_amd import metric
    x = torch.zeros(5, 4)
    with pytest.raises(RuntimeError):
        ops.ensemble_softmax([x, x])
    with pytest.raises(RuntimeError):
        ops.ensemble_softmax([])
    with pytest.raises(RuntimeError):
        ops.label_confusion(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        ops.pack_cloud(torch.zeros(4, 3), torch.zeros(2, dtype=torch.int64), torch.tensor([0, 2]), [2], [0], [2])
    ev = metric.DeviceEvaluator(metric.CLASS_NAMES, metric.EVAL_CLASS_IDS)
    with pytest.raises(RuntimeError):                      # host arrays: metric.Evaluator exists for them
        ev.update(np.zeros(3, np.int64), np.zeros(3, np.int64))
    with pytest.raises(RuntimeError):
        ev.update(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    assert ev.confusion_matrix.shape == (20, 20) and ev.confusion_matrix.sum() == 0
    for bad in ([0, -1], [0.5, 1.0]):
        with pytest.raises(ValueError):
            metric.DeviceEvaluator(['a', 'b'], bad)
    with pytest.raises(ValueError):
        metric.DeviceEvaluator(['a', 'b'], [1, 2, 3])

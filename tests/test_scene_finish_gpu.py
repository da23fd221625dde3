"""The scene finish on the MI355X: mvp_ensemble_softmax_f32 against the float64 oracle in every layout it takes, its special rows,
mvp_label_confusion_i64 against the oracle, and metric.DeviceEvaluator against metric.Evaluator."""
import functools

import numpy as np
import pytest
import torch

from tests import scene_finish_oracle as FO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NS, MS = (1, 63, 64, 65, 257, 5000), (1, 4, 8)


def t(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)  # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _case(M, n, C):
    """The inputs of one shape and their oracle, computed once for all layouts (read-only)."""
    x = (np.random.RandomState(7).randn(M, n, C) * 3).astype(np.float32)
    P32, l32, P64, l64 = FO.ensemble(x)
    for a in (x, P64, l64):
        a.setflags(write=False)
    return x, P64, l64


def _lay(x, layout):
    """x (n,C) float32 -> a device tensor of that shape and content in the given memory layout"""
    n, C = x.shape
    if layout == 'rows':
        return t(x)
    if layout == 'transposed':            # the (C,n) network output, viewed as rows
        return t(x.T).t()
    if layout == 'padded':                # rows with a padded stride (a multiple of four floats: the 16-byte path stays open for C % 4 == 0)
        buf = torch.full((n, C + 4), float('nan'), device=DEV)
        buf[:, :C] = t(x)
        return buf[:, :C]
    assert layout == 'misaligned'         # the base pointer one float off 16-byte alignment
    buf = torch.empty(n * C + 1, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[1:] = t(x).reshape(-1)
    return buf[1:].view(n, C)


@pytest.mark.parametrize('layout', ['rows', 'transposed', 'padded', 'misaligned'])
@pytest.mark.parametrize('C', [1, 13, 20, 64])
def test_ensemble_equals_the_float64_oracle(C, layout):
    """|P - P64| <= M (C + 8) 2^-24 (derived: per model expf within 2 ulp, C - 1 additions, a division and the rounding of x - mx, on
    values <= 1); labels equal wherever the oracle's top two differ by more than twice that; at most 1 % of the rows left out."""
    import mvpnet_amd.ops as ops
    worst, left = 0.0, 0
    for M in MS:
        for n in NS:
            x, P64, l64 = _case(M, n, C)
            models = [_lay(x[m], layout) for m in range(M)]
            assert all(m.stride() == models[0].stride() and tuple(m.shape) == (n, C) for m in models)
            prob, label = ops.ensemble_softmax(models)
            assert prob.dtype == torch.float32 and tuple(prob.shape) == (n, C) and prob.is_contiguous() and label.dtype == torch.int64
            bar = FO.prob_bar(M, C)
            err = float(np.abs(prob.cpu().numpy().astype(np.float64) - P64).max())
            ok = FO.decided(P64, bar)
            worst, left = max(worst, err / bar), left + int((~ok).sum())
            print('C %d %s M %d n %d: max |P - P64| %.3e (bar %.3e), rows under the gap %d' % (C, layout, M, n, err, bar, int((~ok).sum())))
            assert err <= bar
            assert np.array_equal(label.cpu().numpy()[ok], l64[ok])
            assert int((~ok).sum()) <= n / 100
            label_only = ops.ensemble_softmax(models, want_prob=False)
            assert label_only[0] is None and torch.equal(label_only[1], label)
    print('C %d %s: worst error / bar %.3f, rows left out %d' % (C, layout, worst, left))


def test_ensemble_special_rows():
    """Exact ties go to the first maximum, an all-equal row gives 0, a NaN gives label 0 and an all-NaN prob row, infinite logits finish."""
    import mvpnet_amd.ops as ops
    M, n, C = 4, 70, 20
    x = (np.random.RandomState(3).randn(M, n, C) * 3).astype(np.float32)
    x[:, 0, :] = -1.0
    x[:, 0, 5] = x[:, 0, 11] = 4.0         # two classes with bit-equal logits in every model
    x[:, 1, :] = 0.75                      # all equal
    x[2, 2, 19] = np.nan                   # one NaN
    x[1, 3, 7] = np.inf
    x[:, 4, :] = -np.inf
    x[:, 5, 3] = -np.inf                   # a class no model can pick: probability 0, harmless
    x[:, 6, 0] = 9.0
    x[:, 6, 19] = 9.0                      # a tie between the first and the last lane's classes
    for layout in ('rows', 'transposed'):
        prob, label = ops.ensemble_softmax([_lay(x[m], layout) for m in range(M)])
        torch.cuda.synchronize()
        prob, label = prob.cpu().numpy(), label.cpu().numpy()
        _, l32, P64, l64 = FO.ensemble(x)
        assert label[0] == 5 and label[1] == 0 and label[2] == 0 and label[6] == 0
        assert np.isnan(prob[2]).all() and np.isnan(prob[3]).all() and np.isnan(prob[4]).all() and label[3] == 0 and label[4] == 0
        assert prob[0, 5] == prob[0, 11] and np.all(prob[1] == prob[1, 0]) and abs(prob[1, 0] - M / C) < 1e-6
        rest = np.arange(n) > 6
        rest[5] = True
        assert np.isfinite(prob[rest]).all() and np.abs(prob[rest] - P64[rest]).max() <= FO.prob_bar(M, C) and prob[5, 3] == 0
        ok = FO.decided(P64[rest], FO.prob_bar(M, C))
        assert np.array_equal(label[rest][ok], l64[rest][ok])
        assert label.min() >= 0 and label.max() < C


def test_ensemble_is_reproducible_and_takes_mixed_strides():
    import mvpnet_amd.ops as ops
    x, P64, l64 = _case(4, 5000, 20)
    models = [t(x[m]) for m in range(4)]
    a = ops.ensemble_softmax(models)
    b = ops.ensemble_softmax(models)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    mixed = [models[0], _lay(x[1], 'transposed'), _lay(x[2], 'padded'), _lay(x[3], 'misaligned')]
    assert len({m.stride() for m in mixed}) > 1
    c = ops.ensemble_softmax(mixed)   # (copied into the first one's strides: the same reads, the same bits)
    assert torch.equal(a[0].view(torch.int32), c[0].view(torch.int32)) and torch.equal(a[1], c[1])
    from mvpnet_amd.scene import ensemble_scene
    d = ensemble_scene(models)
    assert torch.equal(a[0].view(torch.int32), d[0].view(torch.int32)) and torch.equal(a[1], d[1])
    empty = ops.ensemble_softmax([torch.zeros((0, 20), device=DEV)])
    assert tuple(empty[0].shape) == (0, 20) and tuple(empty[1].shape) == (0,)
    for bad in ([models[0], models[1][:10]], [models[0].double()], [models[0]] * 9, [torch.zeros((4, 65), device=DEV)], [models[0][0]]):
        with pytest.raises(RuntimeError):
            ops.ensemble_softmax(bad)


def _labels(n, seed):
    rs = np.random.RandomState(seed)
    gt = rs.choice(np.array(FO.EVAL_CLASS_IDS + [-100, 0, 13, 40, 255], np.int64), n)
    pred = rs.choice(np.array(FO.EVAL_CLASS_IDS + [0, 41], np.int64), n)
    if n >= 5:
        gt[:5] = [-100, 0, 13, 40, 255]
    return pred, gt


@pytest.mark.parametrize('n', [1, 64, 65, 5000])
def test_confusion_equals_the_oracle(n):
    import mvpnet_amd.ops as ops
    lut = FO.lut_of(FO.EVAL_CLASS_IDS)
    pred, gt = _labels(n, n)
    mat = torch.zeros((20, 20), dtype=torch.int64, device=DEV)
    assert ops.label_confusion(t(pred), t(gt), mat, pred_lut=t(lut), gt_lut=t(lut)) is mat
    exp = FO.label_confusion(pred, gt, 20, lut, lut)
    assert np.array_equal(mat.cpu().numpy(), exp) and (n < 64 or 0 < exp.sum() < n)
    pred2, gt2 = _labels(n, n + 1)
    ops.label_confusion(t(pred2), t(gt2), mat, pred_lut=t(lut), gt_lut=t(lut))   # a second call accumulates on top
    assert np.array_equal(mat.cpu().numpy(), exp + FO.label_confusion(pred2, gt2, 20, lut, lut))
    # a table on one side only
    one = torch.zeros((20, 20), dtype=torch.int64, device=DEV)
    pos = np.where((pred >= 0) & (pred < len(lut)), lut[np.clip(pred, 0, len(lut) - 1)], -1).astype(np.int64)
    ops.label_confusion(t(pos), t(gt), one, gt_lut=t(lut))
    assert np.array_equal(one.cpu().numpy(), exp)
    # no tables: C = 64 fills the LDS table exactly (C*C = 4096), C = 65 is one past it (global atomics)
    for C in (64, 65):
        rs = np.random.RandomState(C + n)
        p, g = rs.randint(-2, C + 2, n).astype(np.int64), rs.randint(-2, C + 2, n).astype(np.int64)
        if n >= 4:
            g[:4], p[:4] = [-100, C, C - 1, 0], [0, 0, C - 1, C]
        m = torch.zeros((C, C), dtype=torch.int64, device=DEV)
        for _ in range(2):
            ops.label_confusion(t(p), t(g), m)
        assert np.array_equal(m.cpu().numpy(), 2 * FO.label_confusion(p, g, C))


def test_confusion_refusals():
    import mvpnet_amd.ops as ops
    mat = torch.zeros((20, 20), dtype=torch.int64, device=DEV)
    p = torch.zeros(8, dtype=torch.int64, device=DEV)
    for args, kw in (((p.int(), p, mat), {}), ((p, p[:4], mat), {}), ((p, p, mat.int()), {}), ((p, p, mat[:, :10]), {}),
                     ((p, p, mat), dict(pred_lut=p)), ((p, p, mat), dict(gt_lut=torch.zeros(0, dtype=torch.int32, device=DEV))),
                     ((p.cpu(), p, mat), {})):
        with pytest.raises(RuntimeError):
            ops.label_confusion(*args, **kw)
    assert int(mat.sum()) == 0


@pytest.mark.parametrize('labels', [None, FO.EVAL_CLASS_IDS])
def test_device_evaluator_equals_the_host_evaluator(labels, capsys):
    from mvpnet_amd.metric import DeviceEvaluator, Evaluator, CLASS_NAMES
    n, C = 5000, 20
    rs = np.random.RandomState(5)
    ids = np.arange(C) if labels is None else np.array(labels)
    dev_ev, host_ev = DeviceEvaluator(CLASS_NAMES, labels), Evaluator(CLASS_NAMES, labels)
    assert np.array_equal(dev_ev.confusion_matrix, host_ev.confusion_matrix)
    scenes = []
    for s in range(2):
        gt = ids[rs.randint(0, C, n)].astype(np.int64)
        pred = np.where(rs.rand(n) < 0.6, gt, ids[rs.randint(0, C, n)]).astype(np.int64)
        gt[rs.rand(n) < 0.2] = -100                                    # ignored ground truth
        pred[rs.rand(n) < 0.1] = C if labels is None else 0            # "no prediction": C, or raw id 0 after scannet_to_nyu40
        scenes.append((pred, gt))
    scenes.append((scenes[0][0], np.full(n, -100, np.int64)))          # a scene whose ground truth is all ignored: adds nothing
    dev_ev.update(t(scenes[0][0]), t(scenes[0][1]))
    host_ev.update(*scenes[0])
    dev_ev.batch_update([t(p) for p, _ in scenes[1:]], [t(g) for _, g in scenes[1:]])
    host_ev.batch_update([p for p, _ in scenes[1:]], [g for _, g in scenes[1:]])
    capsys.readouterr()
    cm = dev_ev.confusion_matrix
    assert cm.dtype == np.float64 and np.array_equal(cm, host_ev.confusion_matrix) and 0 < cm.sum() < 2 * n
    assert dev_ev.overall_acc == host_ev.overall_acc and dev_ev.overall_iou == host_ev.overall_iou
    np.testing.assert_array_equal(dev_ev.class_seg_acc, host_ev.class_seg_acc)
    np.testing.assert_array_equal(dev_ev.class_iou, host_ev.class_iou)
    # int32 labels (a cast, no refusal) and (B,N) shapes go in as Evaluator takes them
    dev_ev.update(t(scenes[1][0].astype(np.int32)).view(2, -1), t(scenes[1][1]).view(2, -1))
    host_ev.update(scenes[1][0].reshape(2, -1), scenes[1][1].reshape(2, -1))
    assert np.array_equal(dev_ev.confusion_matrix, host_ev.confusion_matrix)

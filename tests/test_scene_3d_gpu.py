"""The sliding-window test of the 3D baselines on the MI355X: mvp_pack_cloud_f32 against its NumPy oracle and against mvp_pack_chunks_f32,
scene.infer_scene_3d against the per-chunk path (scene2chunks_legacy, every chunk a batch of one padded to min_nb_pts, scene.infer_scene)
with and without colours, its edge cases, and the round trip through scene.ensemble_scene and metric.DeviceEvaluator."""
import functools

import numpy as np
import pytest
import torch

from tests import scene_finish_oracle as FO
from tests import scene_ragged_oracle as RO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CFG = dict(num_centroids=(256, 64, 16, 4), radius=(0.1, 0.2, 0.4, 0.8), max_neighbors=(32, 32, 32, 32))
SCENE = dict(n_pts=24000, min_nb_pts=1024, chunk_size=(1.5, 1.5), chunk_stride=1.0, chunk_thresh=300, chunk_margin=(0.2, 0.2))
PAD_SEED = 11


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_pack_cloud_equals_the_oracle():
    """The lengths and buckets of test_pack_equals_the_oracle (n_c = 1, n_c = N_c and N_c - n_c = 1 among them), two seeds; uint8 colours,
    float features of 1, 3 and 8 channels, and no feature; the points are the bits ops.pack_chunks writes."""
    import mvpnet_amd.ops as ops
    rs = np.random.RandomState(3)
    pts = rs.standard_normal((5000, 3)).astype(np.float32)
    col = rs.randint(0, 256, (5000, 3)).astype(np.uint8)
    feat = rs.standard_normal((5000, 8)).astype(np.float32)
    feat[::7, 0], feat[1::7, 1] = np.float32(-0.0), np.nan            # copied bit for bit
    lengths = [1, 1024, 1023, 700, 3000, 257, 64, 5000, 1]
    out_len = [64, 1024, 1024, 1024, 4096, 1536, 64, 5000, 1]
    index = np.concatenate([np.sort(rs.choice(5000, n, replace=False)) for n in lengths]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    slot_base, at = [0] * len(lengths), 0
    for c in np.argsort(out_len, kind='stable'):  # sorted by size, as the bucketed batches lie in their buffers
        slot_base[c], at = at, at + out_len[c]
    args = (t(pts), t(index), t(offsets), lengths, slot_base, out_len)
    for seed in (0, 2 ** 40 + 12345):
        plain = ops.pack_chunks(t(pts), t(index), t(offsets), lengths, [3 * s for s in slot_base], out_len, seed=seed)
        sources = [dict(colors=col), dict(), dict(feature=feat[:, :1]), dict(feature=feat[:, :3]), dict(feature=feat)]
        for src in sources:
            got_p, got_f = ops.pack_cloud(*args, seed=seed, **{k: t(v) for k, v in src.items()})
            exp_p, exp_f = FO.pack_cloud(pts, index, offsets, slot_base, out_len, seed=seed, **src)
            assert got_p.dtype == torch.float32 and got_p.numel() == 3 * at == exp_p.size and not np.isnan(exp_p).any()
            assert torch.equal(got_p.view(torch.int32), plain.view(torch.int32))
            assert np.array_equal(got_p.cpu().numpy().view(np.uint32), exp_p.view(np.uint32))
            if not src:
                assert got_f is None and exp_f is None
                continue
            Cf = 3 if 'colors' in src else src['feature'].shape[1]
            assert got_f.dtype == torch.float32 and got_f.numel() == Cf * at == exp_f.size
            assert np.array_equal(got_f.cpu().numpy().view(np.uint32), exp_f.view(np.uint32))
    # chunks 1, 2, 3 are one (B,3,N) batch and one (B,Cf,N) batch; a padded slot carries its source point's feature
    got_p, got_f = ops.pack_cloud(*args, seed=5, colors=t(col))
    b = slot_base[1]
    batch_p, batch_f = got_p[3 * b:3 * (b + 3 * 1024)].view(3, 3, 1024), got_f[3 * b:3 * (b + 3 * 1024)].view(3, 3, 1024)
    source = index[offsets[3]:offsets[4]][RO.pad_slots(700, 1024, 5, 3)]
    assert torch.equal(batch_p[2], t(pts[source]).t()) and torch.equal(batch_f[2], t(_over_255(col[source])).t())
    for bad in (dict(lengths=[0] + lengths[1:]), dict(out_len=[64, 1023] + out_len[2:]), dict(index=t(index).int()),
                dict(lengths=lengths[1:]), dict(index=torch.from_numpy(index)), dict(slot_base=[-1] + slot_base[1:]),
                dict(colors=t(col), feature=t(feat)), dict(colors=t(col).float()), dict(colors=t(col)[:10]), dict(feature=t(feat).double()),
                dict(feature=t(np.zeros((5000, 9), np.float32))), dict(feature=t(feat)[:, 0]), dict(colors=t(col).cpu())):
        kw = dict(points=t(pts), index=t(index), offsets=t(offsets), lengths=lengths, slot_base=slot_base, out_len=out_len)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.pack_cloud(**kw)


def _over_255(colors):
    """colors / 255 as scannet_3d.py:82 computes it: an IEEE float32 division (torch divides by a scalar through its reciprocal on the device)"""
    return np.asarray(colors, np.uint8).astype(np.float32) / np.float32(255.0)


def _model(in_channels):
    """The small PN2SSG with the fixtures' deterministic weights (tests/golden/weights.py: xavier-uniform layers, non-trivial BatchNorm
    statistics and biases).  PyTorch's default initialisation leaves this coordinate-only network with almost flat logits -- a spread of
    the order of 1e-3, so that several per cent of the points sit under the fixed 2e-4 top-two gap whatever computes them --; the bars
    below are about the two paths agreeing, so the comparator's logits have to be decisive."""
    from mvpnet_amd.pn2 import PN2SSG
    from tests.golden.weights import load_into
    model = PN2SSG(in_channels, 20, dropout_prob=0.0, **CFG)
    load_into(model, 101)
    return model.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _scene():
    from mvpnet_amd.synthetic import make_rgbd_scene
    pts = make_rgbd_scene(3, 2, n_pts=SCENE['n_pts'], h=30, w=40)['points'].astype(np.float32)
    col = np.random.RandomState(21).randint(0, 256, (len(pts), 3)).astype(np.uint8)
    return pts, col


@functools.lru_cache(maxsize=None)
def _run(with_color):
    """infer_scene_3d and the per-chunk comparator on the scene, once per variant -> (ours, theirs, number of chunks)."""
    from mvpnet_amd.chunks import scene2chunks_legacy
    from mvpnet_amd.scene import infer_scene, infer_scene_3d, plan_buckets
    pts_np, col_np = _scene()
    pts, col, feat = t(pts_np), t(col_np), t(_over_255(col_np))
    model = _model(3 if with_color else 0)
    kw = {k: SCENE[k] for k in ('chunk_size', 'chunk_stride', 'chunk_thresh', 'chunk_margin')}
    ours = infer_scene_3d(model, pts, col if with_color else None, min_nb_pts=SCENE['min_nb_pts'], batch_size=8, pad_seed=PAD_SEED, **kw)
    assert not model.training
    idx = scene2chunks_legacy(pts, kw['chunk_size'], kw['chunk_stride'], thresh=kw['chunk_thresh'], margin=kw['chunk_margin'])
    lengths = [int(i.numel()) for i in idx]
    batches, _ = plan_buckets(lengths, min_nb_pts=SCENE['min_nb_pts'], batch_size=8)
    assert len(idx) >= 6 and len(batches) < len(idx) and len({N for N, _ in batches}) > 1
    singles = []
    for c, ind in enumerate(idx):  # every chunk a batch of one, padded as transforms.Pad does: duplicates of its own points behind them
        choice = ind[t(RO.pad_slots(lengths[c], max(lengths[c], SCENE['min_nb_pts']), PAD_SEED, c))]
        b = {'points': pts[choice].t()[None].contiguous()}
        if with_color:
            b['feature'] = feat[choice].t()[None].contiguous()
        singles.append(b)
    theirs = infer_scene(model, singles, idx, len(pts_np))
    return ours, theirs, len(idx)


@pytest.mark.parametrize('with_color', [False, True])
def test_infer_scene_3d_equals_the_per_chunk_path(with_color):
    """The bars of test_bucketed_scene_equals_the_per_chunk_path: counts equal, mean logits within 1e-4, labels equal wherever the
    comparator's top-two gap is at least 2e-4, at most 1 % of the points left out, points without a vote carry label C on both sides."""
    (mean, label, cnt), (emean, elabel, ecnt), C = _run(with_color)
    n_pts = SCENE['n_pts']
    assert tuple(mean.shape) == (n_pts, 20) and mean.dtype == torch.float32 and label.dtype == torch.int64 and cnt.dtype == torch.int32
    assert torch.equal(cnt, ecnt)
    voted = ecnt > 0
    gap_logit = float((mean - emean).abs().max())
    top2 = emean.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) >= 2e-4
    left_out, unvoted = int((~decided).sum()), int((~voted).sum())
    changed = int((label != elabel).sum())
    print('3d chunks e2e (colours %s): chunks %d, max |mean logit difference| %.3e, points under the 2e-4 gap %d of %d (without a vote: %d), '
          'labels changed %d, median top-two gap %.3e' % (with_color, C, gap_logit, left_out, n_pts, unvoted, changed,
                                                          float((top2[:, 0] - top2[:, 1]).median())))
    assert torch.isfinite(mean).all() and int(voted.sum()) > n_pts // 2
    assert gap_logit <= 1e-4
    assert torch.equal(label[decided], elabel[decided]) and torch.equal(label[~voted], elabel[~voted])
    assert bool((label[~voted] == 20).all()) and bool((elabel[~voted] == 20).all())
    assert left_out <= n_pts // 100


def test_colours_reach_the_network():
    """float32 colours already divided by 255 give the bits the uint8 store gives; other colours give other logits."""
    from mvpnet_amd.scene import infer_scene_3d
    pts_np, col_np = _scene()
    kw = {k: SCENE[k] for k in ('chunk_size', 'chunk_stride', 'chunk_thresh', 'chunk_margin')}
    kw.update(min_nb_pts=SCENE['min_nb_pts'], batch_size=8, pad_seed=PAD_SEED)
    model = _model(3).train()
    mean = _run(True)[0][0]
    as_float = infer_scene_3d(model, t(pts_np), t(_over_255(col_np)), **kw)[0]
    assert model.training, 'the mode is restored'
    assert torch.equal(as_float.view(torch.int32), mean.view(torch.int32))
    other = infer_scene_3d(model, t(pts_np), t(255 - col_np), **kw)[0]
    assert float((other - mean).abs().max()) > 1e-3


def test_edges():
    from mvpnet_amd.scene import infer_scene_3d
    pts_np, col_np = _scene()
    pts = t(pts_np)

    class Refuses(torch.nn.Module):
        num_classes, in_channels = 20, 0

        def forward(self, batch):
            raise AssertionError('nothing goes through the model')

    mean, label, cnt = infer_scene_3d(Refuses(), pts, chunk_thresh=10 ** 6)   # no kept window
    assert tuple(mean.shape) == (len(pts_np), 20) and not mean.any() and bool((label == 20).all()) and not cnt.any()
    assert cnt.dtype == torch.int32 and label.dtype == torch.int64
    for kw in (dict(), dict(use_color=True)):
        m = Refuses()
        m.in_channels = 0 if kw else 3
        with pytest.raises(RuntimeError, match='colours'):
            infer_scene_3d(m, pts, None, **kw)                                 # a model that wants colours, called without any
    with pytest.raises(RuntimeError):
        infer_scene_3d(Refuses(), pts.cpu())
    m = Refuses()
    m.in_channels = 3
    with pytest.raises(RuntimeError):
        infer_scene_3d(m, pts, t(col_np)[:100])


def test_round_trip_through_ensemble_and_evaluator():
    """infer_scene_3d of two models -> ensemble_scene -> DeviceEvaluator, against the oracle's ensemble and metric.Evaluator on the host."""
    from mvpnet_amd.metric import DeviceEvaluator, Evaluator, CLASS_NAMES
    from mvpnet_amd.scene import ensemble_scene
    means = [_run(False)[0][0], _run(True)[0][0]]
    n = SCENE['n_pts']
    prob, label = ensemble_scene(means)
    P32, l32, P64, l64 = FO.ensemble(np.stack([m.cpu().numpy() for m in means]))
    bar = FO.prob_bar(2, 20)
    ok = FO.decided(P64, bar)
    unvoted = (_run(False)[0][2] == 0).cpu().numpy()
    got = label.cpu().numpy()
    print('round trip: max |P - P64| %.3e (bar %.3e), rows under the gap %d of %d (without a vote: %d)' % (
        np.abs(prob.cpu().numpy() - P64).max(), bar, int((~ok).sum()), n, int(unvoted.sum())))
    assert np.abs(prob.cpu().numpy() - P64).max() <= bar and np.array_equal(got[ok], l64[ok])
    assert (got[unvoted] == 0).all() and not ok[unvoted].any()   # zero logits in every model: an exact tie, class 0
    assert int((~ok & ~unvoted).sum()) <= n // 100
    gt = np.random.RandomState(4).randint(0, 20, n).astype(np.int64)
    gt[::9] = -100
    dev_ev, host_ev = DeviceEvaluator(CLASS_NAMES), Evaluator(CLASS_NAMES)
    dev_ev.update(label, t(gt))
    host_ev.update(np.where(ok, l64, got), gt)   # the oracle's labels; under the gap, where float32 may choose either, the device's
    assert np.array_equal(dev_ev.confusion_matrix, host_ev.confusion_matrix) and dev_ev.confusion_matrix.sum() == (gt >= 0).sum()
    assert dev_ev.overall_iou == host_ev.overall_iou and dev_ev.overall_acc == host_ev.overall_acc
    raw = torch.tensor(FO.EVAL_CLASS_IDS + [0], device=DEV)[label]                # scannet_to_nyu40[label]: plain indexing
    assert raw.min() >= 1 and set(raw.unique().tolist()) <= set(FO.EVAL_CLASS_IDS)

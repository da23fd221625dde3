"""Whole-scene voting on the MI355X: mvp_vote_nearest_f32 / ops.vote_nearest against the committed scikit-learn fixture and the NumPy
oracle (indices and sums bit-identical), adversarial geometry, scene.infer_scene_votes against the same result assembled by hand, and the
entry point inside a captured graph."""
import numpy as np
import pytest
import torch

from tests import scene_vote_oracle as VO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def fixture(golden):
    g = golden('scene_vote')
    return {k: g[k] for k in g.files}


def _logits(V, C, nb, seed):
    """(V,C,nb) float32 from a seeded CPU generator"""
    return torch.randn(V, C, nb, generator=torch.Generator().manual_seed(seed)).numpy()


def _finish(total, V):
    from mvpnet_amd import _lib as L
    n, C = total.shape
    cnt = torch.full((n,), V, dtype=torch.int32, device=DEV)
    mean = torch.empty_like(total)
    label = torch.empty(n, dtype=torch.int64, device=DEV)
    L.call('mvp_vote_finish_f32', total, L.ptr(total), L.ptr(cnt), n, C, L.ptr(mean), L.ptr(label))
    return mean, label


def _run(points, keys, logits, layout='rows'):
    """-> sum, nn, swept of ops.vote_nearest; layout 'rows': the logits as the transposed view of a contiguous (V,nb,C) tensor (what
    PN2SSG returns), 'planes': a contiguous (V,C,nb) tensor."""
    import mvpnet_amd.ops as ops
    lg = t(logits)
    if layout == 'rows':
        lg = lg.transpose(1, 2).contiguous().transpose(1, 2)
        assert not lg.is_contiguous() or lg.size(1) == 1 or lg.size(2) == 1
    swept = torch.zeros(1, dtype=torch.int32, device=DEV)
    total, nn = ops.vote_nearest(t(points), t(keys), lg, return_index=True, swept=swept)
    assert total.dtype == torch.float32 and tuple(total.shape) == (len(points), logits.shape[1])
    assert nn.dtype == torch.int64 and tuple(nn.shape) == (len(keys), len(points))
    return total, nn, int(swept.item())


def _check_exact(points, keys, logits, layout='rows'):
    total, nn, swept = _run(points, keys, logits, layout)
    etotal, enn = VO.propagate(points, keys, logits)
    assert np.array_equal(nn.cpu().numpy(), enn)
    assert np.array_equal(total.cpu().numpy(), etotal)
    return total, nn, swept


@pytest.mark.parametrize('layout', ['planes', 'rows'])
def test_fixture(fixture, layout):
    P = VO.FIXTURE
    pts = fixture['points']
    keys = pts[fixture['vote_inds'].astype(np.int64)]
    logits = _logits(P['V'], 20, P['nb'], 5)
    total, nn, swept = _run(pts, keys, logits, layout)
    assert np.array_equal(nn.cpu().numpy(), fixture['nn'].astype(np.int64))  # scikit-learn's ball tree
    etotal, enn = VO.propagate(pts, keys, logits)
    assert np.array_equal(total.cpu().numpy(), etotal)
    mean, label = _finish(total, P['V'])
    emean, elabel = VO.finish(etotal, P['V'])
    assert np.array_equal(mean.cpu().numpy(), emean) and np.array_equal(label.cpu().numpy(), elabel)
    assert swept == 0  # every query is certified by its 27 cells (tests/test_scene_vote_cpu.py)


@pytest.mark.parametrize('n,nb,V,C', [(1, 1, 1, 1), (17, 3, 2, 20), (4097, 255, 1, 20), (5000, 256, 4, 7), (3000, 2049, 2, 33), (2000, 32768, 1, 20), (500, 65536, 1, 20)])
def test_shapes(n, nb, V, C):
    """The smallest shape; tiny odd sizes; sweep only with n not a multiple of the 16 queries per workgroup; the smallest gridded cloud;
    more than two columns per lane; the reference's cloud size, its keys drawn WITH replacement from a 20 000-point room (duplicates:
    the lowest index wins); the largest cloud the entry point admits, 65536 keys of a 70 000-point room."""
    from mvpnet_amd import _lib as L
    rs = np.random.RandomState(n + nb)
    if nb >= 32768:
        room = VO.room_cloud(20000 if nb == 32768 else 70000, 31)
        pts = room[rs.choice(len(room), n, replace=False)]
        keys = room[rs.randint(0, len(room), (V, nb))]
    else:
        pts = VO.room_cloud(n, 30 + n % 7)
        keys = np.stack([pts[rs.choice(n, nb, replace=False)] for _ in range(V)])
    _, _, swept = _check_exact(pts, keys, _logits(V, C, nb, 6))
    gridded = L.lib().mvp_vote_nearest_workspace(V, nb) > 0
    assert gridded == (nb >= 256)
    if not gridded:
        assert swept == n * V


@pytest.mark.parametrize('step', [0.02, 0.015625])
def test_lattice_midpoints_take_the_lowest_index(step):
    """Keys on a lattice (in shuffled order), queries at the cells' midpoints: up to eight equidistant keys."""
    rs = np.random.RandomState(3)
    ijk = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing='ij'), -1).reshape(-1, 3)
    keys = (ijk[rs.permutation(len(ijk))].astype(np.float32) * np.float32(step))[None]
    mid = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    pts = ((mid * np.float32(step) + (mid + 1) * np.float32(step)) * np.float32(0.5)).astype(np.float32)
    d = VO.dist2(pts[:256], keys[0])
    assert ((d == d.min(1, keepdims=True)).sum(1) > 1).any(), 'the case has ties'
    _check_exact(pts, keys, _logits(1, 20, keys.shape[1], 7))


def test_padding_rule():
    """n < nb: the keys are the scene followed by copies of point 0 (the reference's np.zeros padding): every point is its own nearest key,
    point 0 with index 0 and not one of the copies."""
    n, nb = 1500, 2048
    pts = VO.room_cloud(n, 41)
    ind = np.concatenate([np.arange(n), np.zeros(nb - n, np.int64)])
    _, nn, _ = _check_exact(pts, pts[ind][None], _logits(1, 20, nb, 8))
    assert np.array_equal(nn.cpu().numpy()[0], np.arange(n))


def test_far_clusters_and_outside_queries_sweep():
    rs = np.random.RandomState(5)
    keys = np.concatenate([rs.rand(1024, 3), rs.rand(1024, 3) + np.array([6.0, 0.0, 0.0])]).astype(np.float32)
    keys = np.stack([keys, keys[rs.permutation(2048)]])
    gap = rs.rand(300, 3) * np.array([4.0, 1.0, 1.0]) + np.array([1.5, 0.0, 0.0])
    near = rs.rand(300, 3) * np.array([7.0, 1.0, 1.0])
    far = rs.rand(100, 3) + rs.choice([-50.0, 50.0], (100, 3))
    pts = np.concatenate([gap, near, far]).astype(np.float32)
    _, _, swept = _check_exact(pts, keys, _logits(2, 20, 2048, 9))
    assert 0 < swept < 2 * len(pts)
    assert swept == int(sum((~VO.certified(pts, k)).sum() for k in keys))  # the oracle's restatement of the rule, query by query


def test_identical_keys():
    rs = np.random.RandomState(6)
    keys = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (300, 1))[None]
    pts = np.concatenate([rs.standard_normal((200, 3)).astype(np.float32), keys[0, :1]])
    _, nn, _ = _check_exact(pts, keys, _logits(1, 20, 300, 10))
    assert (nn == 0).all()


def test_non_finite_rows_do_no_harm():
    """One NaN query row and one inf key: the call completes, every other row is exact, every index lies in [0, nb)."""
    rs = np.random.RandomState(7)
    pts = VO.room_cloud(2000, 43)
    keys = np.stack([pts[rs.choice(2000, 1024, replace=False)] for _ in range(2)])
    keys[0, 5, 1] = np.inf
    pts = pts.copy()
    pts[7] = np.nan
    logits = _logits(2, 20, 1024, 11)
    total, nn, _ = _run(pts, keys, logits)
    torch.cuda.synchronize()
    etotal, enn = VO.propagate(pts, keys, logits)
    ok = np.arange(2000) != 7
    nn, total = nn.cpu().numpy(), total.cpu().numpy()
    assert nn.min() >= 0 and nn.max() < 1024
    assert np.array_equal(nn[:, ok], enn[:, ok]) and np.array_equal(total[ok], etotal[ok])
    assert not (nn[0] == 5).any()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
CFG = dict(num_centroids=(256, 64, 16, 4), radius=(0.1, 0.2, 0.4, 0.8), max_neighbors=(32, 32, 32, 32))


def _model(in_channels):
    from mvpnet_amd.pn2 import PN2SSG
    torch.manual_seed(3)
    return PN2SSG(in_channels, 20, dropout_prob=0.0, **CFG).to(DEV).eval()


def _by_hand(model, pts, feat, vote_inds):
    """model(batch)['seg_logit'] to the CPU, then the oracle."""
    keys = pts[vote_inds]
    batch = {'points': t(keys).transpose(1, 2).contiguous()}
    if feat is not None:
        batch['feature'] = t(feat[vote_inds]).transpose(1, 2).contiguous()
    with torch.no_grad():
        logit = model(batch)['seg_logit'].cpu().numpy()
    total, _ = VO.propagate(pts, keys, logit)
    return VO.finish(total, len(vote_inds))


@pytest.mark.parametrize('n,with_feature', [(3000, False), (700, False), (3000, True)])
def test_infer_scene_votes(n, with_feature):
    from mvpnet_amd.scene import infer_scene_votes
    nb, V = 1024, 2
    pts = VO.room_cloud(n, 50, size=(2.0, 1.5, 1.0))
    feat = np.random.RandomState(9).rand(n, 3).astype(np.float32) if with_feature else None
    model = _model(3 if with_feature else 0)
    kw = dict(feature=None if feat is None else t(feat), nb_pts=nb, num_votes=V)
    mean, label, inds = infer_scene_votes(model, t(pts), generator=torch.Generator().manual_seed(12), **kw)
    assert tuple(mean.shape) == (n, 20) and tuple(label.shape) == (n,) and label.dtype == torch.int64
    assert tuple(inds.shape) == (V, nb) and inds.dtype == torch.int64
    inds_np = inds.cpu().numpy()
    if n >= nb:
        assert all(len(np.unique(r)) == nb for r in inds_np) and not np.array_equal(inds_np[0], inds_np[1])  # drawn without replacement
    else:
        assert all(np.array_equal(r, np.concatenate([np.arange(n), np.zeros(nb - n, np.int64)])) for r in inds_np)
    emean, elabel = _by_hand(model, pts, feat, inds_np)
    assert np.array_equal(mean.cpu().numpy(), emean) and np.array_equal(label.cpu().numpy(), elabel)
    assert int(label.min()) >= 0 and int(label.max()) < 20  # no "no prediction" class on this path
    # the same subsamples passed in reproduce the run; so does an equally seeded generator
    mean2, label2, inds2 = infer_scene_votes(model, t(pts), vote_inds=inds, **kw)
    assert torch.equal(mean2, mean) and torch.equal(label2, label) and torch.equal(inds2, inds)
    mean3, label3, inds3 = infer_scene_votes(model, t(pts), generator=torch.Generator().manual_seed(12), **kw)
    assert torch.equal(inds3, inds) and torch.equal(mean3, mean) and torch.equal(label3, label)
    # the model's mode comes back
    model.train()
    mean4, _, _ = infer_scene_votes(model, t(pts), vote_inds=inds, **kw)
    assert model.training and torch.equal(mean4, mean)
    model.eval()
    infer_scene_votes(model, t(pts), vote_inds=inds, **kw)
    assert not model.training


def test_vote_nearest_inside_a_captured_graph(fixture):
    """The entry point only enqueues two launches on the given stream: captured once and replayed on fresh input through the same static
    buffers it gives the eager result."""
    from mvpnet_amd import _lib as L
    P = VO.FIXTURE
    V, nb, n, C = P['V'], P['nb'], P['n'], 20
    pts_np = fixture['points']
    keys_np = pts_np[fixture['vote_inds'].astype(np.int64)]
    logits_np = _logits(V, C, nb, 13)
    pts, keys, lg = t(pts_np), t(keys_np), t(logits_np)
    total = torch.full((n, C), -1.0, dtype=torch.float32, device=DEV)
    nn = torch.full((V, n), -1, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(L.lib().mvp_vote_nearest_workspace(V, nb)), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.call('mvp_vote_nearest_f32', pts, L.ptr(pts), n, L.ptr(keys), V, nb, L.ptr(lg), lg.stride(0), lg.stride(2), lg.stride(1), C,
               L.ptr(total), L.ptr(nn), None, L.ptr(ws), ws.numel())
    for rep in range(2):
        total.fill_(-1.0)
        nn.fill_(-1)
        if rep == 1:  # other input through the same buffers: the votes in reverse order
            keys.copy_(t(keys_np[::-1]))
            lg.copy_(t(logits_np[::-1]))
        g.replay()
        torch.cuda.synchronize()
        order = slice(None, None, -1) if rep == 1 else slice(None)
        etotal, enn = VO.propagate(pts_np, keys_np[order], logits_np[order])
        assert np.array_equal(nn.cpu().numpy(), enn) and np.array_equal(total.cpu().numpy(), etotal)
        assert np.array_equal(enn, fixture['nn'][order].astype(np.int64))

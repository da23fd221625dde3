"""The lift backward as a gather on the MI355X (mvp_lift_backward_f32, ops.lift_gather_backward and the backward of ops.lift /
ops.lift_gather in the reproducible mode): BIT-equal to the sequential float32 loop of tests/lift_backward_oracle.py -- ascending edges,
one rounding per addition, a map that starts at +0.0 --, every element written, nothing else written, the same bits in every run."""
import numpy as np
import pytest
import torch

from tests import lift_backward_oracle as O
from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _run(grad, index, P):
    import mvpnet_amd.ops as ops
    out = ops.lift_gather_backward(t(grad), t(index), P)
    assert out.dtype == torch.float32 and tuple(out.shape) == (grad.shape[0], P, grad.shape[-1]) and out.is_contiguous()
    return out


def _assert_bit_equal(out, want):
    got = _bits(out).cpu().numpy()
    bad = np.argwhere(got != want.view(np.int32))
    assert len(bad) == 0, '{} elements differ from the oracle, the first at (chunk, pixel, channel) = {}'.format(len(bad), tuple(bad[0]))


# ---- 1. small mixed -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [8, 64, 20, 6])
def test_small_mixed(C):
    """C = 8, 64, 20 (MVPNet2D's logits): 16 bytes per lane; C = 6: one element per lane.  Indices in [-2, P + 2]."""
    grad, index, P, want = O.mixed_case(C)
    _assert_bit_equal(_run(grad, index, P), want)


# ---- 2. hot pixels --------------------------------------------------------------------------------------------------------------------
def test_hot_pixels():
    """Lists of 2000+ and of all 3000 edges of a chunk: rebuilt in order from the index.  The rows can tell a wrong order."""
    grad, index, P, want = O.hot_case()
    back = O.lift_backward(grad, index, P, descending=True)
    differs = (want.view(np.int32) != back.view(np.int32)).any(axis=2)
    assert differs[0, 7] and differs[1, 95], 'ascending and descending sums differ on the hot rows'
    _assert_bit_equal(_run(grad, index, P), want)


# ---- 3. P beyond one workgroup's counters -----------------------------------------------------------------------------------------------
WINDOW_SHAPES = [(57600, 2048, 3, 8), (384000, 4096, 5, 4)]   # 3 x 120 x 160 and 5 x 240 x 320 pixels


@pytest.mark.parametrize('P,N,k,C', WINDOW_SHAPES)
def test_more_pixels_than_one_workgroup_counts(P, N, k, C):
    grad, index, P, want = O.window_case(P, N, k, C)
    lengths = O.list_lengths(index, P)
    assert lengths.max() > 16 and (lengths == 1).any()
    _assert_bit_equal(_run(grad, index, P), want)


def test_every_way_a_list_is_ordered():
    """List lengths on both sides of every threshold of the build (registers up to 16, one wave up to 128, the ordered rebuild beyond),
    in the first, an inner and the last (partial) range of 8192 pixels, their edges interleaved at random; k = 1 and an odd edge count
    (the index is then read one entry per load); P is odd (the gather takes two pixels per lane)."""
    P, C = 20001, 4
    lengths = [1, 2, 3, 15, 16, 17, 18, 63, 64, 65, 127, 128, 129, 130, 300, 1025]
    rs = np.random.RandomState(3)
    ends = [0, 8191, 8192, 16383, 16384, P - 1]
    pixels = np.concatenate([ends, rs.choice(np.setdiff1d(np.arange(P), ends), 3 * len(lengths) - 6, replace=False)])
    index = np.repeat(pixels, np.tile(lengths, 3)[rs.permutation(len(pixels))])
    index = np.concatenate([index, [-1, P, -7, P + 5]])
    index = index[rs.permutation(len(index))].astype(np.int64).reshape(1, -1, 1)
    assert index.shape[1] % 2 == 1
    grad = O.gradients(rs, 1, index.shape[1], 1, C)
    _assert_bit_equal(_run(grad, index, P), O.lift_backward(grad, index, P))


# ---- 4. every element written, nothing else ---------------------------------------------------------------------------------------------
def _arena_call(grad, index, P, N=None):
    """The entry on operands carved out of a poisoned arena -> (arena, result)."""
    from mvpnet_amd import _lib as L
    B, n, k, C = grad.shape
    N = n if N is None else N
    a = Arena(DEV)
    a.inp('grad', t(grad)).inp('index', t(index), fill=0)
    a.scratch('ws', L.lib().mvp_lift_backward_workspace_bytes(B, P, N, k), dtype=torch.uint8)
    a.out('out', (B, P, C))
    a.build()
    L.call('mvp_lift_backward_f32', a['grad'], L.ptr(a['grad']), L.ptr(a['index']), B, P, C, N, k, L.ptr(a['ws']), L.ptr(a['out']))
    torch.cuda.synchronize()
    return a, a.result('out')


@pytest.mark.parametrize('C', [8, 6])
def test_no_edges_and_no_neighbours_give_a_map_of_positive_zeros(C):
    grad, index, P, _ = O.mixed_case(C)
    for kw, ix in ((dict(N=0), index), (dict(), np.full_like(index, -1))):
        a, out = _arena_call(grad, ix, P, **kw)
        assert a.check() == []
        assert not _bits(out).any(), 'every word is the bit pattern of +0.0f'


@pytest.mark.parametrize('C', [8, 64, 20, 6])
def test_the_entry_writes_only_its_output_and_workspace(C):
    grad, index, P, want = O.mixed_case(C)
    a, out = _arena_call(grad, index, P)
    assert a.check() == []   # guard bands intact, grad and index unchanged, no unwritten (NaN) element in the result
    _assert_bit_equal(out, want)


# ---- 5. the same bits every run -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['hot'] + WINDOW_SHAPES, ids=str)
def test_the_same_bits_in_every_run(case):
    import mvpnet_amd.ops as ops
    grad, index, P, want = O.hot_case() if case == 'hot' else O.window_case(*case)
    g, ix = t(grad), t(index)
    first = ops.lift_gather_backward(g, ix, P)
    for _ in range(4):
        assert torch.equal(_bits(ops.lift_gather_backward(g, ix, P)), _bits(first))
    _assert_bit_equal(first, want)


# ---- 6. through autograd --------------------------------------------------------------------------------------------------------------
NV, H, W = 2, 12, 16


def _inputs(B, nv, N, seed, h=H, w=W, n_frames=9):
    """B chunks of a synthetic RGB-D scene, as tests/test_lift_half_gpu.py builds them (the helper of tests/test_lift_store_gpu.py without
    the store): nv of its frames each (never the one with the lost pose), N of the scene's own points each."""
    from mvpnet_amd.synthetic import make_rgbd_scene
    sc = make_rgbd_scene(5, n_frames, n_pts=30000, h=h, w=w)
    rs = np.random.RandomState(seed)
    good = [f for f in range(n_frames) if np.isfinite(sc['pose'][f]).all()]
    sel = np.stack([rs.choice(good, nv, replace=False) for _ in range(B)])
    pts = np.stack([sc['points'][rs.choice(len(sc['points']), N, replace=False)] for _ in range(B)])
    cam = np.broadcast_to(sc['cam_matrix'][:3, :3], (B, nv, 3, 3)).astype(np.float32)
    kinv = np.broadcast_to(sc['kinv'], (B, nv, 3, 3)).astype(np.float32)
    return dict(depth=t(sc['depth_mm'][sel].astype(np.int16)), kinv=t(kinv), cam=t(cam), pose=t(sc['pose'][sel]), points=t(pts.astype(np.float32)))


@pytest.fixture
def reproducible():
    from mvpnet_amd import _lib as L
    old = L.set_deterministic(True)
    try:
        yield
    finally:
        L.set_deterministic(old)


@pytest.mark.parametrize('augmented', [False, True], ids=['plain', 'flip+rot'])
def test_the_backward_of_lift_and_lift_gather_is_the_oracle(augmented, reproducible):
    import mvpnet_amd.ops as ops
    B, N, k, C = 2, 256, 3, 8
    inp = _inputs(B, NV, N, seed=12)
    kw = {}
    if augmented:
        ang = np.array([0.7, -2.1])
        rot = np.zeros((B, 3, 3))
        rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang), 1.0
        kw = dict(flip=torch.tensor([[True, False], [False, True]], device=DEV), rot=t(rot))
    feat = torch.randn(B, NV, H, W, C, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
    gfeat, _, knn = ops.lift(feat, inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'], k=k, **kw)[:3]
    assert bool((knn >= 0).any()) and int(knn.max()) < NV * H * W
    if augmented:
        plain = ops.lift(feat.detach(), inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'], k=k)[2]
        assert not torch.equal(plain, knn), 'the flip acts: mirrored pixel ids'
    up = O.gradients(np.random.RandomState(5), B, N, k, C)
    gfeat.backward(t(up))
    want = O.lift_backward(up, knn.cpu().numpy(), NV * H * W)
    assert bool(want.any()) and tuple(feat.grad.shape) == (B, NV, H, W, C)
    _assert_bit_equal(feat.grad.view(B, NV * H * W, C), want)
    # ops.lift_gather with the indices given
    feat2 = feat.detach().clone().requires_grad_(True)
    gfeat2, _ = ops.lift_gather(feat2, None, knn)
    assert torch.equal(_bits(gfeat2.detach()), _bits(gfeat.detach()))
    gfeat2.backward(t(up))
    _assert_bit_equal(feat2.grad.view(B, NV * H * W, C), want)


# ---- 7. the model ---------------------------------------------------------------------------------------------------------------------
def test_a_trainable_feature_map_gets_the_same_gradient_bits_twice(reproducible):
    """A tiny MVPNet3D whose 2D network is a stub that hands out a Parameter as the (B * nv, C, h, w) map: in the reproducible mode two
    forward + backward passes from the same state give bit-equal gradients of the map and of every 3D parameter."""
    from mvpnet_amd.pn2 import PN2SSG
    from mvpnet_amd.mvpnet3d import MVPNet3D, SegLoss
    B, N, C = 2, 256, 16

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.map = torch.nn.Parameter(torch.randn(B * NV, C, H, W, generator=torch.Generator().manual_seed(2)))

        def forward(self, data):
            return {'feature': self.map}

    torch.manual_seed(3)
    cfg = dict(num_centroids=(128, 32, 8, 4), radius=(0.2, 0.4, 0.8, 1.6), max_neighbors=(32, 32, 32, 32))
    model = MVPNet3D(Stub(), '', PN2SSG(C, 20, dropout_prob=0.0, **cfg), in_channels=C, mlp_channels=(16, 16, 16)).to(DEV).train()
    inp = _inputs(B, NV, N, seed=31)
    label = torch.randint(0, 20, (B, N), generator=torch.Generator().manual_seed(4)).to(DEV)
    batch = {'images': torch.zeros(B, NV, 3, H, W, device=DEV), 'points': inp['points'].transpose(1, 2).contiguous(), 'seg_label': label,
             'depth': inp['depth'], 'cam_matrix': inp['cam'], 'kinv': inp['kinv'], 'pose': inp['pose'], 'k': 3}
    loss_fn = SegLoss()

    def grads():
        model.zero_grad(set_to_none=True)
        loss_fn(model(dict(batch)), batch)['seg_loss'].backward()
        torch.cuda.synchronize()
        return {name: p.grad.detach().clone() for name, p in model.named_parameters() if p.grad is not None}

    first, second = grads(), grads()
    assert 'net_2d.map' in first and bool(first['net_2d.map'].any()) and bool(torch.isfinite(first['net_2d.map']).all())
    assert sum(name.startswith('net_3d.') for name in first) > 0 and first.keys() == second.keys()
    bad = [name for name in first if not torch.equal(_bits(first[name]), _bits(second[name]))]
    assert not bad, 'gradients that differ between two passes from the same state: {}'.format(bad)

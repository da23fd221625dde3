"""ops.lift_store (mvp_lift_store_f32) on the MI355X: the fused lifting reading its feature rows from a store shared by all chunks
through a (B,nv) slot table, against ops.lift on the materialised copy store[view_slot] -- bit for bit --, the zero rows of slots outside
the store, the memory one call takes, and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
H, W, FRAMES = 30, 40, 9


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_SCENES = {}


def _scene(h, w, n_frames, n_pts):
    from mvpnet_amd.synthetic import make_rgbd_scene
    key = (h, w, n_frames, n_pts)
    if key not in _SCENES:
        _SCENES[key] = make_rgbd_scene(5, n_frames, n_pts=n_pts, h=h, w=w)
    return _SCENES[key]


def _inputs(B, nv, N, C, U, depth_kind, seed, h=H, w=W, n_frames=FRAMES, box=False):
    """B chunks of a synthetic RGB-D scene: nv of its frames each (never the one with the lost pose), N of the scene's own points each, a
    random store of U < B * nv maps and a slot table that repeats slots across chunks and inside chunk 0."""
    sc = _scene(h, w, n_frames, 30000)
    rs = np.random.RandomState(seed)
    good = [f for f in range(n_frames) if np.isfinite(sc['pose'][f]).all()]
    sel = np.stack([rs.choice(good, nv, replace=False) for _ in range(B)])
    pts = np.stack([sc['points'][rs.choice(len(sc['points']), N, replace=False)] for _ in range(B)])
    depth = sc['depth_mm'][sel]
    depth = t(depth.astype(np.int16)) if depth_kind == 'int16' else t(depth.astype(np.float32) / np.float32(1000.))
    cam = np.broadcast_to(sc['cam_matrix'][:3, :3], (B, nv, 3, 3)).astype(np.float32)
    kinv = np.broadcast_to(sc['kinv'], (B, nv, 3, 3)).astype(np.float32)
    assert U < B * nv
    slot = rs.randint(0, U, (B, nv)).astype(np.int32)
    slot[0, 1] = slot[0, 0]
    slot[B - 1, 0] = slot[0, 0]
    store = torch.from_numpy(rs.standard_normal((U, h, w, C)).astype(np.float32)).to(DEV)
    out = dict(store=store, view_slot=t(slot), depth=depth, kinv=t(kinv), cam=t(cam), pose=t(sc['pose'][sel]), points=t(pts.astype(np.float32)))
    if box:  # a pixel box inside each chunk's points: pixels outside it fall out of the search; chunk 0's box holds no pixel at all
        lo, hi = np.percentile(pts[:, :, :2], 10, axis=1), np.percentile(pts[:, :, :2], 90, axis=1)
        lo[0], hi[0] = 100.0, 100.5
        out['box'] = t(np.concatenate([lo, hi], 1).astype(np.float32))
    return out


def _both(inp, k):
    import mvpnet_amd.ops as ops
    args = (inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'])
    got = ops.lift_store(inp['store'], inp['view_slot'], *args, k=k, box=inp.get('box'))
    want = ops.lift(inp['store'][inp['view_slot'].long()], *args, k=k, box=inp.get('box'))
    return got, want


def _assert_bit_equal(got, want):
    for name, a, b in zip(('gfeat', 'gxyz', 'knn_indices'), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert not any(x.requires_grad for x in got)


# B, nv, N, C, k, depth, U, box: one-wave workgroups with the `B < 8` placement and N no multiple of 64 (k = 1, 3, 8: the narrowest, the
# model's and the widest instance); 9 * ceil(29000 / 256) = 1026 >= 1024 workgroups: the 256-thread shape, XCD placement with B % 8 != 0
# (surplus workgroups exit); another channel width and k, float32 depth, a pixel box.
CASES = [(2, 3, 300, 64, 3, 'int16', 4, False), (2, 3, 300, 64, 1, 'int16', 4, False), (2, 3, 300, 64, 8, 'int16', 4, False),
         (9, 3, 29000, 64, 3, 'int16', 11, False), (3, 5, 1000, 8, 5, 'float32', 7, True)]


@pytest.mark.parametrize('B,nv,N,C,k,depth_kind,U,box', CASES)
def test_bit_equal_to_lift_on_the_materialised_copy(B, nv, N, C, k, depth_kind, U, box):
    got, want = _both(_inputs(B, nv, N, C, U, depth_kind, seed=B * 100 + k, box=box), k)
    _assert_bit_equal(got, want)
    gfeat, gxyz, knn = got
    assert tuple(gfeat.shape) == (B, N, k, C) and tuple(gxyz.shape) == (B, N, k, 3) and tuple(knn.shape) == (B, N, k) and knn.dtype == torch.int64
    found = knn >= 0
    assert bool(found.any()) and int(knn.max()) < nv * H * W
    assert bool(gfeat[found].abs().sum(-1).gt(0).all()), 'a found neighbour has its store row'
    if box:
        assert not found[0].any() and bool(found[1:].any()), 'chunk 0 has no valid pixel: every neighbour is missing'
        assert not gfeat[~found].any() and not gxyz[~found].any()


def test_slots_outside_the_store_give_zero_rows():
    import mvpnet_amd.ops as ops
    B, nv, N, C, k, U = 2, 3, 300, 64, 3, 4
    inp = _inputs(B, nv, N, C, U, 'int16', seed=42)
    args = (inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'])
    gfeat, gxyz, knn = ops.lift_store(inp['store'], inp['view_slot'], *args, k=k)
    bad = inp['view_slot'].clone()
    bad[0, 2], bad[1, 0] = -1, U
    bfeat, bxyz, bknn = ops.lift_store(inp['store'], bad, *args, k=k)
    assert torch.equal(bknn, knn) and torch.equal(bxyz, gxyz)
    view = torch.div(knn, H * W, rounding_mode='floor')  # (-1 for a missing neighbour)
    hit = torch.zeros_like(knn, dtype=torch.bool)
    hit[0], hit[1] = view[0] == 2, view[1] == 0
    assert int(hit[0].sum()) > 0 and int(hit[1].sum()) > 0, 'both views own neighbours'
    assert not bfeat[hit].any() and bool(gfeat[hit].any())
    assert torch.equal(bfeat[~hit], gfeat[~hit])


def test_one_call_allocates_no_copy_of_the_feature_maps():
    import mvpnet_amd.ops as ops
    B, nv, h, w, C, N, k, U = 8, 3, 120, 160, 64, 512, 3, 6
    replaced = B * nv * h * w * C * 4
    assert replaced == 117964800
    inp = _inputs(B, nv, N, C, U, 'int16', seed=3, h=h, w=w, n_frames=5)
    args = (inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = ops.lift_store(inp['store'], inp['view_slot'], *args, k=k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print('peak allocation of one lift_store call: %d bytes (the (B,nv,h,w,C) tensor it replaces: %d)' % (peak, replaced))
    assert peak < replaced // 2 == 58982400  # (what it must allocate is ~12 MB: search records, depth plane, outputs)
    assert bool((out[2] >= 0).any())


def test_refusals():
    import mvpnet_amd.ops as ops
    B, nv, N, C, k, U = 2, 3, 300, 64, 3, 4
    inp = _inputs(B, nv, N, C, U, 'int16', seed=1)

    def call(**change):
        a = dict(inp, **change)
        return ops.lift_store(a['store'], a['view_slot'], a['depth'], a['kinv'], a['cam'], a['pose'], a['points'], k=k)

    call()
    for change in (dict(store=inp['store'].double()), dict(view_slot=inp['view_slot'].long()), dict(points=inp['points'].double()),
                   dict(depth=inp['depth'].int()), dict(pose=inp['pose'].double()),
                   dict(view_slot=inp['view_slot'][:, :2]), dict(view_slot=inp['view_slot'].reshape(-1)), dict(view_slot=inp['view_slot'][:1]),
                   dict(store=inp['store'].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)),   # (U,h,w,C) shape, channel-major memory
                   dict(store=inp['store'][:, :, :W - 1]),                                          # another map size
                   dict(store=inp['store'].cpu()), dict(view_slot=inp['view_slot'].cpu()), dict(points=inp['points'].cpu()),
                   {key: v.cpu() for key, v in inp.items()}):
        with pytest.raises(RuntimeError):
            call(**change)

"""Lifting from bfloat16 / float16 feature maps and stores on the MI355X (mvp_lift_h16, mvp_lift_aug_h16, mvp_lift_store_h16,
mvp_lift_gather_h16): the rows are widened inside the gather, and widening is exact, so every result must be BIT-equal to today's float32
op on the widened copy.  The widened copy is made on the host (`feature.cpu().float()`), independent of the kernels under test, and the
features carry the 16-bit patterns a widening can get wrong: both zeros, the smallest and the largest subnormal of each sign, +-max
finite, +-inf (no NaN)."""
import numpy as np
import pytest
import torch

from tests.arena import Arena
from tests.test_lift_store_gpu import H, W, _inputs
from tests.test_scene_prep_gpu import E2E, _Feature2D, _model as _prep_model

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
DTYPES = [torch.bfloat16, torch.float16]
# +0, -0, smallest / largest subnormal of each sign, +-max finite; +-inf
PATTERNS = {torch.bfloat16: ([0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x7F7F, 0xFF7F], [0x7F80, 0xFF80]),
            torch.float16: ([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF], [0x7C00, 0xFC00])}


def _i16(bits):
    return torch.tensor([b - 65536 if b >= 32768 else b for b in bits], dtype=torch.int16)


def _half_feature(shape, dtype, seed):
    """randn rounded to `dtype`; channel 0 of pixel p (flat over the leading dimensions) = pattern p % 8, channel 1 = +-inf by p % 2."""
    feat = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)
    bits = feat.view(torch.int16).view(-1, shape[-1])
    p = torch.arange(bits.size(0))
    eight, inf = PATTERNS[dtype]
    bits[:, 0] = _i16(eight)[p % 8]
    bits[:, 1] = _i16(inf)[p % 2]
    assert not torch.isnan(feat.float()).any()
    return feat.to(DEV)


def _widened(feat):
    """The exactly widened float32 copy, made on the host."""
    return feat.cpu().float().to(DEV)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _assert_bit_equal(got, want, names=('gfeat', 'gxyz', 'knn_indices')):
    assert len(got) == len(want)
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b), name
    assert got[0].dtype == torch.float32 and not any(x.requires_grad for x in got)


def _assert_every_pattern_gathered(gfeat, found, dtype):
    """At least one gathered row (of a found neighbour) carries each of the eight patterns in channel 0 and each infinity in channel 1."""
    eight, inf = PATTERNS[dtype]
    rows = _bits(gfeat)[found]
    for channel, patterns in ((0, eight), (1, inf)):
        want = _bits(_i16(patterns).view(dtype).float())
        for pattern, w in zip(patterns, want.tolist()):
            assert bool((rows[:, channel] == w).any()), 'no gathered row carries the pattern 0x%04X' % pattern


# ---- 1. ops.lift ----------------------------------------------------------------------------------------------------------------------
# B, nv, N, C, k, depth, box: one-wave workgroups with the `B < 8` placement and N no multiple of 64 (k = 1, 3, 8); 9 * ceil(29000 / 256) =
# 1026 >= 1024 workgroups: the 256-thread shape, XCD placement with B % 8 != 0; float32 depth with a pixel box whose chunk 0 sees no pixel
# (all of its rows zero); the narrowest row (C = 4: 8 bytes, one lane)
LIFT_CASES = [(2, 3, 300, 64, 1, 'int16', False), (2, 3, 300, 64, 3, 'int16', False), (2, 3, 300, 64, 8, 'int16', False),
              (9, 3, 29000, 64, 3, 'int16', False), (3, 5, 1000, 8, 5, 'float32', True), (2, 3, 300, 4, 3, 'int16', False)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,nv,N,C,k,depth_kind,box', LIFT_CASES)
def test_lift_is_bit_equal_to_the_float32_lift_on_the_widened_copy(B, nv, N, C, k, depth_kind, box, dtype):
    import mvpnet_amd.ops as ops
    inp = _inputs(B, nv, N, 4, 2, depth_kind, seed=B * 100 + k, box=box)
    args = (inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'])
    feat = _half_feature((B, nv, H, W, C), dtype, seed=C + k)
    got = ops.lift(feat, *args, k=k, box=inp.get('box'))
    want = ops.lift(_widened(feat), *args, k=k, box=inp.get('box'))
    _assert_bit_equal(got, want)
    gfeat, _, knn = got
    assert tuple(gfeat.shape) == (B, N, k, C)
    found = knn >= 0
    _assert_every_pattern_gathered(gfeat, found, dtype)
    if box:
        assert not found[0].any() and bool(found[1:].any()), 'chunk 0 has no valid pixel: every neighbour is missing'
        assert not _bits(gfeat)[~found].any(), 'a missing neighbour is a row of +0'


@pytest.mark.parametrize('dtype', DTYPES)
def test_lift_with_flip_and_rotation(dtype):
    """The `_aug` entry: mirrored views index the feature map in mirrored order, the rotation acts on the gathered xyz and the points."""
    import mvpnet_amd.ops as ops
    B, nv, N, C, k = 2, 3, 300, 64, 3
    inp = _inputs(B, nv, N, 4, 2, 'int16', seed=77)
    args = (inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'])
    flip = torch.tensor([[True, False, True], [False, True, False]], device=DEV)
    ang = np.array([0.7, -2.1])
    rot = np.zeros((B, 3, 3))
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang), 1.0
    rot = torch.from_numpy(rot).to(DEV)
    feat = _half_feature((B, nv, H, W, C), dtype, seed=5)
    got = ops.lift(feat, *args, k=k, flip=flip, rot=rot, return_image_xyz=True)
    want = ops.lift(_widened(feat), *args, k=k, flip=flip, rot=rot, return_image_xyz=True)
    _assert_bit_equal(got, want, ('gfeat', 'gxyz', 'knn_indices', 'image_xyz', 'image_mask', 'points_rot'))
    plain = ops.lift(feat, *args, k=k)
    assert not torch.equal(got[2], plain[2]) and not torch.equal(got[1], plain[1]), 'the flip and the rotation act'
    _assert_every_pattern_gathered(got[0], got[2] >= 0, dtype)


# ---- 2. ops.lift_store ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_lift_store_is_bit_equal_to_lift_on_the_widened_materialised_copy(dtype):
    import mvpnet_amd.ops as ops
    B, nv, N, C, k, U = 2, 3, 300, 64, 3, 4
    inp = _inputs(B, nv, N, C, U, 'int16', seed=42)
    args = (inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'])
    store = _half_feature((U, H, W, C), dtype, seed=9)
    got = ops.lift_store(store, inp['view_slot'], *args, k=k)
    want = ops.lift(_widened(store)[inp['view_slot'].long()], *args, k=k)
    _assert_bit_equal(got, want)
    gfeat, gxyz, knn = got
    _assert_every_pattern_gathered(gfeat, knn >= 0, dtype)
    # slots -1 and U: zero rows, everything else unchanged
    bad = inp['view_slot'].clone()
    bad[0, 2], bad[1, 0] = -1, U
    bfeat, bxyz, bknn = ops.lift_store(store, bad, *args, k=k)
    assert torch.equal(bknn, knn) and torch.equal(bxyz, gxyz)
    view = torch.div(knn, H * W, rounding_mode='floor')
    hit = torch.zeros_like(knn, dtype=torch.bool)
    hit[0], hit[1] = view[0] == 2, view[1] == 0
    assert int(hit[0].sum()) > 0 and int(hit[1].sum()) > 0, 'both views own neighbours'
    assert not _bits(bfeat)[hit].any() and bool(_bits(gfeat)[hit].any())
    assert torch.equal(_bits(bfeat)[~hit], _bits(gfeat)[~hit])


# ---- 3. ops.lift_gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [64, 6])
def test_lift_gather_is_bit_equal_to_the_float32_gather_on_the_widened_copy(C, dtype):
    """C = 64: four channels per lane; C = 6: the generic kernel, one element per lane.  Indices -1 and P give zero rows."""
    import mvpnet_amd.ops as ops
    B, P, N, k = 3, 1111, 257, 3
    g = torch.Generator().manual_seed(C)
    feat = _half_feature((B, P, C), dtype, seed=C)
    xyz = torch.randn(B, P, 3, generator=g).to(DEV)
    index = torch.randint(0, P, (B, N, k), generator=g)
    index[0, 0, 0], index[1, 5, 2], index[2, N - 1, k - 1], index[2, 7, 1] = -1, P, -1, P
    index[0, 1] = torch.arange(k)          # (pixels 0, 1, 2: patterns at both ends of a row of eight are surely gathered)
    index = index.to(DEV)
    for image_xyz in (xyz, None):
        got = ops.lift_gather(feat, image_xyz, index)
        want = ops.lift_gather(_widened(feat), image_xyz, index)
        assert torch.equal(_bits(got[0]), _bits(want[0])) and got[0].dtype == torch.float32 and tuple(got[0].shape) == (B, N, k, C)
        assert (got[1] is None and want[1] is None) if image_xyz is None else torch.equal(got[1], want[1])
    missing = (index < 0) | (index >= P)
    assert int(missing.sum()) == 4 and not _bits(got[0])[missing].any()
    _assert_every_pattern_gathered(got[0], ~missing, dtype)


# ---- 4. no widened copy ---------------------------------------------------------------------------------------------------------------
def test_one_call_allocates_no_widened_copy_of_the_feature_maps():
    import mvpnet_amd.ops as ops
    B, nv, h, w, C, N, k = 8, 3, 120, 160, 64, 512, 3
    replaced = B * nv * h * w * C * 4
    assert replaced == 117964800
    inp = _inputs(B, nv, N, 4, 2, 'int16', seed=3, h=h, w=w, n_frames=5)
    args = (inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'])
    feat = torch.randn((B, nv, h, w, C), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(torch.bfloat16)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = ops.lift(feat, *args, k=k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print('peak allocation of one lift call on a bfloat16 map: %d bytes (the float32 copy it replaces: %d)' % (peak, replaced))
    assert peak < replaced // 2 == 58982400  # (what it must allocate is ~12 MB: search records, depth plane, outputs)
    assert bool((out[2] >= 0).any()) and out[0].dtype == torch.float32


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import mvpnet_amd.ops as ops
    B, nv, N, C, k, U = 2, 3, 300, 64, 3, 4
    inp = _inputs(B, nv, N, C, U, 'int16', seed=1)
    args = (inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'])
    feat = torch.randn(B, nv, H, W, C, generator=torch.Generator().manual_seed(2)).to(DEV)
    store = inp['store']
    for dtype in DTYPES:
        ops.lift(feat.to(dtype), *args, k=k)
        ops.lift_store(store.to(dtype), inp['view_slot'], *args, k=k)
        with pytest.raises(RuntimeError, match=r'forward only.*feature\.float\(\)'):   # a half feature that needs a gradient
            ops.lift(feat.to(dtype).requires_grad_(True), *args, k=k)
        with pytest.raises(RuntimeError, match=r'forward only.*feature\.float\(\)'):
            ops.lift_gather(feat.to(dtype).requires_grad_(True), None, torch.zeros(B, N, k, dtype=torch.int64, device=DEV))
        with torch.no_grad():                                                        # ... which nobody asks for under no_grad
            ops.lift(feat.to(dtype).requires_grad_(True), *args, k=k)
        with pytest.raises(RuntimeError):                                            # a CPU tensor
            ops.lift(feat.to(dtype).cpu(), *args, k=k)
        with pytest.raises(RuntimeError):
            ops.lift_store(store.to(dtype).cpu(), inp['view_slot'], *args, k=k)
        with pytest.raises(RuntimeError):                                            # (U,h,w,C) shape, channel-major memory
            ops.lift_store(store.to(dtype).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), inp['view_slot'], *args, k=k)
        with pytest.raises(RuntimeError):                                            # a half store of another map size
            ops.lift_store(store.to(dtype)[:, :, :W - 1], inp['view_slot'], *args, k=k)
    for op in (lambda f: ops.lift(f, *args, k=k), lambda f: ops.lift_store(f[0, :U // 2 + 1], inp['view_slot'], *args, k=k),
               lambda f: ops.lift_gather(f, None, torch.zeros(B, N, k, dtype=torch.int64, device=DEV))):
        with pytest.raises(RuntimeError):                                            # float64, as before
            op(feat.double())


# ---- 6. guard bands (bfloat16: the arena has its poison pattern) -------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['mvp_lift_h16', 'mvp_lift_store_h16'])
def test_the_entries_write_only_their_outputs_and_read_only_their_inputs(entry):
    import mvpnet_amd.ops as ops
    from mvpnet_amd import _lib as L
    B, nv, N, C, k, U = 2, 3, 300, 64, 3, 4
    inp = _inputs(B, nv, N, C, U, 'int16', seed=21)
    store_entry = entry == 'mvp_lift_store_h16'
    g = torch.Generator().manual_seed(6)
    feat = torch.randn((U, H, W, C) if store_entry else (B, nv, H, W, C), generator=g).to(torch.bfloat16).to(DEV)
    a = Arena(DEV)
    a.inp('depth', inp['depth'], fill=1500).inp('kinv', inp['kinv']).inp('cam', inp['cam']).inp('pose', inp['pose']).inp('points', inp['points'])
    a.inp('feature', feat)
    if store_entry:
        a.inp('view_slot', inp['view_slot'], fill=0)
    a.scratch('ws', L.lib().mvp_lift_workspace_bytes(B, nv, H, W, N), dtype=torch.uint8)
    a.out('knn', (B, N, k), dtype=torch.int64).out('gfeat', (B, N, k, C)).out('gxyz', (B, N, k, 3))
    a.build()
    p = lambda name: L.ptr(a[name])
    head = (p('depth'), 1, p('kinv'), p('cam'), p('pose'), None, p('points'), p('feature'), L.LIMITS['MVP_FEATURE_BF16'])
    tail = (B, nv, H, W, N, C, k, p('ws'), p('knn'), p('gfeat'), p('gxyz'))
    if store_entry:
        L.call(entry, feat, *head, p('view_slot'), U, *tail)
        want = ops.lift_store(feat, inp['view_slot'], inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'], k=k)
    else:
        L.call(entry, feat, *head, *tail, None, None)
        want = ops.lift(feat, inp['depth'], inp['kinv'], inp['cam'], inp['pose'], inp['points'], k=k)
    torch.cuda.synchronize()
    assert a.check() == []
    knn = a.result('knn')
    assert int(knn.min()) >= -1 and int(knn.max()) < nv * H * W, 'every index written'
    _assert_bit_equal((a.result('gfeat'), a.result('gxyz'), knn), want)


# ---- 7. the model ---------------------------------------------------------------------------------------------------------------------
class _Typed2D(_Feature2D):
    """The stand-in 2D network returning its map in `dtype` (widen = False) or that map widened again (widen = True); counts its images."""

    def __init__(self, dtype, widen):
        super().__init__()
        self.dtype, self.widen, self.seen = dtype, widen, 0

    def forward(self, data):
        self.seen += data['image'].size(0)
        feat = super().forward(data)['feature'].to(self.dtype)
        return {'feature': feat.float() if self.widen else feat}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def scene():
    """The ragged end-to-end scene of tests/test_scene_shared_gpu.py."""
    from mvpnet_amd.synthetic import make_rgbd_scene
    sc = make_rgbd_scene(3, E2E['n_frames'], n_pts=E2E['n_pts'], h=E2E['h'], w=E2E['w'])
    F, h, w = sc['depth_mm'].shape
    images = np.random.RandomState(8).standard_normal((F, 3, h, w)).astype(np.float32)
    return dict(sc=sc, images=_t(images), pts=_t(sc['points']), depth=_t(sc['depth_mm'].astype(np.int16)), pose=_t(sc['pose']))


def _kw(**extra):
    kw = dict(num_rgbd_frames=3, k=3, min_nb_pts=E2E['min_nb_pts'], num_base_pts=E2E['num_base_pts'], batch_size=8, pad_seed=11,
              generator=torch.Generator(device=DEV).manual_seed(7), **E2E['chunk'])
    kw.update(extra)
    return kw


@pytest.fixture(scope='module')
def batch(scene):
    from mvpnet_amd.scene import prepare_scene_bucketed
    batches = prepare_scene_bucketed(scene['pts'], scene['depth'], scene['sc']['cam_matrix'], scene['pose'], scene['images'], **_kw())[0]
    return next(b for b in batches if b['points'].size(0) > 1)


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_model_lifts_a_half_feature_map_as_it_is(batch, dtype):
    model = _prep_model()
    B, nv = batch['depth'].shape[:2]
    with torch.no_grad():
        model.net_2d = _Typed2D(dtype, widen=True)
        want = model(dict(batch))['seg_logit']
        model.net_2d = _Typed2D(dtype, widen=False)
        got = model(dict(batch))['seg_logit']
        assert torch.equal(got, want) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        # the same batch through a half store: no net_2d call
        feat = model.net_2d({'image': batch['images'].reshape(B * nv, *batch['images'].shape[2:])})['feature']
        assert feat.dtype == dtype
        perm = torch.randperm(B * nv, generator=torch.Generator().manual_seed(2)).to(DEV)
        store = feat.permute(0, 2, 3, 1).contiguous()[perm]
        view_slot = torch.argsort(perm).to(torch.int32).view(B, nv)
        seen = model.net_2d.seen
        shared = {key: v for key, v in batch.items() if key != 'images'}
        got = model(dict(shared, feature_store=store, view_slot=view_slot))['seg_logit']
    assert model.net_2d.seen == seen, 'a store batch does not run the 2D network'
    assert torch.equal(got, want)


def test_the_model_widens_a_half_feature_map_that_needs_a_gradient(batch):
    """The scatter-add backward is float32 only: under grad, a half map that requires grad is widened first (it raised before)."""
    class Trainable(_Feature2D):
        def __init__(self):
            super().__init__()
            self.gain = torch.nn.Parameter(torch.ones(()))

        def forward(self, data):
            return {'feature': (super().forward(data)['feature'] * self.gain).to(torch.bfloat16)}

    model = _prep_model()
    model.net_2d = Trainable().to(DEV)
    model._after_lift = lambda data_batch, points, plan, gfeat, gxyz: gfeat   # the lift alone: what is behind it is not the subject
    gfeat = model(dict(batch))
    assert gfeat.dtype == torch.float32 and gfeat.requires_grad
    with torch.no_grad():
        assert torch.equal(_bits(model(dict(batch))), _bits(gfeat.detach())), 'the half map as it is gives the same rows'
    gfeat.sum().backward()
    assert model.net_2d.gain.grad is not None and bool(torch.isfinite(model.net_2d.gain.grad)) and float(model.net_2d.gain.grad) != 0.0


# ---- 8. the whole scene ---------------------------------------------------------------------------------------------------------------
def _shared(scene, net_2d, **extra):
    from mvpnet_amd.scene import infer_scene_shared
    model = _prep_model()
    model.net_2d = net_2d
    return infer_scene_shared(model, scene['pts'], scene['depth'], scene['sc']['cam_matrix'], scene['pose'], scene['images'], **_kw(**extra))


def _assert_same_scene(got, want):
    for name, a, b in zip(('mean logits', 'labels', 'counts'), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name


def test_a_bfloat16_store_of_bfloat16_values_changes_nothing_and_holds_twice_the_frames(scene, monkeypatch):
    from mvpnet_amd import scene as S
    want = _shared(scene, _Typed2D(torch.bfloat16, widen=True))          # float32 output already rounded to bfloat16 values
    assert int((want[2] > 0).sum()) > scene['pts'].size(0) // 2
    caps, stores = [], []
    plan, make = S.plan_store_groups, S._frame_store
    monkeypatch.setattr(S, 'plan_store_groups', lambda frames, cap: caps.append(cap) or plan(frames, cap))
    monkeypatch.setattr(S, '_frame_store', lambda *a, **kw: stores.append(make(*a, **kw)) or stores[-1])
    h, w, C = E2E['h'], E2E['w'], 16
    budget = 5 * h * w * C * 4 + 100
    assert budget // (h * w * C * 2) == 10 and budget // (h * w * C * 4) == 5
    got = _shared(scene, _Typed2D(torch.bfloat16, widen=True), store_dtype=torch.bfloat16, max_store_bytes=budget)
    _assert_same_scene(got, want)
    # (a single batch that needs more than the cap is a run of its own: the stores' sizes are plan_store_groups' business)
    assert caps == [10] and len(stores) > 1 and all(s[0].dtype == torch.bfloat16 for s in stores)
    del stores[:]
    _assert_same_scene(_shared(scene, _Typed2D(torch.bfloat16, widen=True), max_store_bytes=budget), want)
    assert caps == [10, 5] and all(s[0].dtype == torch.float32 for s in stores)


def test_a_network_that_returns_float16_is_taken_with_a_float16_store_only(scene):
    want = _shared(scene, _Typed2D(torch.float16, widen=True))
    net_2d = _Typed2D(torch.float16, widen=False)
    _assert_same_scene(_shared(scene, net_2d, store_dtype=torch.float16), want)
    assert net_2d.seen > 0
    with pytest.raises(RuntimeError, match='net_2d must return a float32'):
        _shared(scene, _Typed2D(torch.float16, widen=False))
    with pytest.raises(RuntimeError, match='net_2d must return a float32'):
        _shared(scene, _Typed2D(torch.float16, widen=False), store_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        _shared(scene, _Typed2D(torch.float16, widen=True), store_dtype=torch.float64)

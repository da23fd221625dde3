"""Scene preparation on the MI355X: mvp_frame_overlap_* and mvp_select_frames_u32 against the NumPy oracle / the committed fixture
(bit-identical), batched selection against a per-chunk loop of chunks.select_frames, prepare_scene -> infer_scene against the same
batches assembled by hand, and both kernels inside a captured graph."""
import numpy as np
import pytest
import torch

from tests import scene_prep_oracle as SO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def scene():
    return SO.fixture_scene()


@pytest.fixture(scope='module')
def fixture(golden):
    return golden('scene_prep')


def _kinv(scene, F):
    return t(np.repeat(scene['kinv'][None], F, 0))


@pytest.mark.parametrize('kind', ['u16', 'f32'])
@pytest.mark.parametrize('packed', [True, False])
def test_overlap_matches_the_fixture(scene, fixture, kind, packed):
    import mvpnet_amd.ops as ops
    P = SO.FIXTURE
    F, nb = P['n_frames'], P['num_base_pts']
    depth = t(scene['depth_mm'].astype(np.int16)) if kind == 'u16' else t(scene['depth_mm'].astype(np.float32) / np.float32(1000.))
    base = t(scene['points'][fixture['base_point_ind']])
    out = ops.rgbd_overlap(depth, _kinv(scene, F), t(scene['pose']), base, radius=P['radius'], packed=packed)
    if packed:
        assert out.dtype == torch.int32 and tuple(out.shape) == (F, (nb + 31) // 32)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), fixture['overlap_bits'])
        assert not out[F // 2].any()  # the frame with the inf pose
    else:
        expect = SO.unpack_bits(fixture['overlap_bits'], nb).T
        assert out.dtype == torch.bool and tuple(out.shape) == (nb, F)
        assert np.array_equal(out.cpu().numpy(), expect)
        assert not out[:, F // 2].any() and out.any()


@pytest.mark.parametrize('nb,F,radius', [(1999, 7, 0.1), (37, 5, 0.1), (1, 3, 0.5), (2000, 1, 0.1), (500, 6, 0.0), (333, 6, 100.0), (4096, 2, 0.1)])
def test_overlap_shapes_and_radii(scene, fixture, nb, F, radius):
    """nb not a multiple of 32, a single frame (the 64-pixel workgroups), a radius that admits nothing (d2 < 0 never holds) and one
    that admits every valid pixel's nearest point, the largest nb the kernel takes; float32 NaN poses are skipped like inf ones."""
    import mvpnet_amd.ops as ops
    rs = np.random.RandomState(nb)
    frames = np.sort(rs.choice(SO.FIXTURE['n_frames'], F, replace=False))
    depth, pose = scene['depth_mm'][frames], scene['pose'][frames].copy()
    if F >= 5:
        pose[1, 2, 3] = np.nan
    base = scene['points'][rs.choice(len(scene['points']), nb, replace=False)]
    expect = SO.rgbd_overlap(depth, scene['kinv'], pose, base, radius)
    out = ops.rgbd_overlap(t(depth.astype(np.int16)), _kinv(scene, F), t(pose), t(base), radius=radius)
    assert np.array_equal(out.cpu().numpy(), expect)
    bits = ops.rgbd_overlap(t(depth.astype(np.int16)), _kinv(scene, F), t(pose), t(base), radius=radius, packed=True)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), SO.pack_bits(expect.T))  # the padding bits of the last word stay zero
    if radius == 0.0:
        assert not expect.any()
    if radius == 100.0:
        finite = np.isfinite(pose).all((1, 2))
        assert expect[:, finite].any(0).all() and not expect[:, ~finite].any()
    with pytest.raises(RuntimeError):
        ops.rgbd_overlap(t(depth.astype(np.int16)), _kinv(scene, F), t(pose), t(np.zeros((4097, 3), np.float32)))


def _loop_select(overlaps, masks, n):
    """the parent commit's way: one chunks.select_frames call per chunk (a host synchronisation per pick)"""
    from mvpnet_amd.chunks import select_frames
    return np.array([select_frames(overlaps[m], n) for m in masks], np.int64).reshape(len(masks), n)


def test_selection_matches_the_fixture(scene, fixture):
    import mvpnet_amd.ops as ops
    P = SO.FIXTURE
    nb, n = P['num_base_pts'], P['num_rgbd_frames']
    ov_bits = t(fixture['overlap_bits'].view(np.int32))
    ch_bits = t(fixture['chunk_bits'].view(np.int32))
    picked, gain = ops.select_frames_batched(ov_bits, ch_bits, n, return_gain=True)
    assert picked.dtype == torch.int64 and gain.dtype == torch.int32
    assert np.array_equal(picked.cpu().numpy(), fixture['picked']) and np.array_equal(gain.cpu().numpy(), fixture['gain'])
    overlaps = ops.unpack_bits(ov_bits, nb).t().contiguous()  # (nb,F) bool
    masks = ops.unpack_bits(ch_bits, nb)
    assert np.array_equal(ops.select_frames_batched(overlaps, masks, n).cpu().numpy(), fixture['picked'])  # bool input
    assert np.array_equal(_loop_select(overlaps, masks, n), fixture['picked'])
    # gain sums to the number of the chunk's base points that the picked frames cover
    covered = torch.stack([overlaps[m][:, p].any(1).sum() for m, p in zip(masks, picked)])
    assert torch.equal(gain.sum(1).long(), covered)


@pytest.mark.parametrize('F,nb,C,n', [(1, 50, 4, 3), (5, 64, 6, 6), (257, 777, 9, 4), (300, 2000, 16, 3), (700, 33, 5, 8)])
def test_selection_on_random_bits(F, nb, C, n):
    """Random overlap matrices: empty chunks, more picks than useful frames (frame 0 again and again once nothing is left), F not a
    multiple of the workgroup size, and forced ties (duplicated frames, the lowest index must win)."""
    import mvpnet_amd.ops as ops
    rs = np.random.RandomState(F * 1000 + nb)
    ov = rs.rand(nb, F) < 0.08
    if F >= 5:
        ov[:, F - 1] = ov[:, 2]      # exact ties between frames
        ov[:, 3] = ov[:, 2]
        ov[:, 0] = False             # frame 0 sees nothing and is still the answer when every score is zero
    masks = rs.rand(C, nb) < 0.3
    masks[0] = False                 # an empty chunk
    if C > 2:
        masks[2] = True              # every base point
    ov_t, mk_t = t(ov), t(masks)
    picked, gain = ops.select_frames_batched(ov_t, mk_t, n, return_gain=True)
    epicked, egain = SO.select_frames_batched(ov, masks, n)
    assert np.array_equal(picked.cpu().numpy(), epicked) and np.array_equal(gain.cpu().numpy(), egain)
    assert np.array_equal(_loop_select(ov_t, mk_t, n), epicked)
    assert (picked[0] == 0).all() and (gain[0] == 0).all()
    packed = ops.select_frames_batched(ops.pack_bits(ov_t.t()), ops.pack_bits(mk_t), n)
    assert torch.equal(packed, picked)
    assert np.array_equal(gain.sum(1).cpu().numpy(), np.array([ov[m][:, list(p)].any(1).sum() for m, p in zip(masks, epicked)]))


def test_kernels_run_inside_a_captured_graph(scene, fixture):
    """Both entry points only enqueue work on the given stream (a memset and a launch; a launch): captured once, replayed on fresh
    input they give the eager result."""
    from mvpnet_amd import _lib as L
    P = SO.FIXTURE
    F, nb, n = P['n_frames'], P['num_base_pts'], P['num_rgbd_frames']
    W = (nb + 31) // 32
    depth = t(scene['depth_mm'].astype(np.int16))
    kinv, pose = _kinv(scene, F), t(scene['pose'])
    base = t(scene['points'][fixture['base_point_ind']])
    ch_bits = t(fixture['chunk_bits'].view(np.int32))
    C = ch_bits.size(0)
    bits = torch.full((F, W), -1, dtype=torch.int32, device=DEV)
    picked = torch.full((C, n), -1, dtype=torch.int64, device=DEV)
    gain = torch.full((C, n), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.call('mvp_frame_overlap_u16', depth, L.ptr(depth), L.ptr(kinv), L.ptr(pose), L.ptr(base), F, P['h'], P['w'], nb, P['radius'], L.ptr(bits))
        L.call('mvp_select_frames_u32', bits, L.ptr(bits), L.ptr(ch_bits), F, C, W, n, L.ptr(picked), L.ptr(gain))
    for rep in range(2):
        bits.fill_(-1)
        picked.fill_(-1)
        gain.fill_(-1)
        if rep == 1:  # other input through the same static buffers: the first two frames swapped
            depth[:2] = depth[:2].flip(0)
            pose[:2] = pose[:2].flip(0)
        g.replay()
        torch.cuda.synchronize()
        expect = fixture['overlap_bits'].copy()
        if rep == 1:
            expect[:2] = expect[:2][::-1]
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), expect)
        eov = SO.unpack_bits(expect, nb).T
        epicked, egain = SO.select_frames_batched(eov, SO.unpack_bits(fixture['chunk_bits'], nb), n)
        assert np.array_equal(picked.cpu().numpy(), epicked) and np.array_equal(gain.cpu().numpy(), egain)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
CFG = dict(num_centroids=(256, 64, 16, 4), radius=(0.1, 0.2, 0.4, 0.8), max_neighbors=(32, 32, 32, 32))
E2E = dict(n_frames=24, n_pts=24000, h=30, w=40, num_base_pts=700, min_nb_pts=1024, batch_size=3,
           chunk=dict(chunk_size=(1.5, 1.5), chunk_stride=1.0, chunk_thresh=300, chunk_margin=(0.2, 0.2)))


class _Feature2D(torch.nn.Module):
    """Stands in for the frozen 2D network: 16 feature channels that are fixed multiples of the image's three."""

    def forward(self, data):
        x = data['image']
        return {'feature': torch.cat([x * (0.25 * (i + 1)) for i in range(6)], 1)[:, :16].contiguous()}


def _model():
    from mvpnet_amd.pn2 import PN2SSG
    from mvpnet_amd.mvpnet3d import MVPNet3D
    torch.manual_seed(3)
    return MVPNet3D(_Feature2D(), '', PN2SSG(16, 20, dropout_prob=0.0, **CFG), in_channels=16, mlp_channels=(16, 16, 16)).to(DEV).eval()


def _by_hand(sc, images, base_point_ind, overlaps=None):
    """The batches prepare_scene must produce, from the NumPy oracle's overlap (or `overlaps` (nb,F) bool, for base_point_ind) and one
    chunks.select_frames call per chunk."""
    from mvpnet_amd.chunks import scene2chunks_legacy, select_frames
    from mvpnet_amd.scene import pad_sparse_chunk
    pts = t(sc['points'])
    chunk_inds, boxes = scene2chunks_legacy(pts, return_bbox=True, stride=E2E['chunk']['chunk_stride'], chunk_size=E2E['chunk']['chunk_size'],
                                            thresh=E2E['chunk']['chunk_thresh'], margin=E2E['chunk']['chunk_margin'])
    if overlaps is None:
        overlaps = SO.rgbd_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], sc['points'][base_point_ind], 0.1)
    masks = SO.chunk_masks_of([c.cpu().numpy() for c in chunk_inds], base_point_ind, len(sc['points']))
    ov_t = t(overlaps)
    picks = [select_frames(ov_t[t(m)], 3) for m in masks]
    gen = torch.Generator().manual_seed(11)
    singles = [pad_sparse_chunk({'points': pts[ind].t().contiguous()}, min_nb_pts=E2E['min_nb_pts'], generator=gen)['points'] for ind in chunk_inds]
    depth, pose = t(sc['depth_mm'].astype(np.int16)), t(sc['pose'])
    cam = t(sc['cam_matrix'][:3, :3])
    kinv = t(np.linalg.inv(sc['cam_matrix'][:3, :3]))
    batches, lo = [], 0
    while lo < len(singles):
        hi = lo + 1
        while hi < len(singles) and hi - lo < E2E['batch_size'] and singles[hi].size(1) == singles[lo].size(1):
            hi += 1
        sel = torch.tensor(picks[lo:hi], device=DEV)
        box = torch.stack(boxes[lo:hi]).cpu().numpy()[:, [0, 1, 3, 4]] + np.array([-0.1, -0.1, 0.1, 0.1])
        batches.append({'images': images[sel].contiguous(), 'points': torch.stack(singles[lo:hi]).contiguous(), 'depth': depth[sel].contiguous(),
                        'cam_matrix': cam.expand(hi - lo, 3, 3, 3).contiguous(), 'kinv': kinv.expand(hi - lo, 3, 3, 3).contiguous(),
                        'pose': pose[sel].contiguous(), 'pixel_box': t(box.astype(np.float32)), 'k': 3})
        lo = hi
    return batches, chunk_inds, picks


def test_prepare_scene_then_infer_scene_equals_the_hand_assembled_batches():
    from mvpnet_amd.synthetic import make_rgbd_scene
    from mvpnet_amd.scene import prepare_scene, infer_scene
    sc = make_rgbd_scene(3, E2E['n_frames'], n_pts=E2E['n_pts'], h=E2E['h'], w=E2E['w'])
    F, h, w = sc['depth_mm'].shape
    images = torch.from_numpy(np.random.RandomState(8).standard_normal((F, 3, h, w)).astype(np.float32)).to(DEV)
    pts, depth, pose = t(sc['points']), t(sc['depth_mm'].astype(np.int16)), t(sc['pose'])
    kw = dict(num_rgbd_frames=3, k=3, min_nb_pts=E2E['min_nb_pts'], batch_size=E2E['batch_size'], num_base_pts=E2E['num_base_pts'], **E2E['chunk'])
    batches, chunk_inds, n_pts = prepare_scene(pts, depth, sc['cam_matrix'], pose, images, generator=torch.Generator(device=DEV).manual_seed(7),
                                               pad_generator=torch.Generator().manual_seed(11), **kw)
    base_point_ind = torch.randperm(len(sc['points']), generator=torch.Generator(device=DEV).manual_seed(7), device=DEV)[:E2E['num_base_pts']].cpu().numpy()
    ebatches, einds, picks = _by_hand(sc, images, base_point_ind)
    assert n_pts == len(sc['points']) and len(chunk_inds) == len(einds) >= 6
    assert any((np.array(p) == 0).all() for p in picks), 'a chunk no frame sees'
    assert any(b['points'].size(0) > 1 for b in batches), 'consecutive chunks of equal size share a batch'
    _assert_same_batches(batches, ebatches)
    for a, b in zip(chunk_inds, einds):
        assert torch.equal(a, b)
    model = _model()
    mean, label, cnt = infer_scene(model, batches, chunk_inds, n_pts)
    emean, elabel, ecnt = infer_scene(model, ebatches, einds, n_pts)
    assert torch.equal(mean, emean) and torch.equal(label, elabel) and torch.equal(cnt, ecnt)  # same kernels, same inputs
    assert int((cnt > 0).sum()) > n_pts // 2 and torch.isfinite(mean).all()
    # the reference's per-scene arrays instead of the computation; lifting maps at another resolution than the overlap's
    base_t, ov = torch.from_numpy(base_point_ind).to(DEV), t(SO.rgbd_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], sc['points'][base_point_ind], 0.1))
    cam_small = sc['cam_matrix'].copy()
    cam_small[0] /= 2
    cam_small[1] /= 2
    b2, inds2, _ = prepare_scene(pts, depth[:, ::2, ::2].contiguous(), cam_small, pose, images, overlap=(base_t, ov), lift_depth=depth,
                                 pad_generator=torch.Generator().manual_seed(11), **kw)
    assert len(b2) == len(ebatches)
    for a, b in zip(b2, ebatches):
        for key in ('images', 'points', 'depth', 'pose', 'pixel_box'):
            assert torch.equal(a[key], b[key]), key
        assert torch.equal(a['cam_matrix'], t((cam_small[:3, :3] / np.array([[0.5], [0.5], [1.0]], np.float32)).astype(np.float32)).expand_as(a['cam_matrix']))


def _e2e_inputs():
    from mvpnet_amd.synthetic import make_rgbd_scene
    sc = make_rgbd_scene(3, E2E['n_frames'], n_pts=E2E['n_pts'], h=E2E['h'], w=E2E['w'])
    F, h, w = sc['depth_mm'].shape
    images = torch.from_numpy(np.random.RandomState(8).standard_normal((F, 3, h, w)).astype(np.float32)).to(DEV)
    kw = dict(num_rgbd_frames=3, k=3, min_nb_pts=E2E['min_nb_pts'], **E2E['chunk'])
    return sc, images, t(sc['points']), t(sc['depth_mm'].astype(np.int16)), t(sc['pose']), kw


def _assert_same_batches(batches, ebatches):
    assert len(batches) == len(ebatches)
    for a, b in zip(batches, ebatches):
        assert set(a) == set(b)
        for key in b:
            if key == 'k':
                assert a[key] == b[key]
            else:
                assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key


def test_a_given_overlap_with_more_base_points_than_the_chunker_kernel_takes():
    """overlap=(base_point_ind, bool overlaps) with 4100 base points: beyond MVP_OVERLAP_MAX_BASE, so the chunks and their base bits come
    from scene2chunks_csr's fallback; within select_frames' 1024 words.  prepare_scene against the hand-assembled batches, key by key;
    prepare_scene_bucketed against those, per chunk."""
    import mvpnet_amd.ops as ops
    from mvpnet_amd.scene import prepare_scene, prepare_scene_bucketed
    sc, images, pts, depth, pose, kw = _e2e_inputs()
    nb, n_pts, floor = 4100, E2E['n_pts'], E2E['min_nb_pts']
    assert ops.overlap.MAX_BASE_POINTS < nb <= 32 * ops.overlap.MAX_SELECT_WORDS
    base = np.random.RandomState(21).choice(n_pts, nb, replace=False)
    ov = SO.rgbd_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], sc['points'][base], 0.1)
    assert ov.dtype == bool and ov.shape == (nb, E2E['n_frames'])
    ebatches, einds, picks = _by_hand(sc, images, base, ov)
    lengths = [int(i.numel()) for i in einds]
    assert len(lengths) == 42 and min(lengths) == 793 and max(lengths) == 3351
    assert sum(n < floor for n in lengths) == 12, 'chunks that are padded'
    assert any(b['points'].size(0) > 1 for b in ebatches), 'consecutive chunks of equal size share a batch'
    assert [0, 0, 0] in picks and len({tuple(p) for p in picks}) >= 16, 'a chunk no frame sees, and many distinct picks'
    given = (t(base), t(ov))
    batches, chunk_inds, got_n = prepare_scene(pts, depth, sc['cam_matrix'], pose, images, overlap=given, batch_size=E2E['batch_size'],
                                               pad_generator=torch.Generator().manual_seed(11), **kw)
    assert got_n == n_pts and len(chunk_inds) == len(einds)
    _assert_same_batches(batches, ebatches)
    for a, b in zip(chunk_inds, einds):
        assert a.dtype == b.dtype and torch.equal(a, b)

    bbatches, inds, n_pts_b, order = prepare_scene_bucketed(pts, depth, sc['cam_matrix'], pose, images, overlap=given, batch_size=8, pad_seed=11, **kw)
    C = len(einds)
    assert n_pts_b == n_pts and sorted(order) == list(range(C)) and len(inds) == C and len(bbatches) < C
    sizes = [b['points'].size(2) for b in bbatches]
    assert sizes == sorted(sizes) and len(set(sizes)) > 1 and all(b['points'].size(0) <= 8 for b in bbatches)
    ref_rows = [{key: b[key][r] for key in b if key != 'k'} for b in ebatches for r in range(b['points'].size(0))]
    i = 0
    for b in bbatches:
        B, N = b['points'].size(0), b['points'].size(2)
        for r in range(B):
            ref, n = ref_rows[order[i + r]], lengths[order[i + r]]
            assert torch.equal(inds[i + r], einds[order[i + r]]) and max(n, floor) <= N < 1.5 * max(n, floor)
            assert torch.equal(b['points'][r, :, :n], pts[inds[i + r]].t()) and torch.equal(b['points'][r, :, :n], ref['points'][:, :n])
            for key in ('images', 'depth', 'cam_matrix', 'kinv', 'pose', 'pixel_box'):
                assert b[key].dtype == ref[key].dtype and torch.equal(b[key][r], ref[key]), key
        i += B
    assert i == C


def test_an_overlap_given_as_bit_rows_equals_the_same_overlap_given_as_bool():
    """700 base points, inside the chunker kernel's limits: int32 (F,W) bit rows against bool (nb,F)."""
    import mvpnet_amd.ops as ops
    from mvpnet_amd.scene import prepare_scene
    sc, images, pts, depth, pose, kw = _e2e_inputs()
    base = np.random.RandomState(21).choice(E2E['n_pts'], 700, replace=False)
    ov = t(SO.rgbd_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], sc['points'][base], 0.1))
    bits = ops.pack_bits(ov.t())
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (E2E['n_frames'], 22) and bool(ov.any())
    run = lambda o: prepare_scene(pts, depth, sc['cam_matrix'], pose, images, overlap=(t(base), o), batch_size=E2E['batch_size'],
                                  pad_generator=torch.Generator().manual_seed(11), **kw)
    (got, got_inds, _), (want, want_inds, _) = run(bits), run(ov)
    assert len(want_inds) >= 6 and any(b['points'].size(0) > 1 for b in want)
    _assert_same_batches(got, want)
    assert len(got_inds) == len(want_inds) and all(torch.equal(a, b) for a, b in zip(got_inds, want_inds))

"""Ragged scenes on the MI355X: the chunker kernels against the reference's golden lists and against scene2chunks_legacy on adversarial
scenes, the pack kernel against its NumPy oracle, the premise the bucketed path rests on (duplicates behind a cloud's own points change
neither the sampled indices nor any ball's distinct points), and prepare_scene_bucketed -> infer_scene against prepare_scene -> infer_scene."""
import numpy as np
import pytest
import torch

from tests import scene_prep_oracle as SO
from tests import scene_ragged_oracle as RO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SIZE, MARGIN = (1.5, 1.5), (0.2, 0.2)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _membership_bits(index, offsets, base_point_ind, n):
    lists = [index[offsets[c]:offsets[c + 1]] for c in range(len(offsets) - 1)]
    return SO.pack_bits(SO.chunk_masks_of(lists, base_point_ind, n)) if lists else np.zeros((0, (len(base_point_ind) + 31) // 32), np.uint32)


def test_csr_equals_the_reference(golden):
    """Lengths, flat indices and boxes of the three golden scenes bit for bit; base-point bits for nb = 333 (no multiple of 32)."""
    from mvpnet_amd.chunks import scene2chunks_csr
    g = golden('chunker')
    for ci in range(3):
        stride, thresh = g['c%d_args' % ci]
        pts = g['c%d_points' % ci]
        base = np.random.RandomState(ci).choice(len(pts), 333, replace=False).astype(np.int64)
        csr = scene2chunks_csr(t(pts), SIZE, float(stride), thresh=int(thresh), margin=MARGIN, base_point_ind=t(base))
        assert csr['lengths'] == g['c%d_lengths' % ci].tolist() and len(csr['lengths']) > 1
        offsets = csr['offsets'].cpu().numpy()
        assert csr['offsets'].dtype == torch.int64 and offsets.tolist() == np.concatenate([[0], np.cumsum(csr['lengths'])]).tolist()
        index = csr['index'].cpu().numpy()
        assert csr['index'].dtype == torch.int64 and np.array_equal(index, g['c%d_indices' % ci])
        assert csr['boxes'].dtype == torch.float64 and np.array_equal(csr['boxes'].cpu().numpy(), g['c%d_boxes' % ci])
        assert csr['base_bits'].dtype == torch.int32 and tuple(csr['base_bits'].shape) == (len(csr['lengths']), 11)
        assert np.array_equal(csr['base_bits'].cpu().numpy().view(np.uint32), _membership_bits(index, offsets, base, len(pts)))
        assert scene2chunks_csr(t(pts), SIZE, float(stride), thresh=int(thresh), margin=MARGIN)['base_bits'] is None


def _adversarial(n):
    """n points with the origin first (corners are then float32(i * stride), exactly), coordinates ON every bound of the windows at 1.0 and
    2.0 -- corner, corner + size, corner - margin, corner + size + margin, rounded to float32 -- and on both float32 neighbours of each;
    one NaN z among them."""
    rs = np.random.RandomState(1000 + n)
    pts = [(0.0, 0.0, 0.5), (4.0, 3.0, 1.0)]
    for corner in (1.0, 2.0):
        for b in (corner, corner + 1.5, corner - 0.2, corner + 1.5 + 0.2):
            b32 = np.float32(b)
            for v in (np.nextafter(b32, np.float32(-np.inf)), b32, np.nextafter(b32, np.float32(np.inf))):
                pts.append((float(v), rs.uniform(0, 3), rs.uniform(0, 2)))
                pts.append((rs.uniform(0, 4), float(v), rs.uniform(0, 2)))
    pts = np.array(pts[:n], np.float32)
    if n > len(pts):
        pts = np.concatenate([pts, (rs.rand(n - len(pts), 3) * np.array([4.0, 3.0, 2.0])).astype(np.float32)])
    if n > 7:
        pts[7, 2] = np.nan
    return pts


def _compare_with_legacy(pts, stride, thresh, base):
    from mvpnet_amd.chunks import scene2chunks_csr, scene2chunks_legacy
    csr = scene2chunks_csr(t(pts), SIZE, stride, thresh=thresh, margin=MARGIN, base_point_ind=None if base is None else t(base))
    idx, boxes = scene2chunks_legacy(torch.from_numpy(pts), SIZE, stride, thresh=thresh, margin=MARGIN, return_bbox=True)
    assert csr['lengths'] == [len(i) for i in idx]
    index, offsets = csr['index'].cpu().numpy(), csr['offsets'].cpu().numpy()
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(csr['lengths'])]).astype(np.int64).tolist()
    assert np.array_equal(index, torch.cat(idx).numpy() if idx else np.zeros(0, np.int64))
    np.testing.assert_array_equal(csr['boxes'].cpu().numpy(), torch.stack(boxes).numpy() if boxes else np.zeros((0, 6)))  # (NaN == NaN here)
    if base is not None:
        assert tuple(csr['base_bits'].shape) == (len(idx), (len(base) + 31) // 32)
        assert np.array_equal(csr['base_bits'].cpu().numpy().view(np.uint32), _membership_bits(index, offsets, base, len(pts)))
    return csr


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 5000])
def test_adversarial_scenes_equal_legacy(n):
    from mvpnet_amd.chunks import _window_corners
    pts = _adversarial(n)
    base = np.random.RandomState(n).choice(n, min(n, 37), replace=False).astype(np.int64)
    if n == 1:  # an extent smaller than a chunk in both axes: no window at all
        csr = _compare_with_legacy(pts, 1.0, 1, base)
        assert csr['lengths'] == [] and csr['index'].numel() == 0 and tuple(csr['base_bits'].shape) == (0, 1)
        return
    corners = _window_corners(torch.from_numpy(pts), np.array(SIZE), 1.0)
    assert np.array_equal(corners[:, 0], np.round(corners[:, 0])) and len(corners) >= 12
    inner, outer = RO.window_tests(pts, corners, SIZE, MARGIN)
    # the bounds are hit from both sides: some special point is inside one window's test and outside it one float32 step further
    assert 0 < inner.sum() < outer.sum() < outer.size
    counts = inner.sum(1)
    k = int(np.sort(counts[counts > 0])[(counts > 0).sum() // 2])  # an inner count that some window has
    at = _compare_with_legacy(pts, 1.0, k, base)       # a window with exactly `thresh` inner points is kept
    above = _compare_with_legacy(pts, 1.0, k + 1, base)  # ... and dropped with thresh - 1
    assert len(at['lengths']) == int((inner.sum(1) >= k).sum()) > len(above['lengths']) == int((inner.sum(1) >= k + 1).sum())
    assert bool(torch.isnan(at['boxes']).any()) == bool(outer[inner.sum(1) >= k][:, 7].any())  # the NaN z reaches its chunks' boxes
    none = _compare_with_legacy(pts, 1.0, 10 ** 6, base)  # nothing kept
    assert none['lengths'] == [] and none['offsets'].tolist() == [0] and tuple(none['boxes'].shape) == (0, 6)
    _compare_with_legacy(pts, 0.5, 1, None)  # more windows, every non-empty one kept


def test_nan_members_narrow_extents_and_clamped_base_points():
    """The op itself with given corners against the NumPy oracle: a NaN x or y is never a member (legacy cannot show that: its corners
    come from an extent that is then NaN), an extent smaller than the chunk in one axis, windows that hold nothing (thresh 0 keeps them:
    empty lists with a (+inf, -inf) z box), out-of-range base points are clamped."""
    import mvpnet_amd.ops as ops
    from mvpnet_amd.chunks import scene2chunks_csr
    pts = _adversarial(2500)
    pts[11, 0] = np.nan
    pts[12, 1] = np.nan
    corners = np.array([(i, j) for i in range(-3, 5) for j in range(3)], np.float32)
    base = np.array([0, 11, 12, 7, 2499, -5, 2500 + 10, 1000] + list(range(30, 60)), np.int64)
    for thresh in (0, 1, 40):
        got = ops.scene_chunks(t(pts), t(corners), SIZE, MARGIN, thresh, base_point_ind=t(base))
        exp = RO.scene_chunks(pts, corners, SIZE, MARGIN, thresh, base_point_ind=np.clip(base, 0, len(pts) - 1))
        assert np.array_equal(got['kept'], exp['kept']) and got['lengths'] == exp['lengths'].tolist()
        index = got['index'].cpu().numpy()
        assert np.array_equal(index, exp['index']) and 11 not in index and 12 not in index
        np.testing.assert_array_equal(got['zbox'].cpu().numpy(), exp['zbox'])
        assert np.array_equal(got['base_bits'].cpu().numpy().view(np.uint32), exp['base_bits'])
        if thresh == 0:
            assert len(got['kept']) == len(corners) and 0 in got['lengths']
            empty = got['lengths'].index(0)
            assert got['zbox'][empty].tolist() == [float('inf'), float('-inf')] and not got['base_bits'][empty].any()
    narrow = (np.random.RandomState(5).rand(3000, 3) * np.array([5.0, 1.0, 2.0])).astype(np.float32)  # y extent 1.0 < 1.5
    csr = _compare_with_legacy(narrow, 1.0, 50, None)
    assert len(csr['lengths']) >= 3
    with pytest.raises(RuntimeError):
        ops.scene_chunks(t(pts).double(), t(corners), SIZE, MARGIN, 1)
    with pytest.raises(RuntimeError):
        ops.scene_chunks(t(pts), t(corners).reshape(-1), SIZE, MARGIN, 1)
    with pytest.raises(RuntimeError):
        ops.scene_chunks(t(pts), torch.from_numpy(corners), SIZE, MARGIN, 1)
    with pytest.raises(RuntimeError):
        ops.scene_chunks(t(pts), t(corners), SIZE, MARGIN, 1, base_point_ind=t(base).int())
    with pytest.raises(RuntimeError):
        ops.scene_chunks(t(pts), t(corners), SIZE, MARGIN, 1, base_point_ind=t(np.arange(4097)))
    assert scene2chunks_csr(t(narrow), SIZE, 1.0, thresh=50, base_point_ind=t(np.arange(4097) % 3000))['base_bits'].shape == (len(csr['lengths']), 129)  # legacy's way


def test_pack_equals_the_oracle():
    """Buckets of four different sizes in one launch; n_c = 1, n_c = N_c and N_c - n_c = 1 among them."""
    import mvpnet_amd.ops as ops
    rs = np.random.RandomState(3)
    pts = rs.standard_normal((5000, 3)).astype(np.float32)
    lengths = [1, 1024, 1023, 700, 3000, 257, 64, 5000, 1]
    out_len = [64, 1024, 1024, 1024, 4096, 1536, 64, 5000, 1]
    index = np.concatenate([np.sort(rs.choice(5000, n, replace=False)) for n in lengths]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    out_base, at = [0] * len(lengths), 0
    for c in np.argsort(out_len, kind='stable'):  # sorted by size, as the bucketed batches lie in their buffer
        out_base[c], at = at, at + 3 * out_len[c]
    for seed in (0, 2 ** 40 + 12345):
        got = ops.pack_chunks(t(pts), t(index), t(offsets), lengths, out_base, out_len, seed=seed)
        exp = RO.pack_chunks(pts, index, offsets, out_base, out_len, seed=seed)
        assert got.dtype == torch.float32 and got.numel() == at == exp.size and not np.isnan(exp).any()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    two = got[out_base[1]:out_base[1] + 3 * 3 * 1024].view(3, 3, 1024)  # chunks 1, 2, 3: one (B,3,N) batch
    assert torch.equal(two[1, :, :1023], t(pts[index[offsets[2]:offsets[3]]]).t())
    with pytest.raises(RuntimeError):  # n_c >= 1
        ops.pack_chunks(t(pts), t(index), t(offsets), [0] + lengths[1:], out_base, out_len)
    with pytest.raises(RuntimeError):  # N_c >= n_c
        ops.pack_chunks(t(pts), t(index), t(offsets), lengths, out_base, [64, 1023] + out_len[2:])
    with pytest.raises(RuntimeError):
        ops.pack_chunks(t(pts), t(index).int(), t(offsets), lengths, out_base, out_len)
    with pytest.raises(RuntimeError):
        ops.pack_chunks(t(pts), t(index), t(offsets), lengths[1:], out_base[1:], out_len[1:])
    with pytest.raises(RuntimeError):
        ops.pack_chunks(t(pts), torch.from_numpy(index), t(offsets), lengths, out_base, out_len)


@pytest.mark.parametrize('n,N,M,radius', [(700, 1024, 256, 0.22), (3000, 4096, 1024, 0.15)])
def test_duplicates_behind_a_cloud_change_neither_samples_nor_balls(n, N, M, radius):
    """The premise of the bucketed path on the shipped kernels: farthest point sampling returns identical indices (lowest index on a
    tie, the originals come first), and every ball (K = 32, first hits in index order) holds the same set of distinct points."""
    import mvpnet_amd.ops as ops
    pts = np.random.RandomState(n).rand(n, 3).astype(np.float32)
    assert len(np.unique(pts, axis=0)) == n
    padded = ops.pack_chunks(t(pts), torch.arange(n, device=DEV), t(np.array([0, n], np.int64)), [n], [0], [N], seed=9).view(1, 3, N)
    source = RO.pad_slots(n, N, 9, 0)  # slot -> original point
    assert torch.equal(padded[0].t(), t(pts[source]))
    cloud, cloud_p = t(pts)[None].contiguous(), padded.transpose(1, 2).contiguous()
    idx = ops.farthest_point_sample(cloud, M, transpose=False)
    idx_p = ops.farthest_point_sample(cloud_p, M, transpose=False)
    assert torch.equal(idx, idx_p) and int(idx.max()) < n and idx.unique().numel() == M
    query = cloud[:, idx[0]].contiguous()
    ball = ops.ball_query(query, cloud, radius, 32, transpose=False)[0].cpu().numpy()
    ball_p = ops.ball_query(query, cloud_p, radius, 32, transpose=False)[0].cpu().numpy()
    assert ball.min() >= 0 and ball_p.max() >= n  # every centroid finds itself; duplicates do enter balls
    sizes = [len(set(row)) for row in ball]
    assert min(sizes) < 32 and max(sizes) == 32  # balls that are not full (duplicates fill them) and balls that are
    for row, row_p in zip(ball, ball_p):
        assert set(row.tolist()) == set(source[row_p].tolist())


def test_bucketed_scene_equals_the_per_chunk_path():
    """prepare_scene_bucketed -> infer_scene against prepare_scene -> infer_scene on the scene and model of tests/test_scene_prep_gpu.py."""
    from mvpnet_amd.synthetic import make_rgbd_scene
    from mvpnet_amd.scene import prepare_scene, prepare_scene_bucketed, infer_scene
    from tests.test_scene_prep_gpu import E2E, _model
    sc = make_rgbd_scene(3, E2E['n_frames'], n_pts=E2E['n_pts'], h=E2E['h'], w=E2E['w'])
    F, h, w = sc['depth_mm'].shape
    images = torch.from_numpy(np.random.RandomState(8).standard_normal((F, 3, h, w)).astype(np.float32)).to(DEV)
    pts, depth, pose = t(sc['points']), t(sc['depth_mm'].astype(np.int16)), t(sc['pose'])
    kw = dict(num_rgbd_frames=3, k=3, min_nb_pts=E2E['min_nb_pts'], num_base_pts=E2E['num_base_pts'], **E2E['chunk'])
    ref_batches, ref_inds, n_pts = prepare_scene(pts, depth, sc['cam_matrix'], pose, images, batch_size=E2E['batch_size'],
                                                 generator=torch.Generator(device=DEV).manual_seed(7), pad_generator=torch.Generator().manual_seed(11), **kw)
    batches, inds, n_pts_b, order = prepare_scene_bucketed(pts, depth, sc['cam_matrix'], pose, images, batch_size=8, pad_seed=11,
                                                           generator=torch.Generator(device=DEV).manual_seed(7), **kw)
    C = len(ref_inds)
    assert n_pts_b == n_pts == E2E['n_pts'] and sorted(order) == list(range(C)) and len(inds) == C >= 6
    assert len(batches) < C, 'fewer batches than chunks'
    sizes = [b['points'].size(2) for b in batches]
    assert sizes == sorted(sizes) and len(set(sizes)) > 1 and all(b['points'].size(0) <= 8 for b in batches)
    ref_rows = [{key: b[key][r] for key in b if key != 'k'} for b in ref_batches for r in range(b['points'].size(0))]
    i, mixed = 0, False
    for b in batches:
        B, N = b['points'].size(0), b['points'].size(2)
        true = [int(inds[i + r].numel()) for r in range(B)]
        mixed = mixed or len(set(true)) > 1
        for r in range(B):
            ref, n = ref_rows[order[i + r]], true[r]
            assert torch.equal(inds[i + r], ref_inds[order[i + r]]) and max(n, E2E['min_nb_pts']) <= N < 1.5 * max(n, E2E['min_nb_pts'])
            assert torch.equal(b['points'][r, :, :n], pts[inds[i + r]].t()) and torch.equal(b['points'][r, :, :n], ref['points'][:, :n])
            member = torch.zeros(n_pts, dtype=torch.bool, device=DEV)
            member[inds[i + r]] = True
            assert bool(member[_rows_of(pts, b['points'][r, :, n:].t())].all())  # the padding: points of the chunk itself
            for key in ('images', 'depth', 'cam_matrix', 'kinv', 'pose', 'pixel_box'):
                assert b[key].dtype == ref[key].dtype and torch.equal(b[key][r], ref[key]), key
        i += B
    assert mixed, 'at least one batch holds chunks of different true lengths'
    model = _model()
    emean, elabel, ecnt = infer_scene(model, ref_batches, ref_inds, n_pts)
    mean, label, cnt = infer_scene(model, batches, inds, n_pts)
    assert torch.equal(cnt, ecnt)
    voted = ecnt > 0
    gap_logit = float((mean - emean).abs().max())
    top2 = emean.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) >= 2e-4
    left_out, unvoted = int((~decided).sum()), int((~voted).sum())
    changed = int((label != elabel).sum())
    print('ragged e2e: chunks %d, batches %d (per-chunk path: %d), max |mean logit difference| %.3e, points under the 2e-4 gap %d of %d '
          '(without a vote: %d), labels changed %d' % (C, len(batches), len(ref_batches), gap_logit, left_out, n_pts, unvoted, changed))
    assert torch.isfinite(mean).all() and int(voted.sum()) > n_pts // 2
    assert gap_logit <= 1e-4
    assert torch.equal(label[decided], elabel[decided]) and torch.equal(label[~voted], elabel[~voted])
    assert left_out <= n_pts // 100


def _rows_of(pts, rows):
    """index of each of `rows` (m,3) in pts (n,3): exact matches (the synthetic scene's points are distinct)."""
    if rows.size(0) == 0:
        return torch.zeros(0, dtype=torch.int64, device=pts.device)
    key = lambda x: x.contiguous().view(torch.int32).long()
    a, b = key(pts), key(rows)
    ha, hb = (a[:, 0] * 1000003 + a[:, 1]) * 1000003 + a[:, 2], (b[:, 0] * 1000003 + b[:, 1]) * 1000003 + b[:, 2]
    sa, perm = ha.sort()
    pos = torch.searchsorted(sa, hb).clamp_(max=sa.numel() - 1)
    assert torch.equal(sa[pos], hb)
    return perm[pos]

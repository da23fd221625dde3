"""Ragged scenes without a GPU: the bucket planner's arithmetic, the NumPy oracle of the pack rule, scene2chunks_csr on a CPU tensor
(it then goes through scene2chunks_legacy) against the reference's golden lists, and the error paths that launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

from tests import scene_prep_oracle as SO
from tests import scene_ragged_oracle as RO
from tests.conftest import load_golden

MIN, MAXB = 2048, 32768
RUNGS = [2048, 3072, 4096, 6144, 8192, 12288, 16384, 24576, 32768]
# just below, on and above rungs; below min_nb_pts; on and above max_bucket (the last two twice: equal oversize chunks stay alone)
LENGTHS = [2047, 2048, 2049, 1, 700, 3071, 3072, 3073, 4096, 4097, 6143, 6145, 8192, 12289, 24577, 32768, 32769, 32769, 50000, 5, 3000, 2048] + [2500] * 70


def _check_plan(lengths, batches, order, min_nb_pts, batch_size, max_batch_points, max_bucket, rungs):
    assert sorted(order) == list(range(len(lengths)))
    assert [c for _, members in batches for c in members] == order  # every chunk in exactly one batch, order = the batches' order
    sizes = [N for N, _ in batches]
    assert sizes == sorted(sizes)
    for N, members in batches:
        assert 1 <= len(members) <= batch_size
        for c in members:
            n = lengths[c]
            if n > max_bucket:
                assert len(members) == 1 and N == n  # alone and unpadded
            else:
                assert N == min(r for r in rungs if r >= max(n, min_nb_pts))
                assert N < 1.5 * max(n, min_nb_pts) or N == min_nb_pts
                assert len(members) == 1 or len(members) * N <= max_batch_points
    for (Na, a), (Nb, b) in zip(batches, batches[1:]):  # ties keep the chunker's order; a batch is only cut when it is full
        if Na == Nb:
            assert a[-1] < b[0] or max(lengths[c] for c in a + b) > max_bucket
            if max(lengths[c] for c in a + b) <= max_bucket:
                assert len(a) == min(batch_size, max(1, max_batch_points // Na))


@pytest.mark.parametrize('batch_size,max_batch_points', [(32, 32 * 8192), (4, 32 * 8192), (32, 20000), (1, 1)])
def test_bucket_planner(batch_size, max_batch_points):
    from mvpnet_amd.scene import plan_buckets, bucket_size
    batches, order = plan_buckets(LENGTHS, min_nb_pts=MIN, batch_size=batch_size, max_batch_points=max_batch_points, max_bucket=MAXB)
    _check_plan(LENGTHS, batches, order, MIN, batch_size, max_batch_points, MAXB, RUNGS)
    assert [bucket_size(n, MIN, MAXB) for n in (1, 2048, 2049, 3072, 3073, 32768, 32769)] == [2048, 2048, 3072, 3072, 4096, 32768, 32769]
    if batch_size == 32 and max_batch_points == 32 * 8192:
        assert len(batches) < len(LENGTHS) // 3
        assert any(len({LENGTHS[c] for c in members}) > 1 for _, members in batches)  # chunks of different true lengths share a batch


def test_bucket_planner_odd_ladder_and_cap():
    """min_nb_pts = 1000 (rungs 1000, 1500, 2000, 3000, ...), a max_bucket that is no rung (chunks up to it are padded to it, not beyond),
    no chunks at all."""
    from mvpnet_amd.scene import plan_buckets, bucket_size
    rungs = [1000, 1500, 2000, 3000, 4000, 5000]  # 5000: the cap
    lengths = [999, 1000, 1001, 1500, 1501, 2999, 3001, 4001, 5000, 5001, 4000]
    batches, order = plan_buckets(lengths, min_nb_pts=1000, batch_size=2, max_batch_points=10 ** 9, max_bucket=5000)
    _check_plan(lengths, batches, order, 1000, 2, 10 ** 9, 5000, rungs)
    assert bucket_size(4001, 1000, 5000) == 5000 and bucket_size(5001, 1000, 5000) == 5001
    assert [bucket_size(n, 7, 10 ** 6) for n in (7, 8, 10, 11, 14, 15, 21, 22)] == [7, 10, 10, 14, 14, 21, 21, 28]  # 1.5 x rounded down
    assert plan_buckets([], min_nb_pts=1000) == ([], [])


@pytest.mark.parametrize('n_c,N_c', [(1, 1), (1, 64), (700, 1024), (1024, 1024), (1023, 1024), (3000, 4096)])
def test_pack_oracle(n_c, N_c):
    rs = np.random.RandomState(n_c)
    pts = rs.rand(5000, 3).astype(np.float32)
    members = np.sort(rs.choice(5000, n_c, replace=False)).astype(np.int64)
    other = np.sort(rs.choice(5000, 40, replace=False)).astype(np.int64)  # a neighbour chunk in front: chunk numbers seed the draws
    index, offsets = np.concatenate([other, members]), [0, 40, 40 + n_c]
    out = RO.pack_chunks(pts, index, offsets, [0, 3 * 64], [64, N_c], seed=77)
    got = out[3 * 64:].reshape(3, N_c).T
    assert np.array_equal(got[:n_c], pts[members])  # prefix = members, in order
    slots = RO.pad_slots(n_c, N_c, 77, 1)
    assert slots.shape == (N_c,) and np.array_equal(slots[:n_c], np.arange(n_c)) and slots.min() >= 0 and slots.max() < n_c
    assert np.array_equal(got, pts[members[slots]])  # every pad slot names a member of its own chunk
    if N_c - n_c >= 300:
        assert len(np.unique(slots[n_c:])) > (N_c - n_c) // 4  # draws, not one value
        assert not np.array_equal(slots[n_c:], RO.pad_slots(n_c, N_c, 78, 1)[n_c:]) and not np.array_equal(slots[n_c:], RO.pad_slots(n_c, N_c, 77, 2)[n_c:])


def test_csr_on_a_cpu_tensor_equals_legacy_and_the_reference():
    from mvpnet_amd.chunks import scene2chunks_csr, scene2chunks_legacy
    g = load_golden('chunker')
    for ci in range(3):
        stride, thresh = g['c%d_args' % ci]
        pts = torch.from_numpy(g['c%d_points' % ci])
        base = torch.from_numpy(np.random.RandomState(ci).choice(len(pts), 333, replace=False).astype(np.int64))
        csr = scene2chunks_csr(pts, (1.5, 1.5), float(stride), thresh=int(thresh), margin=(0.2, 0.2), base_point_ind=base)
        idx, boxes = scene2chunks_legacy(pts, (1.5, 1.5), float(stride), thresh=int(thresh), margin=(0.2, 0.2), return_bbox=True)
        assert csr['lengths'] == g['c%d_lengths' % ci].tolist() == [len(i) for i in idx]
        assert csr['offsets'].dtype == torch.int64 and csr['offsets'].tolist() == np.concatenate([[0], np.cumsum(csr['lengths'])]).tolist()
        np.testing.assert_array_equal(csr['index'].numpy(), g['c%d_indices' % ci])
        np.testing.assert_array_equal(csr['boxes'].numpy(), g['c%d_boxes' % ci])
        assert csr['boxes'].dtype == torch.float64 and torch.equal(csr['boxes'], torch.stack(boxes))
        masks = SO.chunk_masks_of([i.numpy() for i in idx], base.numpy(), len(pts))
        assert np.array_equal(csr['base_bits'].numpy().view(np.uint32), SO.pack_bits(masks))
    none = scene2chunks_csr(torch.from_numpy(g['c0_points']), (1.5, 1.5), 1.0, thresh=10 ** 9)  # nothing kept
    assert none['lengths'] == [] and none['offsets'].tolist() == [0] and none['index'].numel() == 0 and tuple(none['boxes'].shape) == (0, 6)
    assert none['base_bits'] is None


def test_the_numpy_oracle_equals_the_reference():
    """tests/scene_ragged_oracle.scene_chunks (what the GPU tests hold the kernel to) gives the reference's own lists."""
    from mvpnet_amd.chunks import _window_corners
    g = load_golden('chunker')
    for ci in range(3):
        stride, thresh = g['c%d_args' % ci]
        pts = g['c%d_points' % ci]
        corners = _window_corners(torch.from_numpy(pts), np.array([1.5, 1.5]), float(stride))
        o = RO.scene_chunks(pts, corners, (1.5, 1.5), (0.2, 0.2), int(thresh))
        assert o['lengths'].tolist() == g['c%d_lengths' % ci].tolist() and np.array_equal(o['index'], g['c%d_indices' % ci])
        assert np.array_equal(o['zbox'].astype(np.float64), g['c%d_boxes' % ci][:, [2, 5]])


def test_cpu_tensors_and_bad_arguments_raise():
    import mvpnet_amd.ops as ops
    from mvpnet_amd.scene import prepare_scene_bucketed
    pts = torch.rand(100, 3)
    with pytest.raises(RuntimeError):
        ops.scene_chunks(pts, torch.zeros(2, 2), (1.5, 1.5), (0.2, 0.2), 1)  # no CPU path behind the op itself
    with pytest.raises(RuntimeError):
        ops.pack_chunks(pts, torch.arange(10), torch.tensor([0, 10]), [10], [0], [16])
    with pytest.raises(RuntimeError):
        prepare_scene_bucketed(pts, torch.zeros(2, 4, 4), np.eye(4, dtype=np.float32), torch.eye(4).expand(2, 4, 4), torch.zeros(2, 3, 4, 4),
                               chunk_size=(1.5, 1.5), chunk_stride=1.0, chunk_thresh=1, chunk_margin=(0.2, 0.2), num_rgbd_frames=3, k=3,
                               num_base_pts=10)


def test_entry_points_refuse_before_launching():
    """MVP_ENULL / MVP_EINVAL / MVP_EUNSUPPORTED come back before any HIP call (safe without a GPU)."""
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    host = lambda *v: (ctypes.c_int64 * len(v))(*v)
    cnt = lambda n, nc, sx=1.5: lib.mvp_scene_chunks_count_f32(d, n, d, nc, sx, 1.5, 0.2, 0.2, d, d, None)
    assert lib.mvp_scene_chunks_count_f32(None, 8, d, 1, 1.5, 1.5, 0.2, 0.2, d, d, None) == -3
    assert cnt(0, 1) == -1 and cnt(8, 0) == -1 and cnt(8, 1, float('nan')) == -1
    assert cnt(2 ** 31, 1) == -2 and cnt(8, 65536) == -2
    fill = lambda n=8, nc=4, C=2, nb=0, total=5, bp=None, bits=None: lib.mvp_scene_chunks_fill_f32(d, n, d, nc, 1.5, 1.5, 0.2, 0.2, d, d, C, bp, nb, d, total,
                                                                                                d, bits, None)
    assert fill(nb=3) == -3 and fill(C=-1) == -1 and fill(total=-1) == -1
    assert fill(nb=4097, bp=d, bits=d) == -2 and fill(n=2 ** 31) == -2 and fill(nc=65536) == -2 and fill(C=65536) == -2
    assert fill(C=0) == 0  # nothing to do, nothing launched
    pack = lambda lengths, out_len, n=8: lib.mvp_pack_chunks_f32(d, n, d, 5, d, len(lengths), d, d, host(*lengths), host(*out_len), 0, d, 10 ** 6, None)
    assert pack([0], [4]) == -1 and pack([3, 5], [4, 4]) == -1 and pack([3], [4], n=0) == -1
    assert pack([3], [2 ** 31]) == -2 and pack([3], [4], n=2 ** 31) == -2
    assert lib.mvp_pack_chunks_f32(d, 8, d, 5, d, 1, d, d, None, host(4), 0, d, 100, None) == -3
    assert lib.mvp_pack_chunks_f32(d, 8, d, 5, d, 0, d, d, host(), host(), 0, d, 0, None) == 0

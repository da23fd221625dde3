"""Scene preparation without a GPU: the NumPy oracle of the RGB-D overlap and of batched frame selection against the committed fixture
(tests/golden/scene_prep.npz, written by tests/golden/make_scene_prep_golden.py), the oracle's selection against
chunks.select_frames, the argument checks of the three new entry points, and the synthetic scene's determinism."""
import ctypes

import numpy as np
import pytest
import torch

from tests import scene_prep_oracle as SO


@pytest.fixture(scope='module')
def scene():
    return SO.fixture_scene()


@pytest.fixture(scope='module')
def fixture(golden):
    return golden('scene_prep')


def test_make_rgbd_scene_is_deterministic(scene, fixture):
    from mvpnet_amd.synthetic import make_rgbd_scene
    P = SO.FIXTURE
    again = make_rgbd_scene(P['scene_id'], P['n_frames'], n_pts=P['n_pts'], h=P['h'], w=P['w'])
    for key in ('points', 'depth_mm', 'cam_matrix', 'kinv', 'pose'):
        assert np.array_equal(scene[key], again[key]), key
    other = make_rgbd_scene(P['scene_id'] + 1, 8, n_pts=1000, h=P['h'], w=P['w'])
    assert not np.array_equal(other['points'], scene['points'][:1000])
    # the scene the fixture was made from
    assert float(scene['points'].astype(np.float64).sum()) == float(fixture['points_sum'])
    assert int(scene['depth_mm'].astype(np.int64).sum()) == int(fixture['depth_sum'])
    F = P['n_frames']
    assert scene['points'].shape == (P['n_pts'], 3) and scene['points'].dtype == np.float32
    assert scene['depth_mm'].shape == (F, P['h'], P['w']) and scene['depth_mm'].dtype == np.uint16
    assert np.isinf(scene['pose'][F // 2]).all() and np.isfinite(np.delete(scene['pose'], F // 2, 0)).all()
    assert np.array_equal(scene['depth_mm'][-1], scene['depth_mm'][F // 3]) and np.array_equal(scene['pose'][-1], scene['pose'][F // 3])
    invalid = (scene['depth_mm'] == 0).mean()
    assert 0.03 <= invalid < 0.5
    down = scene['pose'][np.isfinite(scene['pose']).all((1, 2))][:, 2, 2]  # z of the viewing direction
    assert (down < -0.5).any() and (down > 0.2).any(), 'floor-facing and upward views'


def test_oracle_overlap_matches_the_fixture(scene, fixture):
    P = SO.FIXTURE
    base = scene['points'][fixture['base_point_ind']]
    overlaps = SO.rgbd_overlap(scene['depth_mm'], scene['kinv'], scene['pose'], base, P['radius'])
    assert overlaps.shape == (P['num_base_pts'], P['n_frames'])
    assert np.array_equal(SO.pack_bits(overlaps.T), fixture['overlap_bits'])
    assert np.array_equal(SO.unpack_bits(fixture['overlap_bits'], P['num_base_pts']).T, overlaps)
    assert not overlaps[:, P['n_frames'] // 2].any()  # the frame with the inf pose
    assert overlaps.any(0).sum() >= P['n_frames'] - 2
    # float32 metres give what uint16 millimetres give (the conversion is part of the definition)
    sub = slice(0, 6)
    depth_m = scene['depth_mm'][sub].astype(np.float32) / np.float32(1000.)
    assert np.array_equal(SO.rgbd_overlap(depth_m, scene['kinv'], scene['pose'][sub], base, P['radius']), overlaps[:, sub])


def test_oracle_selection_matches_the_fixture_and_select_frames(scene, fixture):
    from mvpnet_amd.chunks import select_frames
    P = SO.FIXTURE
    nb, n = P['num_base_pts'], P['num_rgbd_frames']
    overlaps = SO.unpack_bits(fixture['overlap_bits'], nb).T
    masks = SO.chunk_masks_of(scene['chunk_inds'], fixture['base_point_ind'], P['n_pts'])
    assert np.array_equal(SO.pack_bits(masks), fixture['chunk_bits'])
    picked, gain = SO.select_frames_batched(overlaps, masks, n)
    assert np.array_equal(picked, fixture['picked']) and np.array_equal(gain, fixture['gain'])
    ov_t = torch.from_numpy(overlaps)
    for c in range(len(masks)):
        assert select_frames(ov_t[torch.from_numpy(masks[c])], n) == list(picked[c]), c
    # what the fixture promises: a chunk no frame sees (frame 0 again and again) and exact ties at a pick's maximum
    unseen = [c for c in range(len(masks)) if masks[c].any() and not overlaps[masks[c]].any()]
    assert unseen and all((picked[c] == 0).all() and (gain[c] == 0).all() for c in unseen)
    first = np.stack([overlaps[m].sum(0) for m in masks])  # (C,F) scores of the first pick
    assert ((first == first.max(1, keepdims=True)).sum(1) > 1)[first.max(1) > 0].any()
    assert (gain.sum(1) == np.stack([overlaps[m][:, list(p)].any(1).sum() for m, p in zip(masks, picked)])).all()


def test_bit_rows_round_trip():
    from mvpnet_amd.ops import pack_bits, unpack_bits
    rs = np.random.RandomState(5)
    for R, nb in ((3, 1), (5, 31), (4, 32), (7, 33), (2, 2000), (0, 40)):
        m = rs.rand(R, nb) < 0.4
        bits = pack_bits(torch.from_numpy(m))
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (R, (nb + 31) // 32)
        assert np.array_equal(bits.numpy().view(np.uint32), SO.pack_bits(m))
        assert np.array_equal(unpack_bits(bits, nb).numpy(), m)


def test_argument_errors_do_not_launch():
    """Precondition failures of the new entry points return MVP_E* before any HIP call (safe without a GPU)."""
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    for name in ('mvp_frame_overlap_f32', 'mvp_frame_overlap_u16'):
        fn = getattr(lib, name)
        assert fn(None, d, d, d, 1, 60, 80, 2000, 0.1, d, None) == -3             # MVP_ENULL
        assert fn(d, None, d, d, 1, 60, 80, 2000, 0.1, d, None) == -3
        assert fn(d, d, None, d, 1, 60, 80, 2000, 0.1, d, None) == -3
        assert fn(d, d, d, None, 1, 60, 80, 2000, 0.1, d, None) == -3
        assert fn(d, d, d, d, 1, 60, 80, 2000, 0.1, None, None) == -3
        assert fn(d, d, d, d, 1, 60, 80, 4097, 0.1, d, None) == -2                # more base points than fit in LDS: MVP_EUNSUPPORTED
        assert fn(d, d, d, d, 1, 60, 80, 0, 0.1, d, None) == -1                   # MVP_EINVAL
        assert fn(d, d, d, d, 1, 0, 80, 2000, 0.1, d, None) == -1
        assert fn(d, d, d, d, -1, 60, 80, 2000, 0.1, d, None) == -1
        assert fn(d, d, d, d, 1 << 19, 64, 64, 2000, 0.1, d, None) == -1          # F * h * w >= 2^31
        assert fn(d, d, d, d, 1, 1 << 32, 1 << 32, 2000, 0.1, d, None) == -1       # h * w would overflow int64
        assert fn(d, d, d, d, 1, 1 << 62, 4, 2000, 0.1, d, None) == -1
        assert fn(d, d, d, d, 1, 60, 80, 2000, -0.1, d, None) == -1
        assert fn(d, d, d, d, 1, 60, 80, 2000, float('nan'), d, None) == -1
        assert fn(d, d, d, d, 0, 60, 80, 2000, 0.1, d, None) == 0                 # nothing to do
    sel = lib.mvp_select_frames_u32
    assert sel(None, d, 4, 2, 63, 3, d, None, None) == -3
    assert sel(d, None, 4, 2, 63, 3, d, None, None) == -3
    assert sel(d, d, 4, 2, 63, 3, None, None, None) == -3
    assert sel(d, d, 0, 2, 63, 3, d, None, None) == -1                            # no frame to pick from
    assert sel(d, d, 4, 2, 0, 3, d, None, None) == -1
    assert sel(d, d, 4, -1, 63, 3, d, None, None) == -1
    assert sel(d, d, 4, 2, 63, -1, d, None, None) == -1
    assert sel(d, d, 4, 2, 1025, 3, d, None, None) == -2                          # uncovered set does not fit in LDS
    assert sel(d, d, 4, 0, 63, 3, d, None, None) == 0
    assert sel(d, d, 4, 2, 63, 0, d, None, None) == 0


def test_no_cpu_fallback():
    import mvpnet_amd.ops as ops
    from mvpnet_amd.chunks import compute_rgbd_overlap
    depth = torch.zeros(2, 6, 8)
    kinv = torch.eye(3).expand(2, 3, 3).contiguous()
    pose = torch.eye(4).expand(2, 4, 4).contiguous()
    base = torch.rand(40, 3)
    with pytest.raises(RuntimeError):
        ops.rgbd_overlap(depth, kinv, pose, base)
    with pytest.raises(RuntimeError):
        ops.select_frames_batched(torch.zeros(40, 2, dtype=torch.bool), torch.zeros(3, 40, dtype=torch.bool), 3)
    with pytest.raises(RuntimeError):
        ops.select_frames_batched(torch.zeros(2, 2, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError):
        compute_rgbd_overlap(torch.rand(100, 3), depth, np.eye(3, dtype=np.float32), pose, num_base_pts=40)

"""The fused scene cloud without a GPU: the NumPy oracle (tests/fuse_cloud_oracle.py) on the synthetic recording and on a hand-made case
whose voxels can be counted by hand, the argument errors of the Python entries on CPU tensors, and the C entries' refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fuse_cloud_oracle as FO

B = FO.INDEX_BIAS


def key_of(ix, iy, iz):
    return ((iz + B) << 42) | ((iy + B) << 21) | (ix + B)


@pytest.fixture(scope='module')
def recording():
    from mvpnet_amd.synthetic import make_rgbd_scene
    sc = make_rgbd_scene(3, 12)
    xyz, mask = FO.unproject_host(sc['depth_mm'], sc['kinv'], sc['pose'])
    return dict(sc=sc, xyz=xyz, mask=mask)


@pytest.mark.parametrize('voxel,voxels,largest,singles', [(0.05, 15894, 29, 4423), (0.25, 933, 313, 7)])
def test_oracle_on_the_synthetic_recording(recording, voxel, voxels, largest, singles):
    xyz, mask = recording['xyz'], recording['mask']
    assert mask.size == 57600 and mask[6].any()  # (frame 6 carries the non-finite pose; its camera depth is still positive)
    got = FO.fuse(xyz, mask, voxel)
    assert got['n_valid'] == 47782 and got['pixel_point'][6].max() == -1, 'the frame with the non-finite pose adds nothing'
    assert (got['keys'].size, int(got['count'].max()), int((got['count'] == 1).sum())) == (voxels, largest, singles)
    assert got['keys'].dtype == np.uint64 and bool((np.diff(got['keys'].astype(object)) > 0).all()), 'keys strictly ascending'
    assert int(got['count'].sum()) == got['n_valid'] and got['points'].min() < 0 < 6.5 < got['points'].max()
    back = FO.fuse(xyz[::-1], mask[::-1], voxel)
    for name in ('keys', 'count'):
        assert np.array_equal(got[name], back[name]), name
    assert np.array_equal(got['points'].view(np.int32), back['points'].view(np.int32)), 'the same point bits in reverse frame order'
    assert np.array_equal(got['pixel_point'], back['pixel_point'][::-1])
    two = FO.fuse(xyz, mask, voxel, min_samples=2)
    assert two['keys'].size == voxels - singles and int((two['pixel_point'] >= 0).sum()) == got['n_valid'] - singles


def hand_case():
    """2 frames of 4x4, voxel 0.25, every number a short binary fraction so that voxel faces are hit exactly.
    Frame 0: rays (u, v, 1), depth 0.25, moved by t = (-0.75, 0, 0): X = (u/4 - 0.75, v/4, 0.25) -- x on a voxel face for every u, negative for
    u < 3, z on the face between the voxels 0 and 1; pixel (0,0) has zero depth.  Frame 1: z_ray = 1 - u, so only column 0 is in front of
    the camera (column 1 has z_cam = 0, columns 2 and 3 z_cam < 0): X = (0, v*d, d) with d = 0.5, and d = 0.375 in row 1."""
    depth = np.full((2, 4, 4), 0.25, np.float32)
    depth[0, 0, 0] = 0.0
    depth[1] = 0.5
    depth[1, 1, 0] = 0.375
    kinv = np.stack([np.eye(3, dtype=np.float32)] * 2)
    kinv[1, 2] = (-1.0, 0.0, 1.0)
    pose = np.stack([np.eye(4, dtype=np.float32)] * 2)
    pose[0, 0, 3] = -0.75
    return depth, kinv, pose


def test_oracle_on_the_hand_made_case():
    depth, kinv, pose = hand_case()
    xyz, mask = FO.unproject_host(depth, kinv, pose)
    assert int(mask[0].sum()) == 15 and not mask[0, 0, 0], 'zero depth'
    assert mask[1, :, 0].all() and not mask[1, :, 1:].any(), 'z_cam <= 0'
    assert np.array_equal(xyz[0, 2, 1], np.float32([-0.5, 0.5, 0.25])) and np.array_equal(xyz[1, 1, 0], np.float32([0.0, 0.375, 0.375]))
    got = FO.fuse(xyz, mask, 0.25)
    want = {key_of(u - 3, v, 1) for v in range(4) for u in range(4) if (v, u) != (0, 0)}   # a point ON a face belongs to the upper voxel
    want |= {key_of(0, 0, 2), key_of(0, 1, 1), key_of(0, 4, 2), key_of(0, 6, 2)}
    assert got['n_valid'] == 19 and len(want) == 18
    assert [int(k) for k in got['keys']] == sorted(want)
    shared = [int(k) for k in got['keys']].index(key_of(0, 1, 1))    # frame 0 pixel (1,3) and frame 1 pixel (1,0)
    assert got['count'][shared] == 2 and int(got['count'].sum()) == 19
    assert np.array_equal(got['points'][shared], np.float32([0.0, 0.3125, 0.3125]))
    assert got['pixel_point'][0, 1, 3] == got['pixel_point'][1, 1, 0] == shared
    assert got['pixel_point'][0, 0, 0] == -1 and (got['pixel_point'][1, :, 1:] == -1).all()
    neg = [int(k) for k in got['keys']].index(key_of(-3, 1, 1))      # x = -0.75 exactly: index -3, not -2 (floor, not truncation)
    assert np.array_equal(got['points'][neg], np.float32([-0.75, 0.25, 0.25])) and got['pixel_point'][0, 1, 0] == neg
    # colours: the mean rounds half up, (2 s + c) / (2 c)
    images = np.zeros((2, 4, 4, 3), np.uint8)
    images[0, 1, 3], images[1, 1, 0] = (10, 0, 255), (11, 1, 255)
    col = FO.fuse(xyz, mask, 0.25, images=images)['colors']
    assert col.dtype == np.uint8 and tuple(col[shared]) == (11, 1, 255)
    # a depth bound acts on the float32 depth, both ends included
    near = FO.fuse(xyz, mask, 0.25, depth=depth, depth_max=0.375)
    assert near['n_valid'] == 16 and near['pixel_point'][1, 1, 0] >= 0 and near['pixel_point'][1, 0, 0] == -1
    mm = FO.fuse(*FO.unproject_host((depth * 1000).astype(np.uint16), kinv, pose), 0.25)
    assert np.array_equal(mm['keys'], got['keys']) and np.array_equal(mm['count'], got['count'])


def cpu_frames(F=2, h=4, w=4):
    depth, kinv, pose = (torch.from_numpy(a) for a in hand_case())
    return depth[:F, :h, :w].contiguous(), kinv[:F].contiguous(), pose[:F].contiguous(), torch.zeros((F, h, w, 3), dtype=torch.uint8)


def test_argument_errors_on_cpu_tensors():
    from mvpnet_amd import ops, scene
    from mvpnet_amd.ops.fuse_cloud import CloudFuser
    depth, kinv, pose, images = cpu_frames()
    with pytest.raises(RuntimeError, match=r'fuse_cloud: depth must be float32 \(m\) or \(u\)int16'):
        ops.fuse_cloud(depth.double(), kinv, pose, voxel=0.25)
    with pytest.raises(RuntimeError, match=r'fuse_cloud: depth must be \(F,h,w\)'):
        ops.fuse_cloud(depth[0], kinv, pose, voxel=0.25)
    with pytest.raises(RuntimeError, match='fuse_cloud: kinv must be'):
        ops.fuse_cloud(depth, kinv.double(), pose, voxel=0.25)
    with pytest.raises(RuntimeError, match='fuse_cloud: pose must be'):
        ops.fuse_cloud(depth, kinv, pose[:1], voxel=0.25)
    with pytest.raises(RuntimeError, match='fuse_cloud: images must be'):
        ops.fuse_cloud(depth, kinv, pose, images.float(), voxel=0.25)
    for bad in (0.0, -0.05, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='voxel must be a finite length > 0'):
            ops.fuse_cloud(depth, kinv, pose, voxel=bad)
        with pytest.raises(ValueError, match='voxel'):
            CloudFuser(bad, 100, 'cpu')
        with pytest.raises(ValueError, match='voxel'):
            scene.scene_from_rgbd(depth, np.eye(4, dtype=np.float32), pose, images, voxel=bad)
    with pytest.raises(ValueError, match='max_voxels'):
        CloudFuser(0.05, 0, 'cpu')
    with pytest.raises(ValueError, match='max_voxels'):
        CloudFuser(0.05, 2 ** 30 + 1, 'cpu')
    assert CloudFuser(0.05, 512, 'cpu').capacity == 1024 and CloudFuser(0.05, 513, 'cpu').capacity == 2048
    with pytest.raises(RuntimeError, match='GPU only'):       # CPU tensors like any others: no fallback
        ops.fuse_cloud(depth, kinv, pose, images, voxel=0.25)
    with pytest.raises(RuntimeError, match='GPU only'):
        scene.scene_from_rgbd(depth, np.eye(4, dtype=np.float32), pose, images, voxel=0.25)
    with pytest.raises(RuntimeError, match='scene_from_rgbd|fuse_cloud: images must be'):
        scene.scene_from_rgbd(depth, np.eye(4, dtype=np.float32), pose, images[:, :2], voxel=0.25)
    fuser = CloudFuser(0.25, 100, 'cpu', colors=False)
    with pytest.raises(RuntimeError, match='colors=False'):
        fuser.add(depth, kinv, pose, images)
    with pytest.raises(RuntimeError, match='no frames were added'):
        fuser.finish()
    with pytest.raises(RuntimeError, match='call finish first'):
        fuser.lookup(depth, kinv, pose)


def test_mixed_colour_and_plain_add_calls_are_refused(monkeypatch):
    """The rule is the fuser's own bookkeeping: with the launches replaced by nothing it shows on CPU tensors."""
    from mvpnet_amd import _lib as L
    from mvpnet_amd.ops.fuse_cloud import CloudFuser
    launched = []
    monkeypatch.setattr(L, 'require_gpu', lambda *tensors: None)
    monkeypatch.setattr(L, 'call', lambda name, *args, **kw: launched.append(name))
    depth, kinv, pose, images = cpu_frames()
    fuser = CloudFuser(0.25, 100, 'cpu')
    fuser.add(depth, kinv, pose, images).add(depth.mul(1000).to(torch.int16), kinv[0], pose)
    assert launched == ['mvp_fuse_cloud_insert_f32', 'mvp_fuse_cloud_insert_u16']
    with pytest.raises(RuntimeError, match='1 add calls gave images and 1 did not'):
        fuser.finish()
    assert len(launched) == 2
    with pytest.raises(ValueError, match='min_samples'):
        CloudFuser(0.25, 100, 'cpu').add(depth, kinv, pose).finish(0)


def test_the_c_entries_refuse_before_any_launch():
    from mvpnet_amd import _lib as L
    lib = L.lib()
    d = ctypes.c_void_p(16)
    inf = float('inf')
    assert lib.mvp_fuse_cloud_table_bytes(1024, 1) == 1024 * 60 + 8 and lib.mvp_fuse_cloud_table_bytes(1024, 0) == 1024 * 36 + 8
    assert lib.mvp_fuse_cloud_table_bytes(1, 0) % 8 == 0 and lib.mvp_fuse_cloud_table_bytes(1, 0) >= 44
    assert lib.mvp_fuse_cloud_table_bytes(3, 0) == 0 and lib.mvp_fuse_cloud_table_bytes(0, 1) == 0 and lib.mvp_fuse_cloud_table_bytes(2 ** 31, 1) == 0
    for name in ('mvp_fuse_cloud_insert_f32', 'mvp_fuse_cloud_insert_u16'):
        def insert(depth=d, F=2, h=4, w=4, voxel=0.05, lo=-inf, hi=inf, table=d, cap=64, colors=1, images=d):
            return getattr(lib, name)(depth, d, d, images, F, h, w, voxel, lo, hi, table, cap, colors, None)
        assert insert(depth=None) == -3 and insert(table=None) == -3 and insert(depth=None, voxel=0.0) == -3
        for voxel in (0.0, -1.0, inf, float('nan')):
            assert insert(voxel=voxel) == -1
        assert insert(cap=48) == -1 and insert(cap=0) == -1 and insert(h=0) == -1 and insert(F=-1) == -1
        assert insert(lo=float('nan')) == -1 and insert(colors=0) == -1
        assert insert(cap=2 ** 31) == -2 and insert(F=2 ** 15, h=2 ** 8, w=2 ** 8) == -2 and insert(F=1, h=2 ** 16, w=2 ** 16) == -2
        assert insert(F=0) == 0, 'no frames: nothing is launched'
    for name in ('mvp_fuse_cloud_lookup_f32', 'mvp_fuse_cloud_lookup_u16'):
        def lookup(depth=d, F=2, h=4, w=4, voxel=0.05, cap=64, rank=d, out=d):
            return getattr(lib, name)(depth, d, d, F, h, w, voxel, -inf, inf, d, cap, rank, out, None)
        assert lookup(depth=None) == -3 and lookup(rank=None) == -3 and lookup(out=None) == -3
        assert lookup(voxel=-0.5) == -1 and lookup(cap=100) == -1 and lookup(cap=2 ** 31) == -2 and lookup(F=2 ** 15, h=2 ** 8, w=2 ** 8) == -2
        assert lookup(F=0) == 0

    def finish(table=d, cap=64, colors=1, slots=d, n=8, points=d, col=d, counts=d, rank=d):
        return lib.mvp_fuse_cloud_finish(table, cap, colors, slots, n, points, col, counts, rank, None)
    assert finish(table=None) == -3 and finish(slots=None) == -3 and finish(points=None) == -3 and finish(counts=None) == -3 and finish(rank=None) == -3
    assert finish(cap=65) == -1 and finish(n=-1) == -1 and finish(n=65) == -1 and finish(colors=0) == -1 and finish(cap=2 ** 31, n=1) == -2
    assert finish(n=0) == 0 and finish(n=0, col=None, colors=0) == 0

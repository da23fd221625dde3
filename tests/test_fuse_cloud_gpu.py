"""ops.fuse_cloud / CloudFuser / scene.scene_from_rgbd / scene.infer_rgbd on the MI355X against the NumPy restatement
(tests/fuse_cloud_oracle.py) fed with ops.unproject's world points.  Every comparison is bit-equal; no tolerance appears anywhere."""
import numpy as np
import pytest
import torch

from tests import fuse_cloud_oracle as FO
from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def world(depth, kinv, pose):
    """ops.unproject's float32 world points and mask of frames (F,h,w) -> host arrays (F,h,w,3), (F,h,w)."""
    from mvpnet_amd import ops
    F = depth.size(0)
    kinv = kinv.expand(F, 3, 3) if kinv.dim() == 2 else kinv
    xyz, mask = ops.unproject(depth[None].contiguous(), kinv[None].contiguous(), pose[None].contiguous())
    return xyz[0].cpu().numpy(), mask[0].cpu().numpy()


def assert_cloud(got, want, what=''):
    """got: (points, colors, count[, pixel_point]) device tensors; want: the oracle's dict."""
    points, colors, count = got[:3]
    assert points.dtype == torch.float32 and tuple(points.shape) == want['points'].shape, what
    assert torch.equal(bits(points), bits(t(want['points']))), what + ' points'
    assert count.dtype == torch.int32 and torch.equal(count, t(want['count'])), what + ' count'
    if want['colors'] is None:
        assert colors is None, what
    else:
        assert colors.dtype == torch.uint8 and torch.equal(colors, t(want['colors'])), what + ' colors'
    if len(got) > 3:
        assert got[3].dtype == torch.int32 and torch.equal(got[3], t(want['pixel_point'])), what + ' pixel_point'


# ---- hand-made frames ------------------------------------------------------------------------------------------------------------
def hand_frames():
    """3 frames of 6x8, voxel 0.25, every number a short binary fraction (exact in float32 and in millimetres).
    Frame 0: rays (u, v, 1), depth 0.25, t = (-0.75, 0, 0): X = (u/4 - 0.75, v/4, 0.25): every x ON a voxel face, negative for u < 3; two
    zero depths; pixel (1,2) at depth 0.375 lands at (0, 0.375, 0.375), in the voxel of pixel (1,3).
    Frame 1: z_ray = 1 - u (only column 0 in front of the camera) and t_y = 32767.5: row 0 has y = 32767.5 (inside), rows >= 1 have
    y >= 32768 (outside the coordinate range).  Frame 2: a non-finite pose."""
    depth = np.full((3, 6, 8), 0.25, np.float32)
    depth[0, 0, 0] = depth[0, 5, 7] = 0.0
    depth[0, 1, 2] = 0.375
    depth[1] = 0.5
    kinv = np.stack([np.eye(3, dtype=np.float32)] * 3)
    kinv[1, 2] = (-1.0, 0.0, 1.0)
    pose = np.stack([np.eye(4, dtype=np.float32)] * 3)
    pose[0, 0, 3] = -0.75
    pose[1, 1, 3] = 32767.5
    pose[2] = np.inf
    images = np.random.RandomState(5).randint(0, 256, (3, 6, 8, 3)).astype(np.uint8)
    return depth, kinv, pose, images


@pytest.mark.parametrize('kind', ['f32', 'u16'])
def test_hand_made_frames(kind):
    from mvpnet_amd import ops
    depth, kinv, pose, images = hand_frames()
    depth = t(depth) if kind == 'f32' else t((depth * 1000).astype(np.int16))
    kinv, pose, images = t(kinv), t(pose), t(images)
    xyz, mask = world(depth, kinv, pose)
    want = FO.fuse(xyz, mask, 0.25, images=images.cpu().numpy())
    # the case holds what it was made for
    pp = want['pixel_point']
    assert (pp[0] >= 0).sum() == 46 and pp[0, 0, 0] == pp[0, 5, 7] == -1, 'zero depth'
    assert pp[0, 1, 2] == pp[0, 1, 3] >= 0 and want['count'][pp[0, 1, 3]] == 2, 'two pixels share a voxel'
    assert xyz[0, 1, 0, 0] == -0.75 and pp[0, 1, 0] >= 0, 'a negative coordinate on a voxel face'
    assert pp[1, 0, 0] >= 0 and (pp[1].reshape(-1)[1:] == -1).all() and xyz[1, 1, 0, 1] == 32768.0, 'z_cam <= 0 and the coordinate range'
    assert (pp[2] == -1).all() and mask[2].any(), 'the non-finite pose'
    got = ops.fuse_cloud(depth, kinv, pose, images, voxel=0.25)
    assert_cloud(got, want, kind)
    # a voxel with one sample gives back ops.unproject's row (here every coordinate is a multiple of 2^-16)
    points, _, count, pixel_point = got
    one = (pixel_point >= 0) & (count[pixel_point.clamp(min=0).long()] == 1)
    assert int(one.sum()) == 45
    assert torch.equal(bits(points[pixel_point[one].long()]), bits(t(xyz)[one]))
    # without colours, and per-frame against shared intrinsics
    plain = ops.fuse_cloud(depth[:1], kinv[0], pose[:1], voxel=0.25)
    assert_cloud(plain, FO.fuse(xyz[:1], mask[:1], 0.25), kind + ' one frame')


def test_contention_on_one_voxel():
    """One 64x64 frame of a flat wall at 0.3 m inside one 4 m voxel: 4096 pixels add to the same slot."""
    from mvpnet_amd import ops
    depth = t(np.full((1, 64, 64), 0.3, np.float32))
    kinv = t(np.diag([1 / 64., 1 / 64., 1.]).astype(np.float32))
    pose = t(np.eye(4, dtype=np.float32)[None])
    images = t(np.random.RandomState(6).randint(0, 256, (1, 64, 64, 3)).astype(np.uint8))
    xyz, mask = world(depth, kinv, pose)
    want = FO.fuse(xyz, mask, 4.0, images=images.cpu().numpy())
    assert want['count'].tolist() == [4096]
    got = ops.fuse_cloud(depth, kinv, pose, images, voxel=4.0)
    assert_cloud(got, want)
    assert not got[3].any()


# ---- the synthetic recording -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rec():
    from mvpnet_amd.synthetic import make_rgbd_scene
    sc = make_rgbd_scene(3, 12)
    images = np.random.RandomState(12).randint(0, 256, sc['depth_mm'].shape + (3,)).astype(np.uint8)
    depth, kinv, pose = t(sc['depth_mm'].astype(np.int16)), t(sc['kinv']), t(sc['pose'])
    xyz, mask = world(depth, kinv, pose)
    want = {v: FO.fuse(xyz, mask, v, images=images) for v in (0.05, 0.25)}
    return dict(sc=sc, depth=depth, kinv=kinv, pose=pose, images=t(images), images_np=images, xyz=xyz, mask=mask, want=want)


@pytest.mark.parametrize('voxel,voxels,singles', [(0.05, 15894, 4423), (0.25, 933, 7)])
def test_synthetic_recording(rec, voxel, voxels, singles):
    from mvpnet_amd import ops
    from mvpnet_amd.ops.fuse_cloud import CloudFuser
    want = rec['want'][voxel]
    assert want['keys'].size == voxels and want['n_valid'] == 47782
    depth, kinv, pose, images = rec['depth'], rec['kinv'], rec['pose'], rec['images']
    got = ops.fuse_cloud(depth, kinv, pose, images, voxel=voxel)
    assert_cloud(got, want)
    assert_cloud(ops.fuse_cloud(depth, kinv, pose, images, voxel=voxel), want, 'a second run')
    back = ops.fuse_cloud(depth.flip(0).contiguous(), kinv, pose.flip(0).contiguous(), images.flip(0).contiguous(), voxel=voxel)
    assert_cloud(back[:3], want, 'frames reversed')
    assert torch.equal(back[3].flip(0), got[3])
    fuser = CloudFuser(voxel, 57600, DEV)
    for lo in range(0, 12, 4):
        fuser.add(depth[lo:lo + 4].contiguous(), kinv, pose[lo:lo + 4].contiguous(), images[lo:lo + 4].contiguous())
    assert_cloud(fuser.finish(), want, 'three add calls')
    # lookup reproduces pixel_point, and every pixel's point lies in the voxel of the pixel's own key
    pixel_point = fuser.lookup(depth, kinv, pose)
    assert torch.equal(pixel_point, got[3])
    valid, key = FO.pixel_keys(rec['xyz'], rec['mask'], voxel)
    assert torch.equal(fuser.keys, t(want['keys'].view(np.int64)))
    hit = pixel_point >= 0
    assert torch.equal(hit, t(valid)) and torch.equal(fuser.keys[pixel_point[hit].long()], t(key.view(np.int64))[hit])
    # frames that were not fused: a depth map of the same scene from a shifted camera finds fused voxels or nothing
    other = fuser.lookup(depth[:2], kinv, pose[2:4].contiguous())
    xyz2, mask2 = world(depth[:2], kinv, pose[2:4].contiguous())
    valid2, key2 = FO.pixel_keys(xyz2, mask2, voxel)
    rank = {int(k): r for r, k in enumerate(want['keys'])}
    assert torch.equal(other, t(np.array([rank.get(int(k), -1) if v else -1 for k, v in zip(key2.ravel(), valid2.ravel())], np.int32).reshape(key2.shape)))
    # min_samples = 2 drops exactly the voxels with one sample and turns their pixels to -1
    two = FO.fuse(rec['xyz'], rec['mask'], voxel, images=rec['images_np'], min_samples=2)
    assert two['keys'].size == voxels - singles
    assert_cloud(fuser.finish(min_samples=2) + (fuser.lookup(depth, kinv, pose),), two, 'min_samples=2')
    assert int((got[3] >= 0).sum()) - int((two['pixel_point'] >= 0).sum()) == singles
    # a depth bound
    near = FO.fuse(rec['xyz'], rec['mask'], voxel, images=rec['images_np'], depth=rec['sc']['depth_mm'], depth_max=2.0)
    assert 0 < near['n_valid'] < want['n_valid']
    assert_cloud(ops.fuse_cloud(depth, kinv, pose, images, voxel=voxel, depth_max=2.0), near, 'depth_max=2')
    both = FO.fuse(rec['xyz'], rec['mask'], voxel, depth=rec['sc']['depth_mm'], depth_min=1.5, depth_max=2.0)
    assert_cloud(ops.fuse_cloud(depth, kinv, pose, voxel=voxel, depth_min=1.5, depth_max=2.0), both, 'depth in [1.5, 2]')


# ---- table pressure, operands between guard bands ------------------------------------------------------------------------------------
def _arena(rec, cap, n):
    """The operands of insert / finish / lookup on the voxel-0.25 case carved out of poisoned buffers: a table of `cap` slots with colours."""
    from mvpnet_amd import _lib as L
    nbytes = L.lib().mvp_fuse_cloud_table_bytes(cap, 1)
    table = torch.zeros(nbytes // 8, dtype=torch.int64)
    table[:cap] = -1
    F, h, w = rec['depth'].shape
    a = Arena(DEV)
    a.inp('depth', rec['depth'].cpu(), fill=0).inp('kinv', rec['kinv'].expand(F, 3, 3).contiguous().cpu()).inp('pose', rec['pose'].cpu())
    a.inp('images', rec['images'].cpu(), fill=0)
    a.acc('table', table)
    a.inp('slots', torch.zeros(max(n, 1), dtype=torch.int64), fill=0)
    a.acc('rank_of_slot', torch.full((cap,), -1, dtype=torch.int32))
    a.out('points', (max(n, 1), 3)).out('colors', (max(n, 1), 3), dtype=torch.uint8).out('count', (max(n, 1),), dtype=torch.int32)
    a.out('pixel_point', (F, h, w), dtype=torch.int32)
    return a.build()


def _insert(a, rec, cap):
    from mvpnet_amd import _lib as L
    F, h, w = rec['depth'].shape
    L.call('mvp_fuse_cloud_insert_u16', a['depth'], L.ptr(a['depth']), L.ptr(a['kinv']), L.ptr(a['pose']), L.ptr(a['images']), F, h, w, 0.25,
           float('-inf'), float('inf'), L.ptr(a['table']), cap, 1)
    torch.cuda.synchronize()
    table = a['table']
    tail = table[cap * 7:].view(torch.int32)
    return table[:cap], tail[:cap], int(tail[cap])


def test_a_table_at_load_091_between_guard_bands(rec):
    """max_voxels = 512 -> 1024 slots for 933 voxels: long probe chains, the same cloud; nothing outside the operands changes."""
    from mvpnet_amd import _lib as L
    from mvpnet_amd import ops
    from mvpnet_amd.ops.fuse_cloud import CloudFuser, kept_slots
    want = rec['want'][0.25]
    n, cap = want['keys'].size, 1024
    assert CloudFuser(0.25, 512, DEV).capacity == cap and n == 933
    assert_cloud(ops.fuse_cloud(rec['depth'], rec['kinv'], rec['pose'], rec['images'], voxel=0.25, max_voxels=512), want, 'max_voxels=512')
    a = _arena(rec, cap, n)
    keys, count, overflow = _insert(a, rec, cap)
    assert a.check(nan_ok=('points',)) == [], 'the insert writes its table only'
    assert overflow == 0 and int((count > 0).sum()) == n
    a['slots'].copy_(kept_slots(keys, count >= 1, n))
    a.snap[torch.int64] = a._bits(torch.int64).clone()  # the slots are an input from here on (and the table is only read)
    F, h, w = rec['depth'].shape
    L.call('mvp_fuse_cloud_finish', a['table'], L.ptr(a['table']), cap, 1, L.ptr(a['slots']), n, L.ptr(a['points']), L.ptr(a['colors']),
           L.ptr(a['count']), L.ptr(a['rank_of_slot']))
    L.call('mvp_fuse_cloud_lookup_u16', a['depth'], L.ptr(a['depth']), L.ptr(a['kinv']), L.ptr(a['pose']), F, h, w, 0.25, float('-inf'), float('inf'),
           L.ptr(a['table']), cap, L.ptr(a['rank_of_slot']), L.ptr(a['pixel_point']))
    torch.cuda.synchronize()
    assert a.check() == []
    assert_cloud((a.result('points'), a.result('colors'), a.result('count'), a.result('pixel_point')), want, 'in the arena')
    rank = a.result('rank_of_slot')
    assert int((rank >= 0).sum()) == n and torch.equal(torch.sort(rank[rank >= 0]).values, torch.arange(n, dtype=torch.int32, device=DEV))


def test_a_full_table_is_an_error_and_writes_nothing_outside(rec):
    """max_voxels = 32 -> 64 slots for 933 voxels: the kernel fills the table, sets the overflow word and drops the rest -- an error return
    it must take safely; finish raises."""
    from mvpnet_amd.ops.fuse_cloud import CloudFuser
    want = rec['want'][0.25]
    cap = 64
    fuser = CloudFuser(0.25, 32, DEV)
    assert fuser.capacity == cap
    fuser.add(rec['depth'], rec['kinv'], rec['pose'], rec['images'])
    with pytest.raises(RuntimeError, match=r'max_voxels \(now 32\)'):
        fuser.finish()
    a = _arena(rec, cap, 0)
    keys, count, overflow = _insert(a, rec, cap)
    assert a.check(nan_ok=('points',)) == []   # (no finish here: the outputs stay unwritten)
    assert overflow == 1 and int((keys != -1).sum()) == cap, 'every slot taken'
    held = {int(k): r for r, k in enumerate(want['keys'].view(np.int64))}
    rows = [held[int(k)] for k in keys.tolist()]   # (a KeyError: a key no pixel has)
    assert len(set(rows)) == cap and torch.equal(count, t(want['count'][rows])), 'the voxels that got a slot are complete'


# ---- composition -------------------------------------------------------------------------------------------------------------------
def test_infer_rgbd_composes_scene_from_rgbd_and_infer_scene_shared():
    from mvpnet_amd import chunks, scene
    from mvpnet_amd.pn2 import PN2SSG
    from mvpnet_amd.synthetic import make_rgbd_scene
    from tests.test_scene_prep_gpu import CFG, E2E
    from tests.test_scene_shared_gpu import NORM, _model
    sc = make_rgbd_scene(5, 24)
    F, h, w = sc['depth_mm'].shape
    raw = t(np.random.RandomState(9).randint(0, 256, (F, h, w, 3)).astype(np.uint8))
    depth, pose, cam = t(sc['depth_mm'].astype(np.int16)), t(sc['pose']), sc['cam_matrix']
    cloud = scene.scene_from_rgbd(depth, cam, pose, raw, voxel=0.1)
    xyz, mask = world(depth, t(sc['kinv']), pose)
    want = FO.fuse(xyz, mask, 0.1, images=raw.cpu().numpy())
    assert_cloud((cloud['points'], cloud['colors'], cloud['count'], cloud['pixel_point']), want)
    n = cloud['points'].size(0)
    assert n > 2000

    def kw():
        return dict(num_rgbd_frames=3, k=3, min_nb_pts=E2E['min_nb_pts'], num_base_pts=E2E['num_base_pts'], batch_size=8, pad_seed=11,
                    generator=torch.Generator(device=DEV).manual_seed(7), image_normalizer=NORM, **E2E['chunk'])
    got = scene.infer_rgbd(_model(), depth, cam, pose, raw, voxel=0.1, **kw())
    mean, label, votes = scene.infer_scene_shared(_model(), cloud['points'], depth, cam, pose, raw, **kw())
    for name in ('points', 'colors', 'count', 'pixel_point'):
        assert torch.equal(bits(got[name]), bits(cloud[name])), name
    assert torch.equal(bits(got['mean']), bits(mean)) and torch.equal(got['label'], label) and torch.equal(got['vote_count'], votes)
    assert int((votes > 0).sum()) > n // 2, 'the fused cloud is chunked and labelled'
    C = mean.size(1)
    pp = cloud['pixel_point'].long()
    frames = torch.where(pp >= 0, label[pp.clamp(min=0)], torch.full_like(pp, C))
    assert got['label_frames'].dtype == torch.int64 and torch.equal(got['label_frames'], frames)
    assert bool((got['label_frames'][pp < 0] == C).all()) and bool((pp < 0).any()) and bool((got['label_frames'] < C).any())
    # the other whole-scene calls take the fused cloud as they take a mesh's vertices
    base, overlap = chunks.compute_rgbd_overlap(cloud['points'], depth, cam, pose, num_base_pts=500, generator=torch.Generator(device=DEV).manual_seed(1))
    assert tuple(overlap.shape) == (500, F) and bool(overlap.any()) and not bool(overlap[:, F // 2].any())
    torch.manual_seed(4)
    net = PN2SSG(3, 20, dropout_prob=0.0, **CFG).to(DEV).eval()
    m3, l3, c3 = scene.infer_scene_3d(net, cloud['points'], colors=cloud['colors'], chunk_stride=1.0, chunk_thresh=100, min_nb_pts=1024)
    assert tuple(m3.shape) == (n, 20) and bool(torch.isfinite(m3).all()) and int((c3 > 0).sum()) > n // 2

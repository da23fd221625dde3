"""Deterministic synthetic RGB-D chunks (no dataset), SURVEY.md sec.8(d).

Stands in for what `ScanNet2D3DChunks.__getitem__` hands the model
(reference: mvpnet/data/scannet_2d3d.py:323-416): a 1.5 m chunk (+0.2 m margin)
of `nb_pts` points, `nv` depth views with pin-hole intrinsics scaled to the image
size (scannet_2d3d.py:206-210) and camera-to-world poses, plus a stand-in for the
frozen 2D network's 64-channel feature map.  Everything is NumPy on the host and
seeded with `RandomState(1000 * config + chunk_id)`; no file, no network.
"""
import numpy as np

CHUNK_SIZE = 1.5      # mvpnet/config/mvpnet_3d.py:20
CHUNK_MARGIN = 0.2    # mvpnet/config/mvpnet_3d.py:22
PIXEL_MARGIN = 0.1    # scannet_2d3d.py:275


def _look_at(cam_pos, target):
    """Camera-to-world 4x4 (ScanNet convention: x right, y down, z forward)."""
    fwd = target - cam_pos
    fwd = fwd / np.linalg.norm(fwd)
    up = np.array([0.0, 0.0, 1.0])
    right = np.cross(fwd, up)
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, cam_pos
    return pose.astype(np.float32)


def make_chunk(chunk_id, config=2, nb_pts=8192, nv=3, h=120, w=160, channels=64, k=3,
               with_feature=True, jitter=0.005):
    """One synthetic chunk.  Returns a dict of host arrays:

    depth_mm (nv,h,w) uint16, cam_matrix (4,4) f32 (already scaled to (h,w)),
    kinv (nv,3,3) f32, pose (nv,4,4) f32, chunk_box (4,) f32 (x0,y0,x1,y1 incl. chunk margin),
    pixel_box (4,) f32 (chunk_box -/+ 0.1, what the in-chunk pixel mask tests),
    points (nb_pts,3) f32, seg_label (nb_pts,) int64 (10 % = -100),
    feature_2d (nv,h,w,channels) f32 channels-last (optional).
    """
    rs = np.random.RandomState(1000 * config + chunk_id)
    ext = CHUNK_SIZE + 2 * CHUNK_MARGIN  # 1.9 m box on the xy-plane
    centre = np.array([0.5 * ext, 0.5 * ext, 0.8])

    cam = np.eye(4, dtype=np.float32)
    cam[0, 0] = cam[1, 1] = 577.87 * w / 640.0
    cam[0, 2] = (w - 1) / 2.0
    cam[1, 2] = (h - 1) / 2.0
    kinv1 = np.linalg.inv(cam[:3, :3])  # float32, as scannet_2d3d.py:38

    poses, depths = [], []
    vv, uu = np.indices((h, w))
    for i in range(nv):
        az = np.deg2rad(rs.uniform(20.0, 70.0))
        el = np.deg2rad(rs.uniform(25.0, 50.0))
        dist = rs.uniform(1.5, 2.5)
        pos = centre + dist * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        pose = _look_at(pos, centre + rs.uniform(-0.2, 0.2, 3))
        # ray-cast floor z=0 and the two far walls x=0, y=0
        rays_cam = np.stack([(uu - cam[0, 2]) / cam[0, 0], (vv - cam[1, 2]) / cam[1, 1], np.ones_like(uu, float)], -1)
        rays_w = rays_cam @ pose[:3, :3].astype(np.float64).T
        o = pose[:3, 3].astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.stack([np.where(rays_w[..., a] < 0, -o[a] / rays_w[..., a], np.inf) for a in (2, 0, 1)], -1)
        z = np.min(t, axis=-1)  # depth along camera z because rays_cam[...,2] == 1
        z = z * (1.0 + 0.03 * np.sin(0.11 * uu + 1.3 * i) * np.sin(0.13 * vv + 0.7 * i))
        z = np.where(np.isfinite(z) & (z < 6.5), z, 0.0)
        mm = np.round(z * 1000.0).astype(np.uint16)
        mm[rs.rand(h, w) < 0.03] = 0  # invalid depth
        poses.append(pose)
        depths.append(mm)
    depth_mm = np.stack(depths)
    pose = np.stack(poses)

    chunk_box = np.array([0.0, 0.0, ext, ext], np.float32)
    pixel_box = np.array([chunk_box[0] - PIXEL_MARGIN, chunk_box[1] - PIXEL_MARGIN,
                          chunk_box[2] + PIXEL_MARGIN, chunk_box[3] + PIXEL_MARGIN], np.float32)

    # world coordinates of the pixels (float64 like the reference) to draw the chunk points from
    d = depth_mm.astype(np.float32) / np.float32(1000.0)
    uv1 = np.stack([uu.ravel(), vv.ravel(), np.ones(h * w, np.int64)], 1)
    cand = []
    for i in range(nv):
        xyz = (kinv1.dot(uv1.T) * d[i].ravel()).T
        ok = xyz[:, 2] > 0
        xyz = np.matmul(xyz, pose[i, :3, :3].T) + pose[i, :3, 3]
        ok &= (xyz[:, 0] > chunk_box[0]) & (xyz[:, 0] < chunk_box[2]) & (xyz[:, 1] > chunk_box[1]) & (xyz[:, 1] < chunk_box[3])
        cand.append(xyz[ok])
    cand = np.concatenate(cand, 0)
    if len(cand) == 0:
        raise RuntimeError('synthetic chunk {} has no valid pixel'.format(chunk_id))
    sel = rs.randint(len(cand), size=nb_pts)
    points = (cand[sel] + rs.normal(0.0, jitter, (nb_pts, 3))).astype(np.float32)

    seg_label = rs.randint(0, 20, nb_pts).astype(np.int64)
    seg_label[rs.rand(nb_pts) < 0.1] = -100

    out = dict(depth_mm=depth_mm, cam_matrix=cam, kinv=np.repeat(kinv1[None], nv, 0).astype(np.float32), pose=pose,
               chunk_box=chunk_box, pixel_box=pixel_box, points=points, seg_label=seg_label, k=k)
    if with_feature:
        out['feature_2d'] = rs.standard_normal((nv, h, w, channels)).astype(np.float32)
    return out


def make_batch(first_chunk_id, batch_size, **kw):
    """Stack `batch_size` consecutive chunks along a leading batch axis."""
    chunks = [make_chunk(first_chunk_id + i, **kw) for i in range(batch_size)]
    out = {}
    for key in chunks[0]:
        if key in ('cam_matrix', 'k'):
            out[key] = chunks[0][key]
        else:
            out[key] = np.stack([c[key] for c in chunks])
    return out


def make_scene(scene_id, n_pts=200000, n_chunks=64, nb_pts=8192):
    """Random overlapping `chunk_ind` sets into an n_pts-point scene (config C4):
    what `ScanNet2D3DChunksTest` + scene2chunks_legacy would hand the vote
    (reference: mvpnet/utils/chunk_util.py:4-53, mvpnet/test_mvpnet_3d.py:142-164)."""
    rs = np.random.RandomState(77000 + scene_id)
    return [np.sort(rs.choice(n_pts, nb_pts, replace=False)).astype(np.int64) for _ in range(n_chunks)]


def _ray_box(o, d, lo, hi):
    """Entry distance of rays o + t d (o (3,), d (...,3)) into the axis-aligned box [lo, hi] (slab test); inf where they miss."""
    with np.errstate(divide='ignore', invalid='ignore'):
        t0 = (lo - o) / d
        t1 = (hi - o) / d
    tn = np.nanmax(np.minimum(t0, t1), axis=-1)
    tf = np.nanmin(np.maximum(t0, t1), axis=-1)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf)


def make_rgbd_scene(scene_id, n_frames, n_pts=60000, h=60, w=80, room=(6.5, 5.5, 2.5), n_boxes=4, jitter=0.005, dup_of=None):
    """One synthetic RGB-D SCENE, what the reference's preprocessing reads per scan (preprocess.py:176-260): a room (floor z = 0,
    four walls, `n_boxes` boxes along the walls), its jittered point cloud, and `n_frames` depth frames ray-cast in make_chunk's
    style along a camera path.  The cameras stand on a ring of radius 1.6 m around the room's centre and look OUTWARD -- level,
    up the walls and down at the floor in turn --, so walls, boxes and the outer floor are all seen while the floor inside the ring
    is seen by no frame (a chunk there has all-zero overlap scores).  3 % of the depth pixels are invalid (0), frame n_frames // 2
    has an `inf` pose (ScanNet marks lost tracking that way; preprocess.py:137-139 skips such frames) and the LAST frame repeats
    frame `dup_of` (default n_frames // 3) exactly, which gives frame selection an exact score tie.
    Returns host arrays: points (n_pts,3) f32, depth_mm (F,h,w) uint16, cam_matrix (4,4) f32 scaled to (h,w), kinv (3,3) f32,
    pose (F,4,4) f32.  Seeded with RandomState(91000 + scene_id)."""
    rs = np.random.RandomState(91000 + scene_id)
    lx, ly, lz = room
    centre = np.array([0.5 * lx, 0.5 * ly])
    ring = 1.6
    boxes = []
    for i in range(n_boxes):  # along the walls, outside the ring
        sx, sy, sz = rs.uniform(0.4, 0.9), rs.uniform(0.4, 0.9), rs.uniform(0.4, 1.2)
        side = i % 4
        along = rs.uniform(0.2, 0.8)
        if side == 0:
            x0, y0 = along * (lx - sx), 0.05
        elif side == 1:
            x0, y0 = lx - sx - 0.05, along * (ly - sy)
        elif side == 2:
            x0, y0 = along * (lx - sx), ly - sy - 0.05
        else:
            x0, y0 = 0.05, along * (ly - sy)
        boxes.append((np.array([x0, y0, 0.0]), np.array([x0 + sx, y0 + sy, sz])))

    # point cloud: area-weighted samples of the floor, the walls and the boxes' visible faces, jittered
    surf = [(np.array([0, 0, 0.]), np.array([lx, 0, 0.]), np.array([0, ly, 0.])),
            (np.array([0, 0, 0.]), np.array([lx, 0, 0.]), np.array([0, 0, lz])), (np.array([0, ly, 0.]), np.array([lx, 0, 0.]), np.array([0, 0, lz])),
            (np.array([0, 0, 0.]), np.array([0, ly, 0.]), np.array([0, 0, lz])), (np.array([lx, 0, 0.]), np.array([0, ly, 0.]), np.array([0, 0, lz]))]
    for lo, hi in boxes:
        e = hi - lo
        ex, ey, ez = np.array([e[0], 0, 0.]), np.array([0, e[1], 0.]), np.array([0, 0, e[2]])
        surf += [(lo + ez, ex, ey), (lo, ex, ez), (lo + ey, ex, ez), (lo, ey, ez), (lo + ex, ey, ez)]
    area = np.array([np.linalg.norm(np.cross(a, b)) for _, a, b in surf])
    which = rs.choice(len(surf), n_pts, p=area / area.sum())
    uv = rs.rand(n_pts, 2)
    org = np.stack([s[0] for s in surf])[which]
    ea = np.stack([s[1] for s in surf])[which]
    eb = np.stack([s[2] for s in surf])[which]
    points = (org + uv[:, :1] * ea + uv[:, 1:] * eb + rs.normal(0.0, jitter, (n_pts, 3))).astype(np.float32)

    cam = np.eye(4, dtype=np.float32)
    cam[0, 0] = cam[1, 1] = 577.87 * w / 640.0
    cam[0, 2] = (w - 1) / 2.0
    cam[1, 2] = (h - 1) / 2.0
    kinv = np.linalg.inv(cam[:3, :3])  # float32, as scannet_2d3d.py:38

    vv, uu = np.indices((h, w))
    rays_cam = np.stack([(uu - cam[0, 2]) / cam[0, 0], (vv - cam[1, 2]) / cam[1, 1], np.ones_like(uu, float)], -1)
    pitches = np.deg2rad([0.0, -35.0, 20.0, -55.0])  # level, floor-facing, up the wall, steeply down
    poses, depths = [], []
    for i in range(n_frames):
        az = 2.0 * np.pi * (i + rs.uniform(-0.3, 0.3)) / max(n_frames - 1, 1) * 3.0  # three turns around the ring
        pitch = pitches[i % 4] + np.deg2rad(rs.uniform(-5.0, 5.0))
        out = np.array([np.cos(az), np.sin(az), 0.0])
        pos = np.array([centre[0], centre[1], 0.0]) + ring * out + np.array([0.0, 0.0, rs.uniform(1.1, 1.6)])
        pose = _look_at(pos, pos + np.cos(pitch) * out + np.array([0.0, 0.0, np.sin(pitch)]))
        rays_w = rays_cam @ pose[:3, :3].astype(np.float64).T
        o = pose[:3, 3].astype(np.float64)
        t = [_ray_box(o, rays_w, lo, hi) for lo, hi in boxes]
        with np.errstate(divide='ignore', invalid='ignore'):
            t.append(np.where(rays_w[..., 2] < 0, -o[2] / rays_w[..., 2], np.inf))              # floor
            t.append(np.where(rays_w[..., 0] < 0, -o[0] / rays_w[..., 0], np.inf))              # wall x = 0
            t.append(np.where(rays_w[..., 0] > 0, (lx - o[0]) / rays_w[..., 0], np.inf))        # wall x = lx
            t.append(np.where(rays_w[..., 1] < 0, -o[1] / rays_w[..., 1], np.inf))              # wall y = 0
            t.append(np.where(rays_w[..., 1] > 0, (ly - o[1]) / rays_w[..., 1], np.inf))        # wall y = ly
        z = np.min(np.stack(t, -1), axis=-1)  # depth along camera z because rays_cam[...,2] == 1
        hit_z = o[2] + z * rays_w[..., 2]
        z = np.where(np.isfinite(z) & (z < 6.5) & (hit_z <= lz), z, 0.0)  # above the walls: open ceiling, no return
        mm = np.round(z * 1000.0).astype(np.uint16)
        mm[rs.rand(h, w) < 0.03] = 0  # invalid depth
        poses.append(pose)
        depths.append(mm)
    depth_mm = np.stack(depths)
    pose = np.stack(poses)
    if n_frames >= 2:
        src = n_frames // 3 if dup_of is None else int(dup_of)
        depth_mm[-1] = depth_mm[src]
        pose[-1] = pose[src]
    if n_frames >= 3:
        pose[n_frames // 2] = np.inf
    return dict(points=points, depth_mm=depth_mm, cam_matrix=cam, kinv=kinv.astype(np.float32), pose=pose)

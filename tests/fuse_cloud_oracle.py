"""NumPy restatement of the fused scene cloud (include/mvp_hip.h, mvp_fuse_cloud_*; plain helper module): np.unique on the voxel keys,
np.add.at on int64 sums, one float64 expression per output.  Nothing here shares code with the kernels.

The float32 world points and the z_cam > 0 mask come from outside: on the GPU from ops.unproject, on the CPU from `unproject_host`, the
float64 un-projection written operation by operation as csrc/unproject_core.h writes it."""
import numpy as np

INDEX_BIAS = 1 << 20


def depth_metres(depth):
    """float32 metres as stored, or (u)int16 millimetres / 1000 in float32 (unproject_core.h, depth_metres)."""
    depth = np.asarray(depth)
    if depth.dtype == np.float32:
        return depth
    assert depth.dtype in (np.uint16, np.int16)
    return depth.view(np.uint16).astype(np.float32) / np.float32(1000.0)


def unproject_host(depth, kinv, pose):
    """depth (F,h,w), kinv (3,3) or (F,3,3) float32, pose (F,4,4) float32 -> xyz (F,h,w,3) float32 (float64 math, rounded once),
    mask (F,h,w) bool = z_cam > 0."""
    d = depth_metres(depth).astype(np.float64)
    F, h, w = d.shape
    k = np.broadcast_to(np.asarray(kinv, np.float32), (F, 3, 3)).astype(np.float64).reshape(F, 9, 1, 1)
    p = np.asarray(pose, np.float32).astype(np.float64).reshape(F, 16, 1, 1)
    dv, du = (a.astype(np.float64)[None] for a in np.indices((h, w)))
    with np.errstate(invalid='ignore', over='ignore'):
        rx = (k[:, 0] * du + k[:, 1] * dv) + k[:, 2]
        ry = (k[:, 3] * du + k[:, 4] * dv) + k[:, 5]
        rz = (k[:, 6] * du + k[:, 7] * dv) + k[:, 8]
        xc, yc, zc = rx * d, ry * d, rz * d
        xw = ((xc * p[:, 0] + yc * p[:, 1]) + zc * p[:, 2]) + p[:, 3]
        yw = ((xc * p[:, 4] + yc * p[:, 5]) + zc * p[:, 6]) + p[:, 7]
        zw = ((xc * p[:, 8] + yc * p[:, 9]) + zc * p[:, 10]) + p[:, 11]
        xyz = np.stack([xw, yw, zw], -1).astype(np.float32)
    return xyz, zc > 0


def pixel_keys(xyz, mask, voxel, depth=None, depth_min=None, depth_max=None):
    """xyz (...,3) float32 world points, mask (...) bool (z_cam > 0), depth (...) in any of the stored types when a bound is given
    -> valid (...) bool, key (...) uint64 (all ones where invalid)."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        valid = np.asarray(mask, bool) & (np.isfinite(xyz) & (np.abs(xyz) < 32768)).all(-1)
        if depth_min is not None or depth_max is not None:
            d = depth_metres(depth)
            valid &= (d >= (-np.inf if depth_min is None else np.float32(depth_min))) & (d <= (np.inf if depth_max is None else np.float32(depth_max)))
        i = np.floor(xyz.astype(np.float64) / np.float64(voxel))  # a float64 division
        valid &= ((i >= -INDEX_BIAS) & (i < INDEX_BIAS)).all(-1)
    b = (np.where(valid[..., None], i, 0).astype(np.int64) + INDEX_BIAS).astype(np.uint64)
    key = (b[..., 2] << np.uint64(42)) | (b[..., 1] << np.uint64(21)) | b[..., 0]
    return valid, np.where(valid, key, np.uint64(0xFFFFFFFFFFFFFFFF))


def fuse(xyz, mask, voxel, images=None, depth=None, depth_min=None, depth_max=None, min_samples=1):
    """-> dict: points (n,3) float32, colors (n,3) uint8 or None, count (n,) int32, keys (n,) uint64 ascending, pixel_point int32 of
    mask's shape, n_valid; all_count: the counts of every filled voxel, before min_samples."""
    valid, key = pixel_keys(xyz, mask, voxel, depth, depth_min, depth_max)
    keys, inverse = np.unique(key[valid], return_inverse=True)
    inverse = inverse.reshape(-1)
    count = np.bincount(inverse, minlength=keys.size).astype(np.int64)
    sums = np.zeros((keys.size, 3), np.int64)
    np.add.at(sums, inverse, np.rint(xyz[valid].astype(np.float64) * 65536.0).astype(np.int64))  # rint: to nearest even
    keep = count >= int(min_samples)
    with np.errstate(invalid='ignore', divide='ignore'):
        points = (sums.astype(np.float64) / count[:, None].astype(np.float64) * 2.0 ** -16).astype(np.float32)
    colors = None
    if images is not None:
        images = np.asarray(images)
        assert images.dtype == np.uint8 and images.shape == key.shape + (3,)
        csum = np.zeros((keys.size, 3), np.uint64)
        np.add.at(csum, inverse, images[valid].astype(np.uint64))
        c = count[:, None].astype(np.uint64)
        colors = ((2 * csum + c) // (2 * c)).astype(np.uint8)[keep]
    rank = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    pixel_point = np.full(key.shape, -1, np.int32)
    pixel_point[valid] = rank[inverse]
    return dict(points=points[keep], colors=colors, count=count[keep].astype(np.int32), keys=keys[keep], pixel_point=pixel_point,
                n_valid=int(valid.sum()), all_count=count)

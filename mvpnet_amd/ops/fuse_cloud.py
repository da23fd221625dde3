"""The scene cloud of an RGB-D recording, on the device (new: the reference reads `points` from the vertices of ScanNet's offline mesh,
mvpnet/data/preprocess/preprocess.py:204, which no other recording has): a voxel-grid fusion of the un-projected depth pixels in
INTEGER sums, so the cloud is the same bit for bit whatever the order of frames, `add` calls or lanes, and the map back from any pixel
to its fused point.  Definition, table layout and limits: include/mvp_hip.h, mvp_fuse_cloud_*; kernels: csrc/fuse_cloud.hip."""
import math

import torch

from .. import _lib as L

_INF = float('inf')


def _frames(who, depth, kinv, pose, images=None):
    """The checks every entry shares -> (entry-point suffix, F, h, w, kinv (F,3,3) contiguous)."""
    if not torch.is_tensor(depth) or depth.dim() != 3 or depth.size(1) < 1 or depth.size(2) < 1:
        raise RuntimeError(who + ': depth must be (F,h,w) with h, w >= 1')
    if depth.dtype == torch.float32:
        suffix = 'f32'
    elif depth.dtype in (torch.int16, torch.uint16):
        suffix = 'u16'  # int16 storage is reinterpreted as uint16 millimetres
    else:
        raise RuntimeError(who + ': depth must be float32 (m) or (u)int16 (mm), got {}'.format(depth.dtype))
    F, h, w = depth.shape
    if F * h * w >= 2 ** 31:
        raise RuntimeError(who + ': F * h * w must stay below 2^31 pixels per call (feed a long recording in several add calls)')
    if not torch.is_tensor(kinv) or kinv.dtype != torch.float32 or tuple(kinv.shape) not in ((3, 3), (F, 3, 3)):
        raise RuntimeError(who + ': kinv must be (3,3) or (F,3,3) float32 inverse intrinsics')
    if not torch.is_tensor(pose) or pose.dtype != torch.float32 or tuple(pose.shape) != (F, 4, 4):
        raise RuntimeError(who + ': pose must be (F,4,4) float32 camera-to-world')
    if kinv.device != depth.device or pose.device != depth.device:
        raise RuntimeError(who + ': kinv and pose must be on the depth maps\' device')
    if images is not None:
        if not torch.is_tensor(images) or images.dtype != torch.uint8 or tuple(images.shape) != (F, h, w, 3):
            raise RuntimeError(who + ': images must be (F,h,w,3) uint8 colour frames of the depth maps\' size')
        if images.device != depth.device:
            raise RuntimeError(who + ': images must be on the depth maps\' device')
    if kinv.dim() == 2:
        kinv = kinv.expand(F, 3, 3)
    return suffix, F, h, w, kinv.contiguous()


def kept_slots(keys, keep, n):
    """keys (capacity,) int64 of a table, keep (capacity,) bool with n set entries -> the n kept slots (n,) int64 in ascending key order.
    A dropped or empty slot sorts as -1 -- the empty mark --, in front of every key (keys are below 2^63)."""
    order = torch.sort(torch.where(keep, keys, torch.full((), -1, dtype=torch.int64, device=keys.device))).indices
    return order[keys.numel() - n:].contiguous()


class CloudFuser:
    """fuser = CloudFuser(voxel, max_voxels, device); fuser.add(...) any number of times; points, colors, count = fuser.finish().

    voxel: the grid's edge in metres, a Python float (it enters the kernels as a double).  max_voxels: the number of voxels the caller
    expects at most; the table has capacity = the next power of two >= 2 * max_voxels slots (48 bytes per slot, 72 with colours), and
    only a recording that fills ALL of them overflows.  colors: keep colour sums (add then takes `images`).  depth_min / depth_max:
    metres, a pixel outside [depth_min, depth_max] is ignored (None: no bound).

    A pixel counts when its camera depth is positive, its world point -- ops.unproject's, bit for bit -- is finite with every
    |coordinate| < 32768 and every voxel index floor(x / voxel) lies in [-2^20, 2^20); a frame with a non-finite pose adds nothing."""

    def __init__(self, voxel, max_voxels, device, colors=True, depth_min=None, depth_max=None):
        voxel = float(voxel)
        if not math.isfinite(voxel) or voxel <= 0.0:
            raise ValueError('CloudFuser: voxel must be a finite length > 0, got {}'.format(voxel))
        max_voxels = int(max_voxels)
        if max_voxels < 1:
            raise ValueError('CloudFuser: max_voxels must be at least 1')
        capacity = 1
        while capacity < 2 * max_voxels:
            capacity *= 2
        if capacity >= 2 ** 31:
            raise ValueError('CloudFuser: max_voxels = {} needs a table of {} slots; the limit is 2^30'.format(max_voxels, capacity))
        self.depth_min = -_INF if depth_min is None else float(depth_min)
        self.depth_max = _INF if depth_max is None else float(depth_max)
        if math.isnan(self.depth_min) or math.isnan(self.depth_max):
            raise ValueError('CloudFuser: depth_min / depth_max must not be NaN')
        self.voxel, self.max_voxels, self.capacity, self.colors = voxel, max_voxels, capacity, bool(colors)
        self.device = torch.device(device)
        self.calls_with_images = self.calls_without_images = 0
        self.table = self.rank_of_slot = self.keys = None

    # ---- the table's arrays as views (layout: include/mvp_hip.h) -----------------------------------------------------------------
    def _make_table(self):
        nbytes = L.lib().mvp_fuse_cloud_table_bytes(self.capacity, int(self.colors))
        assert nbytes % 8 == 0 and nbytes > 0
        self.table = torch.zeros(nbytes // 8, dtype=torch.int64, device=self.device)
        self.table[:self.capacity].fill_(-1)  # the empty mark: all ones

    def _count_and_overflow(self):
        tail = self.table[self.capacity * (7 if self.colors else 4):].view(torch.int32)
        return tail[:self.capacity], tail[self.capacity:self.capacity + 1]

    def _check_frames(self, who, depth, kinv, pose, images=None):
        suffix, F, h, w, kinv = _frames(who, depth, kinv, pose, images)
        if depth.device != self.device:
            raise RuntimeError('{}: the frames are on {}, the fuser on {}'.format(who, depth.device, self.device))
        L.require_gpu(depth, kinv, pose, images)
        return suffix, F, h, w, kinv

    def add(self, depth, kinv, pose, images=None):
        """Fuse F more frames: depth (F,h,w) float32 metres or (u)int16 millimetres, kinv (3,3) or (F,3,3) float32 inverse intrinsics of
        that resolution, pose (F,4,4) float32 camera-to-world, images (F,h,w,3) uint8 or None.  One launch, no synchronisation.  Either
        every call gives images or none does (finish raises otherwise)."""
        if images is not None and not self.colors:
            raise RuntimeError('CloudFuser.add: this fuser was made with colors=False and keeps no colour sums')
        suffix, F, h, w, kinv = self._check_frames('CloudFuser.add', depth, kinv, pose, images)
        if self.table is None:
            self._make_table()
        self.rank_of_slot = self.keys = None  # a finished result no longer describes the table
        if images is None:
            self.calls_without_images += 1
        else:
            self.calls_with_images += 1
        L.call('mvp_fuse_cloud_insert_' + suffix, depth, L.ptr(depth), L.ptr(kinv), L.ptr(pose), L.ptr(images), F, h, w, self.voxel,
               self.depth_min, self.depth_max, L.ptr(self.table), self.capacity, int(self.colors))
        return self

    def finish(self, min_samples=1):
        """-> points (n,3) float32, colors (n,3) uint8 (None when no images were added), count (n,) int32: the voxels with at least
        `min_samples` pixels in ascending key order; `self.keys` (n,) int64 holds their keys.  May be called again (another min_samples,
        more frames added since).  One device-to-host read: n and the overflow word, together."""
        if self.calls_with_images and self.calls_without_images:
            raise RuntimeError('CloudFuser.finish: {} add calls gave images and {} did not; a colour mean needs the colour of every pixel'.format(
                self.calls_with_images, self.calls_without_images))
        min_samples = int(min_samples)
        if min_samples < 1:
            raise ValueError('CloudFuser.finish: min_samples must be at least 1')
        if self.table is None:
            raise RuntimeError('CloudFuser.finish: no frames were added')
        cap, dev = self.capacity, self.device
        count, overflow = self._count_and_overflow()
        keep = count >= min_samples
        n, full = torch.stack([keep.sum(), overflow[0].long()]).tolist()  # (the one read)
        if full:
            raise RuntimeError('CloudFuser.finish: the recording has more voxels than the table\'s {} slots and pixels were dropped: '
                               'raise max_voxels (now {})'.format(cap, self.max_voxels))
        slots = kept_slots(self.table[:cap], keep, n)
        with_colors = self.calls_with_images > 0
        points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((n, 3), dtype=torch.uint8, device=dev) if with_colors else None
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        self.rank_of_slot = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        L.call('mvp_fuse_cloud_finish', self.table, L.ptr(self.table), cap, int(self.colors), L.ptr(slots), n, L.ptr(points), L.ptr(colors),
               L.ptr(counts), L.ptr(self.rank_of_slot))
        self.keys = self.table[:cap][slots]
        return points, colors, counts

    def lookup(self, depth, kinv, pose):
        """pixel_point (F,h,w) int32 of ANY frames (the fused ones or others): the row, in the last finish's result, of the voxel the pixel
        falls in; -1 for a pixel that does not count (the rule of `add`, depth bounds included), a voxel no pixel filled, or one that
        min_samples dropped.  One launch, reads only."""
        if self.rank_of_slot is None:
            raise RuntimeError('CloudFuser.lookup: call finish first (and again after adding frames)')
        suffix, F, h, w, kinv = self._check_frames('CloudFuser.lookup', depth, kinv, pose)
        out = torch.empty((F, h, w), dtype=torch.int32, device=self.device)
        L.call('mvp_fuse_cloud_lookup_' + suffix, depth, L.ptr(depth), L.ptr(kinv), L.ptr(pose), F, h, w, self.voxel, self.depth_min, self.depth_max,
               L.ptr(self.table), self.capacity, L.ptr(self.rank_of_slot), L.ptr(out))
        return out


def fuse_cloud(depth, kinv, pose, images=None, *, voxel, max_voxels=None, min_samples=1, depth_min=None, depth_max=None, pixel_point=True):
    """One recording in one go: CloudFuser(voxel, max_voxels, ...).add(depth, kinv, pose, images).finish(min_samples) and the lookup of the
    same frames.  max_voxels: None = the pixel count (a table that cannot overflow).
    -> points (n,3) float32, colors (n,3) uint8 or None, count (n,) int32, pixel_point (F,h,w) int32 (None with pixel_point=False)."""
    _, F, h, w, kinv = _frames('fuse_cloud', depth, kinv, pose, images)
    fuser = CloudFuser(voxel, max(F * h * w, 1) if max_voxels is None else max_voxels, depth.device, colors=images is not None,
                       depth_min=depth_min, depth_max=depth_max)
    points, colors, count = fuser.add(depth, kinv, pose, images).finish(min_samples)
    return points, colors, count, (fuser.lookup(depth, kinv, pose) if pixel_point else None)

"""The whole-scene chunker and the packing of ragged chunks on the device (new: the reference cuts a scene into chunks with NumPy
membership matrices, mvpnet/utils/chunk_util.py:4-53, and pads one chunk at a time in its test loop, mvpnet/test_mvpnet_3d.py:146-154)."""
import numpy as np
import torch

from .. import _lib as L
from .overlap import MAX_BASE_POINTS

MAX_WINDOWS = L.LIMITS['MVP_CHUNKER_MAX_WINDOWS']
MAX_CLOUD_CHANNELS = L.LIMITS['MVP_PACK_CLOUD_MAX_CHANNELS']


def supported(n, nc, nb=0):
    """The shapes mvp_scene_chunks_* take (MVP_EUNSUPPORTED beyond)."""
    return n < 2 ** 31 and nc <= MAX_WINDOWS and nb <= MAX_BASE_POINTS


def _pair(v, name):
    v = tuple(float(x) for x in v)
    if len(v) != 2:
        raise RuntimeError('scene_chunks: {} must be two numbers'.format(name))
    return v


def scene_chunks(points, corners, chunk_size, margin, thresh, base_point_ind=None):
    """The chunks of a scene as index lists in CSR form: two launches and ONE read of 2 * nc counters in between (batch shapes are host
    values).  points (n,3) float32 and corners (nc,2) float32 -- the windows' lower xy corners -- on the device; chunk_size, margin: pairs
    of Python floats; a window is kept when it has at least `thresh` points by the inner test; base_point_ind (nb,) int64 or None.
    -> dict: kept (C,) int64 NumPy array of window ids, lengths: list of C ints, offsets (C+1,) int64 and index (sum of lengths,) int64 on
    the device -- chunk c is index[offsets[c]:offsets[c+1]], ascending --, zbox (C,2) float32 min / max z of the members (+inf / -inf for
    an empty list), base_bits (C,ceil(nb/32)) int32 bit rows or None.  Definition (pinned): include/mvp_hip.h, mvp_scene_chunks_*."""
    L.require_gpu(points, corners, base_point_ind)
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32 or points.size(0) < 1:
        raise RuntimeError('scene_chunks: points must be (n,3) float32, n >= 1')
    if corners.dim() != 2 or corners.size(1) != 2 or corners.dtype != torch.float32 or corners.device != points.device:
        raise RuntimeError('scene_chunks: corners must be (nc,2) float32 on the points\' device')
    nb = 0
    if base_point_ind is not None:
        if base_point_ind.dtype != torch.int64 or base_point_ind.dim() != 1 or base_point_ind.numel() < 1 or base_point_ind.device != points.device:
            raise RuntimeError('scene_chunks: base_point_ind must be (nb,) int64 on the points\' device, nb >= 1')
        nb = base_point_ind.numel()
    (sx, sy), (mx, my) = _pair(chunk_size, 'chunk_size'), _pair(margin, 'margin')
    n, nc, dev = points.size(0), corners.size(0), points.device
    if not supported(n, nc, nb):
        raise RuntimeError('scene_chunks: needs fewer than 2^31 points, at most {} windows and {} base points'.format(MAX_WINDOWS, MAX_BASE_POINTS))
    W = (nb + 31) // 32
    kept, lengths = np.zeros(0, np.int64), []
    if nc:
        counts = torch.empty((2, nc), dtype=torch.int32, device=dev)
        L.call('mvp_scene_chunks_count_f32', points, L.ptr(points), n, L.ptr(corners), nc, sx, sy, mx, my, L.ptr(counts[0]), L.ptr(counts[1]))
        counts = counts.cpu().numpy()  # the read
        kept = np.nonzero(counts[0] >= thresh)[0]
        lengths = counts[1][kept].astype(np.int64)
    C = len(kept)
    host_offsets = np.zeros(C + 1, np.int64)
    np.cumsum(lengths, out=host_offsets[1:])
    total = int(host_offsets[-1])
    out = {'kept': kept, 'lengths': [int(v) for v in lengths],
           'index': torch.empty(total, dtype=torch.int64, device=dev), 'zbox': torch.empty((C, 2), dtype=torch.float32, device=dev),
           'base_bits': torch.empty((C, W), dtype=torch.int32, device=dev) if nb else None}
    # one upload: the offsets, and behind them the window ids as int32 pairs
    table = np.zeros(C + 1 + (C + 1) // 2, np.int64)
    table[:C + 1] = host_offsets
    table[C + 1:].view(np.int32)[:C] = kept
    table = torch.from_numpy(table).to(dev)
    out['offsets'] = table[:C + 1]
    if C:
        L.call('mvp_scene_chunks_fill_f32', points, L.ptr(points), n, L.ptr(corners), nc, sx, sy, mx, my, L.ptr_at(table, C + 1), L.ptr(table), C,
               L.ptr(base_point_ind), nb, L.ptr(out['index']) if total else None, total, L.ptr(out['zbox']), L.ptr(out['base_bits']))
    return out


def pack_chunks(points, index, offsets, lengths, out_base, out_len, seed=0):
    """Every chunk of a scene as padded coordinate rows, one launch.  points (n,3) float32, index (total,) int64 and offsets (C+1,) int64
    on the device (scene_chunks' lists); lengths, out_base, out_len: C host ints each -- chunk c has lengths[c] points and becomes the
    (3, out_len[c]) matrix at float out_base[c] of the result: its points in order, then duplicates of them drawn by the counter hash of
    mvp_sample_chunks_f32's pad rule from `seed`.  -> flat float32 tensor; `out[b:b + B*3*N].view(B,3,N)` is a batch of B chunks of one
    length laid one after the other.  Needs out_len[c] >= lengths[c] >= 1.  Definition (pinned): include/mvp_hip.h, mvp_pack_chunks_f32."""
    L.require_gpu(points, index, offsets)
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32 or points.size(0) < 1:
        raise RuntimeError('pack_chunks: points must be (n,3) float32, n >= 1')
    if index.dtype != torch.int64 or index.dim() != 1 or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise RuntimeError('pack_chunks: index must be (total,) int64 and offsets (C+1,) int64')
    if index.device != points.device or offsets.device != points.device:
        raise RuntimeError('pack_chunks: points, index and offsets must be on one device')
    C = offsets.numel() - 1
    host = np.array([lengths, out_base, out_len], dtype=np.int64).reshape(3, -1)
    if host.shape[1] != C:
        raise RuntimeError('pack_chunks: lengths, out_base and out_len must have one entry per chunk ({})'.format(C))
    if C and (host[0].min() < 1 or (host[2] < host[0]).any() or host[1].min() < 0):
        raise RuntimeError('pack_chunks: needs out_len[c] >= lengths[c] >= 1 and out_base[c] >= 0')
    out_floats = int((host[1] + 3 * host[2]).max()) if C else 0
    out = torch.empty(out_floats, dtype=torch.float32, device=points.device)
    if C == 0:
        return out
    if int(host[0].sum()) > index.numel():
        raise RuntimeError('pack_chunks: the chunks list {} points but index has {}'.format(int(host[0].sum()), index.numel()))
    dev_table = torch.from_numpy(host[1:]).to(points.device)  # (2,C): out_base, out_len
    L.call('mvp_pack_chunks_f32', points, L.ptr(points), points.size(0), L.ptr(index), index.numel(), L.ptr(offsets), C, L.ptr(dev_table[0]),
           L.ptr(dev_table[1]), host[0].ctypes.data, host[2].ctypes.data, int(seed) & (2 ** 64 - 1), L.ptr(out), out_floats)
    return out


def pack_cloud(points, index, offsets, lengths, slot_base, out_len, colors=None, feature=None, seed=0):
    """pack_chunks with a per-point feature beside the coordinates, one launch: what the 3D baselines' sliding-window test feeds PN2SSG.
    points, index, offsets, lengths, out_len, seed: as pack_chunks.  slot_base: C host ints, the chunks' places in SLOTS -- chunk c's
    points are the (3, out_len[c]) matrix at float 3 * slot_base[c] of `points_flat`, its features the (Cf, out_len[c]) matrix at float
    Cf * slot_base[c] of `feature_flat`; chunks of one length in consecutive slots are a (B,3,N) and a (B,Cf,N) batch.
    colors (n,3) uint8 -> colors / 255 (Cf = 3), or feature (n,Cf) float32, 1 <= Cf <= 8, copied; at most one of them.  A padded slot
    repeats one member's point AND feature.  -> (points_flat, feature_flat or None); points_flat holds the bits pack_chunks writes
    with out_base = 3 * slot_base.  Definition (pinned): include/mvp_hip.h, mvp_pack_cloud_f32."""
    L.require_gpu(points, index, offsets, colors, feature)
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32 or points.size(0) < 1:
        raise RuntimeError('pack_cloud: points must be (n,3) float32, n >= 1')
    if index.dtype != torch.int64 or index.dim() != 1 or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise RuntimeError('pack_cloud: index must be (total,) int64 and offsets (C+1,) int64')
    if index.device != points.device or offsets.device != points.device:
        raise RuntimeError('pack_cloud: points, index and offsets must be on one device')
    if colors is not None and feature is not None:
        raise RuntimeError('pack_cloud: colors or feature, not both')
    n, Cf = points.size(0), 0
    if colors is not None:
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (n, 3) or colors.device != points.device:
            raise RuntimeError('pack_cloud: colors must be (n,3) uint8 on the points\' device')
        Cf = 3
    if feature is not None:
        if feature.dtype != torch.float32 or feature.dim() != 2 or feature.size(0) != n or not 1 <= feature.size(1) <= MAX_CLOUD_CHANNELS \
                or feature.device != points.device:
            raise RuntimeError('pack_cloud: feature must be (n,Cf) float32 on the points\' device, 1 <= Cf <= {}'.format(MAX_CLOUD_CHANNELS))
        Cf = feature.size(1)
    C = offsets.numel() - 1
    if not (len(lengths) == len(slot_base) == len(out_len) == C):
        raise RuntimeError('pack_cloud: lengths, slot_base and out_len must have one entry per chunk ({})'.format(C))
    host = np.array([lengths, slot_base, out_len], dtype=np.int64).reshape(3, -1)
    if C and (host[0].min() < 1 or (host[2] < host[0]).any() or host[1].min() < 0):
        raise RuntimeError('pack_cloud: needs out_len[c] >= lengths[c] >= 1 and slot_base[c] >= 0')
    out_slots = int((host[1] + host[2]).max()) if C else 0
    out_points = torch.empty(3 * out_slots, dtype=torch.float32, device=points.device)
    out_feature = torch.empty(Cf * out_slots, dtype=torch.float32, device=points.device) if Cf else None
    if C == 0:
        return out_points, out_feature
    if int(host[0].sum()) > index.numel():
        raise RuntimeError('pack_cloud: the chunks list {} points but index has {}'.format(int(host[0].sum()), index.numel()))
    dev_table = torch.from_numpy(host[1:]).to(points.device)  # (2,C): slot_base, out_len
    L.call('mvp_pack_cloud_f32', points, L.ptr(points), L.ptr(colors), L.ptr(feature), Cf, n, L.ptr(index), index.numel(), L.ptr(offsets), C,
           L.ptr(dev_table[0]), L.ptr(dev_table[1]), host[0].ctypes.data, host[2].ctypes.data, int(seed) & (2 ** 64 - 1), L.ptr(out_points),
           L.ptr(out_feature), out_slots)
    return out_points, out_feature

"""A training batch of chunks drawn on the device (new: the reference draws one chunk per data-loader worker call in NumPy,
mvpnet/data/scannet_2d3d.py:341-381 and :199-204)."""
import torch

from .. import _lib as L

MAX_NB_PTS = L.LIMITS['MVP_SAMPLE_MAX_PTS']  # the crop sorts its (key, index) pairs in LDS
MAX_TRIES = L.LIMITS['MVP_SAMPLE_MAX_TRIES']
MAX_CHUNKS = L.LIMITS['MVP_SAMPLE_MAX_CHUNKS']

_WORKSPACE = {}


def _workspace(entry, device, *shape):
    """The scratch of a call of `entry` (this module's or scene_sample's), one buffer per (entry, size, device): two entry points never
    share one.  Safe for calls issued on ONE stream per device (the launches run in stream order); two streams sampling at the same time
    must call the library with scratch of their own."""
    nbytes = int(getattr(L.lib(), entry + '_workspace')(*shape))
    ws = _WORKSPACE.get((entry, nbytes, device))
    if ws is None:
        ws = _WORKSPACE[(entry, nbytes, device)] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return ws, nbytes


def _i64(t, name, who='sample_chunks'):
    if not torch.is_tensor(t) or t.dtype != torch.int64:
        raise RuntimeError('{}: {} must be an int64 tensor'.format(who, name))
    return t


def _seed(seed, who):
    """-> (the 64 bits of an int seed, the device's seed tensor or None)"""
    if not torch.is_tensor(seed):
        return int(seed) & (2 ** 64 - 1), None
    if not seed.is_cuda or seed.dtype != torch.int64 or seed.numel() != 1:
        raise RuntimeError(who + ': a tensor seed must be one int64 on the device')
    return 0, seed


def sample_chunks(points, seg_label, scene_offsets, scene_of_chunk, center_ind, nb_pts, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2),
                  chunk_thresh=0.3, seed=0, base_point_ind=None, bounds_f64=False):
    """B training chunks in one call, no host synchronisation (`ScanNet2D3DChunks.__getitem__`'s chunk choice and resampling).
    points (Ntot,3) float32 and seg_label (Ntot,) int64: S scenes one after the other (labels mapped, negative = unlabelled);
    scene_offsets (S+1,) int64; scene_of_chunk (B,) int64; center_ind (B,T) int64: the centres to try, indices inside the chunk's scene
    (their range is the caller's: nothing here reads a tensor back); base_point_ind (S,nbp) int64 or None; seed: an int, or an int64
    tensor of one element on the device (a captured graph then draws afresh on every replay).  bounds_f64: ScanNet3DChunks' float64 box.
    -> dict: choice (B,nb_pts) int64 inside the scene, points (B,3,nb_pts) float32, seg_label (B,nb_pts) int64, chunk_box (B,4) float32,
    try_index (B,) int32 (-1: the whole-scene fallback), num_members (B,) int32 [, base_bits (B,ceil(nbp/32)) int32 bit rows].
    Definition (pinned): include/mvp_hip.h, mvp_sample_chunks_f32."""
    L.require_gpu(points, seg_label, scene_offsets, scene_of_chunk, center_ind, base_point_ind)
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32 or points.size(0) < 1:
        raise RuntimeError('sample_chunks: points must be (Ntot,3) float32, Ntot >= 1')
    Ntot = points.size(0)
    if _i64(seg_label, 'seg_label').shape != (Ntot,):
        raise RuntimeError('sample_chunks: seg_label must be (Ntot,)')
    if _i64(scene_offsets, 'scene_offsets').dim() != 1 or scene_offsets.numel() < 2:
        raise RuntimeError('sample_chunks: scene_offsets must be (S+1,), S >= 1')
    S = scene_offsets.numel() - 1
    if _i64(scene_of_chunk, 'scene_of_chunk').dim() != 1:
        raise RuntimeError('sample_chunks: scene_of_chunk must be (B,)')
    B = scene_of_chunk.numel()
    if _i64(center_ind, 'center_ind').dim() != 2 or center_ind.size(0) != B or center_ind.size(1) < 1:
        raise RuntimeError('sample_chunks: center_ind must be (B,T), T >= 1')
    T = center_ind.size(1)
    nb_pts = int(nb_pts)
    if not (1 <= nb_pts <= MAX_NB_PTS and T <= MAX_TRIES and B <= MAX_CHUNKS and Ntot < 2 ** 31):
        raise RuntimeError('sample_chunks: needs 1 <= nb_pts <= {}, T <= {}, B <= {} and fewer than 2^31 points'.format(MAX_NB_PTS, MAX_TRIES, MAX_CHUNKS))
    nbp = 0
    if base_point_ind is not None:
        if _i64(base_point_ind, 'base_point_ind').dim() != 2 or base_point_ind.size(0) != S or base_point_ind.size(1) < 1:
            raise RuntimeError('sample_chunks: base_point_ind must be (S,nbp), nbp >= 1')
        nbp = base_point_ind.size(1)
    sx, sy = (float(v) for v in chunk_size)
    mx, my = (float(v) for v in chunk_margin)
    seed, seed_dev = _seed(seed, 'sample_chunks')
    dev = points.device
    out = {'choice': torch.empty((B, nb_pts), dtype=torch.int64, device=dev),
           'points': torch.empty((B, 3, nb_pts), dtype=torch.float32, device=dev),
           'seg_label': torch.empty((B, nb_pts), dtype=torch.int64, device=dev),
           'chunk_box': torch.empty((B, 4), dtype=torch.float32, device=dev),
           'try_index': torch.empty((B,), dtype=torch.int32, device=dev),
           'num_members': torch.empty((B,), dtype=torch.int32, device=dev)}
    if nbp:
        out['base_bits'] = torch.empty((B, (nbp + 31) // 32), dtype=torch.int32, device=dev)
    if B == 0:
        return out
    ws, nbytes = _workspace('mvp_sample_chunks', dev, Ntot, B, T, nb_pts)
    L.call('mvp_sample_chunks_f32', points, L.ptr(points), L.ptr(seg_label), L.ptr(scene_offsets), L.ptr(scene_of_chunk), L.ptr(center_ind),
           L.ptr(base_point_ind), Ntot, S, B, T, nbp, nb_pts, sx, sy, mx, my, float(chunk_thresh), int(bool(bounds_f64)),
           seed, L.ptr(seed_dev), L.ptr(out['choice']), L.ptr(out['points']), L.ptr(out['seg_label']),
           L.ptr(out['chunk_box']), L.ptr(out['try_index']), L.ptr(out['num_members']), L.ptr(out.get('base_bits')), L.ptr(ws), nbytes)
    return out

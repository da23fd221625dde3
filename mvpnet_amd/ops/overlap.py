"""Frame selection inputs on the device (new: the reference computes `pointwise_rgbd_overlap` offline with an open3d KD-tree,
mvpnet/data/preprocess/preprocess.py:99-170, and selects frames per chunk in a NumPy loop, mvpnet/data/scannet_2d3d.py:20-30).

Bit rows: a bool matrix with `nb` columns is packed 32 columns per word, column j = bit j % 32 of word j // 32, W = ceil(nb / 32)
words per row.  torch has no arithmetic on uint32, so the words are carried in int32 tensors (the bit pattern is what counts)."""
import torch

from .. import _lib as L

MAX_BASE_POINTS = L.LIMITS['MVP_OVERLAP_MAX_BASE']  # the base points of mvp_frame_overlap_* live in LDS
MAX_SELECT_WORDS = 1024  # mvp_select_frames_u32 keeps the uncovered set in LDS


def pack_bits(mask):
    """bool (R, nb) -> int32 (R, ceil(nb / 32)) bit rows, on mask's device: nothing comes back to the host; the only host
    traffic is the 8-byte weight constant going up."""
    if mask.dim() != 2 or mask.dtype != torch.bool:
        raise RuntimeError('pack_bits: expected a 2-D bool tensor')
    R, nb = mask.shape
    W = (nb + 31) // 32
    m = torch.zeros((R, W * 32), dtype=torch.uint8, device=mask.device)
    m[:, :nb] = mask
    weight = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=mask.device)  # (an 8-byte host-to-device copy)
    by = (m.view(R, W * 4, 8) * weight).sum(-1, dtype=torch.uint8)  # little-endian bytes of the words
    return by.contiguous().view(torch.int32)


def unpack_bits(bits, nb):
    """int32 (R, W) bit rows -> bool (R, nb), on bits' device."""
    if bits.dim() != 2 or bits.dtype != torch.int32 or bits.size(1) * 32 < nb:
        raise RuntimeError('unpack_bits: expected int32 (R, W) bit rows with W * 32 >= nb')
    by = bits.contiguous().view(torch.uint8)  # (R, W*4)
    shift = torch.arange(8, dtype=torch.uint8, device=bits.device)
    m = (by.unsqueeze(-1) >> shift) & 1
    return m.view(bits.size(0), bits.size(1) * 32)[:, :nb].bool()


def rgbd_overlap(depth, kinv, pose, base_points, radius=0.1, packed=False):
    """Which base points does every frame see (compute_rgbd_knn's inner loop, preprocess.py:129-158)?
    depth (F,h,w) float32 metres or (u)int16 millimetres, kinv (F,3,3) float32 inverse intrinsics of THAT resolution, pose (F,4,4)
    float32 camera-to-world, base_points (nb,3) float32, nb <= 4096.
    -> bool (nb,F) in the layout of the reference's `pointwise_rgbd_overlap`, or with packed=True the int32 (F, ceil(nb/32)) bit rows
    mvp_select_frames_u32 reads.  Definition (pinned, include/mvp_hip.h): a pixel with z_cam > 0 marks its nearest base point
    (float32 (dx*dx + dy*dy) + dz*dz, lowest index on ties) iff d2 < fl32(radius * radius); frames with a non-finite pose see nothing."""
    L.require_gpu(depth, kinv, pose, base_points)
    if depth.dim() != 3:
        raise RuntimeError('rgbd_overlap: depth must be (F,h,w)')
    F, h, w = depth.shape
    if kinv.shape != (F, 3, 3) or pose.shape != (F, 4, 4) or kinv.dtype != torch.float32 or pose.dtype != torch.float32:
        raise RuntimeError('rgbd_overlap: kinv must be (F,3,3) float32 and pose (F,4,4) float32')
    if base_points.dim() != 2 or base_points.size(1) != 3 or base_points.dtype != torch.float32 or base_points.size(0) < 1:
        raise RuntimeError('rgbd_overlap: base_points must be (nb,3) float32, nb >= 1')
    if depth.dtype == torch.float32:
        name = 'mvp_frame_overlap_f32'
    elif depth.dtype in (torch.int16, torch.uint16):
        name = 'mvp_frame_overlap_u16'  # int16 storage is reinterpreted as uint16 millimetres
    else:
        raise RuntimeError('rgbd_overlap: depth must be float32 (m) or (u)int16 (mm)')
    nb = base_points.size(0)
    bits = torch.empty((F, (nb + 31) // 32), dtype=torch.int32, device=depth.device)
    L.call(name, depth, L.ptr(depth), L.ptr(kinv), L.ptr(pose), L.ptr(base_points), F, h, w, nb, float(radius), L.ptr(bits))
    if packed:
        return bits
    return unpack_bits(bits, nb).t().contiguous()


def select_frames_batched(overlap, chunk_base_mask, num_rgbd_frames, return_gain=False, frame_begin=None, frame_count=None):
    """`select_frames` (scannet_2d3d.py:20-30) for all chunks of a scene in one launch; with bit rows as input there is no host
    synchronisation, bool input is packed first (pack_bits: one 8-byte constant copied to the device per matrix).
    overlap: bool (nb,F) (the reference's layout) or int32 (F,W) bit rows; chunk_base_mask: bool (C,nb) -- base point j lies in
    chunk c -- or int32 (C,W) bit rows.  -> picked (C,n) int64 [, gain (C,n) int32: newly covered base points per pick]; row c equals
    select_frames(overlap[chunk_base_mask[c]], n).
    frame_begin, frame_count (C,) int64 (both or neither): the chunks of a TRAINING batch, every chunk with the frames of its own
    scene -- overlap then holds all scenes' frames one scene after the other, chunk c chooses among frames [begin, begin + count) only
    and gets GLOBAL frame indices (mvp_select_frames_ranges_u32).  Device tensors are taken as they are (no synchronisation; count >= 1
    and the range are then the caller's, a chunk without frames gets -1); host tensors or sequences are checked here first."""
    L.require_gpu(overlap, chunk_base_mask)
    if overlap.dim() != 2 or chunk_base_mask.dim() != 2:
        raise RuntimeError('select_frames_batched: overlap and chunk_base_mask must be 2-D')
    ov = pack_bits(overlap.t()) if overlap.dtype == torch.bool else overlap
    cb = pack_bits(chunk_base_mask) if chunk_base_mask.dtype == torch.bool else chunk_base_mask
    if ov.dtype != torch.int32 or cb.dtype != torch.int32:
        raise RuntimeError('select_frames_batched: expected bool matrices or int32 bit rows')
    if overlap.dtype == torch.bool and chunk_base_mask.dtype == torch.bool and overlap.size(0) != chunk_base_mask.size(1):
        raise RuntimeError('select_frames_batched: overlap (nb,F) and chunk_base_mask (C,nb) disagree on nb')
    if ov.size(1) != cb.size(1):
        raise RuntimeError('select_frames_batched: overlap and chunk_base_mask have different numbers of words per row')
    ov, cb = ov.contiguous(), cb.contiguous()
    F, W = ov.shape
    C = cb.size(0)
    n = int(num_rgbd_frames)
    if F < 1 or n < 0:
        raise RuntimeError('select_frames_batched: needs at least one frame and num_rgbd_frames >= 0')
    picked = torch.empty((C, n), dtype=torch.int64, device=ov.device)
    gain = torch.empty((C, n), dtype=torch.int32, device=ov.device) if return_gain else None
    if (frame_begin is None) != (frame_count is None):
        raise RuntimeError('select_frames_batched: frame_begin and frame_count go together')
    if frame_begin is not None:
        rng = []
        for r in (frame_begin, frame_count):
            r = torch.as_tensor(r)
            if r.dtype != torch.int64 or r.shape != (C,):
                raise RuntimeError('select_frames_batched: frame_begin and frame_count must be (C,) int64')
            rng.append(r)
        if not rng[0].is_cuda and not rng[1].is_cuda and C:  # host-known ranges: refused before anything is launched
            if int(rng[1].min()) < 1 or int(rng[0].min()) < 0 or int((rng[0] + rng[1]).max()) > F:
                raise RuntimeError('select_frames_batched: every chunk needs frame_count >= 1 and a range inside [0, {})'.format(F))
        fb, fc = (r.to(ov.device).contiguous() for r in rng)
        L.call('mvp_select_frames_ranges_u32', ov, L.ptr(ov), L.ptr(cb), L.ptr(fb), L.ptr(fc), F, C, W, n, L.ptr(picked), L.ptr(gain))
        return (picked, gain) if return_gain else picked
    L.call('mvp_select_frames_u32', ov, L.ptr(ov), L.ptr(cb), F, C, W, n, L.ptr(picked), L.ptr(gain))
    return (picked, gain) if return_gain else picked

"""Device-side chunker and frame selection: what runs right BEFORE the hot path in the reference's
CPU data loader -- `scene2chunks_legacy` (mvpnet/utils/chunk_util.py:4-53), `select_frames` (mvpnet/data/scannet_2d3d.py:20-30)
and the crop / pad resampling to a fixed point count (scannet_2d3d.py:374-381).  Same names, arguments and results; tensors
stay on the GPU (one tiny host round trip for the scene bounding box, one for the variable-length index lists).

Arithmetic note: the reference mixes float32 points with Python floats; the goldens were produced by running the reference under
NumPy 2 (NEP 50: `np.float32 + python float` stays float32), and this file reproduces exactly that: corners in float32, the upper
bounds and the margins in float64."""
import numpy as np
import torch


def _window_corners(points, chunk_size, stride):
    """(nc,2) float32 lower xy corners of the sliding windows, on the host (chunk_util.py:20-30)."""
    ext = torch.stack([points.min(0).values, points.max(0).values]).cpu().numpy()  # (2,3) float32, the one scalar round trip
    coord_min, coord_max = ext[0], ext[1]
    limit = coord_max - coord_min
    num_chunks = np.ceil((limit[:2] - chunk_size) / stride).astype(int) + 1
    return np.array([(coord_min[0] + np.float32(i * stride), coord_min[1] + np.float32(j * stride))
                     for i in range(num_chunks[0]) for j in range(num_chunks[1])], np.float32).reshape(-1, 2)


def scene2chunks_legacy(points, chunk_size, stride, thresh=1000, margin=(0.2, 0.2), return_bbox=False):
    """points (n,3) float32 tensor (any device) -> list of int64 index tensors [, list of (6,) float64 bboxes x1,y1,z1,x2,y2,z2]."""
    assert points.dim() == 2 and points.size(1) == 3 and points.dtype == torch.float32
    dev = points.device
    chunk_size = np.asarray(chunk_size, np.float64)
    margin_np = np.asarray(margin, np.float64)
    corners = _window_corners(points, chunk_size, stride)
    if corners.shape[0] == 0:
        return ([], []) if return_bbox else []
    lo = torch.from_numpy(corners).to(dev)                                       # (nc,2) float32
    hi = lo.double() + torch.from_numpy(chunk_size).to(dev)                      # float64 like `corner + chunk_size`
    mg = torch.from_numpy(margin_np).to(dev)
    xy = points[:, :2]
    xyd = xy.double()
    inner = ((xy[None] >= lo[:, None]) & (xyd[None] <= hi[:, None])).all(-1)     # (nc,n)
    keep = inner.sum(1) >= thresh
    outer = ((xyd[None] >= (lo.double() - mg)[:, None]) & (xyd[None] <= (hi + mg)[:, None])).all(-1)
    outer = outer[keep]
    counts = outer.sum(1).tolist()                                               # the second (and last) host round trip
    flat = outer.nonzero()[:, 1]
    chunk_indices = list(torch.split(flat, counts))
    if not return_bbox:
        return chunk_indices
    z = points[:, 2]
    big = torch.tensor(float('inf'), device=dev)
    zmin = torch.where(outer, z[None], big).amin(1).double()
    zmax = torch.where(outer, z[None], -big).amax(1).double()
    lo_k, hi_k = lo.double()[keep] - mg, hi[keep] + mg
    boxes = torch.cat([lo_k, zmin[:, None], hi_k, zmax[:, None]], dim=1)
    return chunk_indices, list(boxes)


def scene2chunks_csr(points, chunk_size, stride, thresh=1000, margin=(0.2, 0.2), base_point_ind=None):
    """scene2chunks_legacy's chunks as ONE flat index list: no (windows x points) matrices, no per-chunk tensors, and with
    `base_point_ind` ((nb,) int64) the chunks' base-point bit rows for ops.select_frames_batched.  Two host round trips: the scene's
    extent, and the windows' point counts (ops.scene_chunks).
    -> dict: offsets (C+1,) int64 and index (total,) int64 on the points' device -- chunk c is index[offsets[c]:offsets[c+1]], ascending
    --, lengths: list of C ints, boxes (C,6) float64 x1,y1,z1,x2,y2,z2 as `scene2chunks_legacy(..., return_bbox=True)`, base_bits
    (C,ceil(nb/32)) int32 or None.  Same lists, bit for bit, as scene2chunks_legacy -- which is also what builds the dict for a CPU tensor
    and for a scene beyond the kernel's limits (2^31 points, 65535 windows, 4096 base points)."""
    from . import ops
    assert points.dim() == 2 and points.size(1) == 3 and points.dtype == torch.float32
    dev = points.device
    nb = 0 if base_point_ind is None else int(base_point_ind.numel())
    size_np, margin_np = np.asarray(chunk_size, np.float64), np.asarray(margin, np.float64)
    corners = _window_corners(points, size_np, stride)
    if not (points.is_cuda and ops.chunker.supported(points.size(0), corners.shape[0], nb)):
        idx, boxes = scene2chunks_legacy(points, chunk_size, stride, thresh=thresh, margin=margin, return_bbox=True)
        lengths = [int(i.numel()) for i in idx]
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
        bits = ops.pack_bits(chunk_base_masks(idx, base_point_ind.to(dev), points.size(0))) if nb else None
        return {'offsets': offsets, 'index': torch.cat(idx) if idx else torch.zeros(0, dtype=torch.int64, device=dev), 'lengths': lengths,
                'boxes': torch.stack(boxes) if boxes else torch.zeros((0, 6), dtype=torch.float64, device=dev), 'base_bits': bits}
    lo = torch.from_numpy(corners).to(dev)
    ch = ops.scene_chunks(points, lo, size_np, margin_np, thresh, base_point_ind=base_point_ind)
    lo_k = lo.double()[torch.from_numpy(ch['kept']).to(dev)]  # the arithmetic of scene2chunks_legacy's boxes, for the kept windows only
    mg = torch.from_numpy(margin_np).to(dev)
    z = ch['zbox'].double()
    boxes = torch.cat([lo_k - mg, z[:, :1], (lo_k + torch.from_numpy(size_np).to(dev)) + mg, z[:, 1:]], dim=1)
    return {'offsets': ch['offsets'], 'index': ch['index'], 'lengths': ch['lengths'], 'boxes': boxes, 'base_bits': ch['base_bits']}


def select_frames(rgbd_overlap, num_rgbd_frames):
    """rgbd_overlap (n_base_points, n_frames) bool tensor: greedy set cover, the frame seeing most still-uncovered base points
    first (lowest frame index on ties, like numpy.argmax).  Returns a list of ints."""
    ov = rgbd_overlap.clone()
    picked = []
    for _ in range(num_rgbd_frames):
        score = ov.sum(0)
        idx = int((score == score.max()).nonzero()[0])
        picked.append(idx)
        ov[ov[:, idx].clone()] = False  # (the mask must not alias the tensor being written)
    return picked


def chunk_base_masks(chunk_indices, base_point_ind, n_pts):
    """bool (C, nb): base point j lies in chunk c (`base_point_mask[base_point_ind]` of scannet_2d3d.py:199-204, for all chunks).
    Goes through a (C, n_pts) bool membership matrix: 12.8 MB for 64 chunks of a 200 000-point scene, C * n_pts bytes in general."""
    dev = base_point_ind.device
    C = len(chunk_indices)
    member = torch.zeros((C, n_pts), dtype=torch.bool, device=dev)
    if C:
        rows = torch.repeat_interleave(torch.arange(C, device=dev), torch.tensor([int(c.numel()) for c in chunk_indices], device=dev))
        member[rows, torch.cat(chunk_indices)] = True
    return member[:, base_point_ind]


def crop_pad_choice(n, nb_pts, generator=None, device=None):
    """Indices that resample n points to exactly nb_pts: all points + random repeats when n < nb_pts, a random subset without
    replacement otherwise (scannet_2d3d.py:374-381; the reference draws from numpy's global RNG, so only the law matches)."""
    if n < nb_pts:
        pad = torch.randint(n, (nb_pts - n,), generator=generator, device=device)
        return torch.cat([torch.arange(n, device=device), pad])
    return torch.randperm(n, generator=generator, device=device)[:nb_pts]


def sample_train_chunks(points, seg_label, scene_offsets, scene_of_chunk, nb_pts, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2),
                        chunk_thresh=0.3, num_tries=10, base_point_ind=None, bounds_f64=False, generator=None):
    """A training batch of chunks drawn on the device: `ScanNet2D3DChunks.__getitem__`'s random chunk and resampling
    (scannet_2d3d.py:341-381) for B dataset indices at once, without a host synchronisation.  points (Ntot,3) float32 / seg_label (Ntot,)
    int64: the resident scenes one after the other, scene_offsets (S+1,) int64, scene_of_chunk (B,) int64, all on the device.
    The `num_tries` centres of every chunk (`np.random.randint(n)` per try in the reference) and the resampling seed are drawn ON THE
    DEVICE from `generator` (a generator of that device, or its global one): the same law as the reference, not the same draws.
    -> ops.sample_chunks' dict (choice, points (B,3,nb_pts), seg_label, chunk_box, try_index, num_members [, base_bits]) + the draws:
    center_ind (B,num_tries) int64 and seed (1,) int64, on the device."""
    from . import ops
    dev = points.device
    n = (scene_offsets[1:] - scene_offsets[:-1])[scene_of_chunk]                              # (B,)
    u = torch.rand((scene_of_chunk.numel(), int(num_tries)), dtype=torch.float64, generator=generator, device=dev)
    center_ind = torch.minimum((u * n[:, None]).long(), (n - 1).clamp_(min=0)[:, None]).contiguous()  # uniform on [0, n)
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=generator, device=dev)
    out = ops.sample_chunks(points, seg_label, scene_offsets, scene_of_chunk, center_ind, nb_pts, chunk_size=chunk_size,
                            chunk_margin=chunk_margin, chunk_thresh=chunk_thresh, seed=seed, base_point_ind=base_point_ind,
                            bounds_f64=bounds_f64)
    out['center_ind'], out['seed'] = center_ind, seed
    return out


def sample_train_scenes(scene_offsets, scene_of_row, nb_pts, Ntot=None, generator=None):
    """`CropPad(nb_pts)` of B whole scenes drawn on the device: what `ScanNet3DScene.__getitem__` does with the transform of
    configs/scannet/3d_baselines/pn2ssg_scene.yaml (mvpnet/data/scannet_3d.py:206-221, mvpnet/data/transforms.py:112-133) for B dataset
    indices at once, without a host synchronisation -- sample_train_chunks' sibling, where crop_pad_choice needs every n on the host.
    scene_offsets (S+1,) int64 and scene_of_row (B,) int64 on the device; Ntot: the store's point count (ops.sample_scenes).  The
    resampling seed is drawn ON THE DEVICE from `generator` (a generator of that device, or its global one): the reference's law, not
    its draws.  -> ops.sample_scenes' dict (choice (B,nb_pts) int64, num_points (B,) int32) + seed (1,) int64 on the device."""
    from . import ops
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=generator, device=scene_offsets.device)
    out = ops.sample_scenes(scene_offsets, scene_of_row, nb_pts, seed=seed, Ntot=Ntot)
    out['seed'] = seed
    return out


def _kinv_of(cam_matrix):
    """inverse of the 3x3 intrinsics in float32 on the host, as the loader does it (np.linalg.inv(cam_matrix[:3, :3]), scannet_2d3d.py:38)."""
    cam = cam_matrix.detach().cpu().numpy() if torch.is_tensor(cam_matrix) else np.asarray(cam_matrix)
    return np.linalg.inv(cam.astype(np.float32)[..., :3, :3])


def compute_rgbd_overlap(points, depth, cam_matrix, pose, num_base_pts=2000, radius=0.1, generator=None, packed=False):
    """`compute_rgbd_knn` (mvpnet/data/preprocess/preprocess.py:99-170) on the device: the two arrays the reference stores per scene.
    points (n,3) float32 device tensor (the whole scene), depth (F,h,w) float32 metres or (u)int16 millimetres, cam_matrix (3,3) or
    (4,4) intrinsics OF THE DEPTH MAPS' RESOLUTION (array or tensor; (F,3,3) for per-frame intrinsics), pose (F,4,4) float32.
    -> base_point_ind (num_base_pts,) int64, overlaps (num_base_pts, F) bool  (`base_point_ind`, `pointwise_rgbd_overlap`); with
    packed=True the overlaps stay the kernel's int32 (F, ceil(num_base_pts/32)) bit rows, as ops.select_frames_batched reads them.

    Base points are `randperm(n)[:num_base_pts]` from `generator` (or torch's global generator of the device): the same LAW as the
    reference's `np.random.choice(n, num_base_pts, replace=False)`, not the same draws.
    The reference works on 80x60 maps made from the 640x480 depth PNGs by PIL's NEAREST resize, which for a factor of 8 samples the
    centre of every 8x8 block, and divides the first two rows of the intrinsics by 8 (preprocess.py:120-126, :143-145); a caller
    holding full-size maps gets the same input with `depth[:, 4::8, 4::8]` and `cam_matrix[0] /= 8; cam_matrix[1] /= 8`.
    The nearest-neighbour rule is pinned in include/mvp_hip.h (float32, strict `<`); ops.rgbd_overlap is the kernel's wrapper."""
    from . import ops
    assert points.dim() == 2 and points.size(1) == 3 and points.dtype == torch.float32
    n = points.size(0)
    if num_base_pts > n:
        raise ValueError('cannot take {} base points from a scene of {} points'.format(num_base_pts, n))
    F = depth.size(0)
    base_point_ind = torch.randperm(n, generator=generator, device=points.device if generator is None else generator.device)
    base_point_ind = base_point_ind[:num_base_pts].to(points.device)
    kinv = torch.from_numpy(np.ascontiguousarray(_kinv_of(cam_matrix))).to(points.device)
    if kinv.dim() == 2:
        kinv = kinv.expand(F, 3, 3)
    overlaps = ops.rgbd_overlap(depth.contiguous(), kinv.contiguous(), pose.contiguous(), points[base_point_ind].contiguous(), radius=radius,
                                packed=packed)
    return base_point_ind, overlaps

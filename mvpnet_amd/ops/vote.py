"""Whole-scene voting on the device (new: the reference propagates every vote's logits to the scene through a scikit-learn ball tree on
the host, one fit + query per vote, mvpnet/test_3d_scene.py:152-164; its whole-scene test of the 2D baseline gathers, averages and
accumulates chunk by chunk, mvpnet/test_2d_chunks.py:137-147 with mvpnet/models/mvpnet_2d.py:22-34)."""
import torch

from .. import _lib as L

MAX_KEYS = 65536    # mvp_vote_nearest_f32: keys per vote
MAX_CLASSES = 64    # logit columns the kernel keeps in registers (mvp_lift_vote_f32: logit columns)
MAX_K = 8           # mvp_lift_vote_f32: neighbours per point

_WORKSPACE = {}


def _workspace(V, nb, device):
    """The grids' scratch, one buffer per (V, nb, device).  Safe for calls issued on ONE stream per device (the launches that use it run in
    stream order, the next call's build waits for this call's query); two streams voting the same shape at the same time would share it
    and must call mvp_vote_nearest_f32 with scratch of their own."""
    nbytes = int(L.lib().mvp_vote_nearest_workspace(V, nb))
    if nbytes == 0:
        return None, 0
    key = (V, nb, device)
    ws = _WORKSPACE.get(key)
    if ws is None:
        ws = _WORKSPACE[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws, nbytes


def vote_nearest(points, keys, logits, return_index=False, swept=None):
    """Every scene point takes, from each of V votes, the logits of that vote's nearest sampled point, added in vote order
    (`pred_logit_whole_scene += seg_logit_per_vote[nn_indices[:, 0]]`, test_3d_scene.py:155-161).
    points (n,3) float32; keys (V,nb,3) float32: the sampled points of each vote; logits (V,C,nb) float32 in ANY strides (the network's
    transposed view of row-major rows is read in place, nothing is copied).  swept: None, or an int32 tensor of one element that the
    caller zeroed: += the number of (point, vote) searches that swept all keys (a test's view of the search path).
    -> sum (n,C) float32 [, nn_index (V,n) int64].  Definition (pinned, include/mvp_hip.h): nearest by float32 (dx*dx + dy*dy) + dz*dz,
    lowest key index on ties; sum = (...(logit_0 + logit_1) + ...), bit-reproducible.  Mean and labels: mvp_vote_finish_f32 with count V."""
    L.require_gpu(points, keys)
    if not logits.is_cuda:
        raise RuntimeError('mvpnet_amd ops run on the GPU only (got a {} tensor); there is no CPU fallback'.format(logits.device))
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32:
        raise RuntimeError('vote_nearest: points must be (n,3) float32')
    if keys.dim() != 3 or keys.size(2) != 3 or keys.dtype != torch.float32:
        raise RuntimeError('vote_nearest: keys must be (V,nb,3) float32')
    V, nb, _ = keys.shape
    if logits.dim() != 3 or logits.size(0) != V or logits.size(2) != nb or logits.dtype != torch.float32:
        raise RuntimeError('vote_nearest: logits must be (V,C,nb) float32 with the V and nb of keys')
    C = logits.size(1)
    if not (1 <= V < 65536 and 1 <= nb <= MAX_KEYS and 1 <= C <= MAX_CLASSES):
        raise RuntimeError('vote_nearest: needs 1 <= V < 65536, 1 <= nb <= {} and 1 <= C <= {}'.format(MAX_KEYS, MAX_CLASSES))
    if swept is not None and (not swept.is_cuda or swept.dtype != torch.int32 or swept.numel() != 1):
        raise RuntimeError('vote_nearest: swept must be one int32 on the device')
    n = points.size(0)
    total = torch.empty((n, C), dtype=torch.float32, device=points.device)
    index = torch.empty((V, n), dtype=torch.int64, device=points.device) if return_index else None
    ws, nbytes = _workspace(V, nb, points.device)
    L.call('mvp_vote_nearest_f32', points, L.ptr(points), n, L.ptr(keys), V, nb, L.ptr(logits), logits.stride(0), logits.stride(2),
           logits.stride(1), C, L.ptr(total), L.ptr(index), L.ptr(swept), L.ptr(ws), nbytes)
    return (total, index) if return_index else total


def lift_vote(logit, view_frame, knn, knn_base, chunk_inds, n_pts, plan=None):
    """The class logits of a frame store lifted to every chunk's points through the pixel k-NN, averaged over k and added into the scene
    in chunk order (`pred_logit_whole_scene[chunk_ind] += seg_logit`, test_2d_chunks.py:146), without the gathered rows or the per-chunk
    means in memory.
    logit (U,C,h,w) float32 in ANY strides: the 2D network's output for U distinct frames where it lies -- NCHW, or channels-last memory
        (rows of C floats, read with 16-byte loads when C % 4 == 0); the strides are taken from the tensor, nothing is copied.
    view_frame (num_chunks,nv) int32 / int64: the store frame of each chunk's view.
    knn (R,k) int64: rows of chunk-local flat pixel ids view*h*w + q (ops.pixel_knn's), < 0 = missing; knn_base: num_chunks host ints,
        the row of each chunk's first point -- chunk i reads rows knn_base[i] .. knn_base[i] + len(chunk_inds[i]) and no others.
    chunk_inds: the chunks' scene point ids, int64 tensors on the device (dist._vote_plan builds and keeps their transposed index), or
        plan: such a plan, instead.
    -> sum (n_pts,C) float32, count (n_pts,) int32; mean and labels: mvp_vote_finish_f32.  Definition (pinned): include/mvp_hip.h,
    mvp_lift_vote_f32; bit-reproducible."""
    from .. import dist as D
    for name, t in (('logit', logit), ('view_frame', view_frame), ('knn', knn)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError('mvpnet_amd ops run on the GPU only (lift_vote: {} is not a device tensor); there is no CPU fallback'.format(name))
    if logit.dim() != 4 or logit.dtype != torch.float32:
        raise RuntimeError('lift_vote: logit must be (U,C,h,w) float32')
    U, C, h, w = logit.shape
    hw = h * w
    if not (U >= 1 and hw >= 1 and 1 <= C <= MAX_CLASSES):
        raise RuntimeError('lift_vote: needs U, h*w >= 1 and 1 <= C <= {}'.format(MAX_CLASSES))
    if h > 1 and w > 1 and logit.stride(2) != w * logit.stride(3):
        raise RuntimeError('lift_vote: the pixels of a frame must lie at one stride (NCHW or channels-last memory)')
    ld_p = logit.stride(3) if w > 1 else (logit.stride(2) if h > 1 else 1)
    if knn.dim() != 2 or knn.dtype != torch.int64 or not knn.is_contiguous() or not 1 <= knn.size(1) <= MAX_K:
        raise RuntimeError('lift_vote: knn must be contiguous (R,k) int64 with 1 <= k <= {}'.format(MAX_K))
    num_chunks = len(knn_base)
    if view_frame.dim() != 2 or view_frame.size(0) != num_chunks or num_chunks < 1 or view_frame.size(1) < 1 or view_frame.dtype not in (torch.int32, torch.int64):
        raise RuntimeError('lift_vote: view_frame must be (num_chunks,nv) int32 with one row per entry of knn_base, num_chunks, nv >= 1')
    nv = view_frame.size(1)
    if nv * hw >= 2 ** 31 or num_chunks * nv >= 2 ** 31 or not 0 <= n_pts < 2 ** 31:
        raise RuntimeError('lift_vote: needs nv*h*w, num_chunks*nv and n_pts below 2^31')
    if plan is None:
        if len(chunk_inds) != num_chunks:
            raise RuntimeError('lift_vote: {} chunk index lists but {} entries of knn_base'.format(len(chunk_inds), num_chunks))
        plan = D._vote_plan(chunk_inds, n_pts, logit.device)
    lens = [int(i.numel()) for i in plan['keep']]
    if len(lens) != num_chunks:
        raise RuntimeError('lift_vote: the plan lists {} chunks but knn_base {}'.format(len(lens), num_chunks))
    for i, (b, n) in enumerate(zip(knn_base, lens)):
        if not 0 <= int(b) <= knn.size(0) - n:
            raise RuntimeError('lift_vote: chunk {} reads rows {} .. {} of knn, which has {}'.format(i, int(b), int(b) + n, knn.size(0)))
    dev = logit.device
    if n_pts == 0:
        return torch.empty((0, C), dtype=torch.float32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev)
    base = torch.tensor([int(b) for b in knn_base], dtype=torch.int64).to(dev)
    vf = view_frame.to(torch.int32).contiguous()
    total = torch.empty((n_pts, C), dtype=torch.float32, device=dev)
    count = torch.empty((n_pts,), dtype=torch.int32, device=dev)
    L.call('mvp_lift_vote_f32', logit, L.ptr(logit), logit.stride(0), ld_p, logit.stride(1), U, hw, C, L.ptr(vf), nv, L.ptr(knn), knn.size(1),
           L.ptr(base), L.ptr(plan['chunk_offsets']), num_chunks, L.ptr(plan['pt_offsets']), L.ptr(plan['pt_slots']), n_pts, L.ptr(total),
           L.ptr(count))
    return total, count


def vote_finish(total, count):
    """The tail of every vote: total (n,C) float32 sums and count (n,) int32 votes -> (mean (n,C) = total / max(count, 1); label (n,) int64:
    the first maximum, C where count is 0).  One launch (mvp_vote_finish_f32, pinned in include/mvp_hip.h)."""
    mean = torch.empty_like(total)
    label = torch.empty(total.size(0), dtype=torch.int64, device=total.device)
    L.call('mvp_vote_finish_f32', total, L.ptr(total), L.ptr(count), total.size(0), total.size(1), L.ptr(mean), L.ptr(label))
    return mean, label

"""Whole-scene voting on the device (new: the reference propagates every vote's logits to the scene through a scikit-learn ball tree on
the host, one fit + query per vote, mvpnet/test_3d_scene.py:152-164)."""
import torch

from .. import _lib as L

MAX_KEYS = 65536    # mvp_vote_nearest_f32: keys per vote
MAX_CLASSES = 64    # logit columns the kernel keeps in registers

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

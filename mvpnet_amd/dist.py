"""One process per GPU over RCCL/xGMI (torch.distributed backend "nccl" == RCCL on ROCm).

The reference is single-process `nn.DataParallel` (mvpnet/train_mvpnet_3d.py:68-70) and tests
whole scenes strictly sequentially on one GPU (mvpnet/test_mvpnet_3d.py:142-164).  Chunks are
independent units, so the path shards with NO data-path collective:
  * training : each rank takes its slice of the batch; ONE all-reduce of the flattened gradients
               of the ~980k trainable parameters (3.9 MB fp32) per step, divided by world size
               (== DataParallel's mean loss over the full batch when slices are equal);
  * inference: rank r runs chunks r, r+W, ...; ONE all-gather of the per-chunk logits, then every
               rank holds all logits and votes (`vote_scene`) -- chunk_ind is host-known.
Everything except the vote kernels also runs on CPU tensors with the gloo backend (tests).
"""
import os

import torch
import torch.distributed as dist


def init_from_env(backend=None):
    """Initialise torch.distributed from RANK / WORLD_SIZE / MASTER_* (torchrun).  Returns
    (rank, world_size, local_rank).  No-op for a single process."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        if backend is None:  # MVP_DIST_BACKEND: debugging aid (e.g. two ranks on ONE GPU over gloo; RCCL refuses duplicate devices)
            backend = os.environ.get('MVP_DIST_BACKEND') or ('nccl' if torch.cuda.is_available() else 'gloo')
        if backend == 'gloo' and os.environ.get('MASTER_ADDR') in ('127.0.0.1', 'localhost') and os.path.isdir('/sys/class/net/lo'):
            # single-node gloo (tests, --dry, the one-GPU debugging set-ups): pin the transport to the loopback interface.  Left alone gloo
            # looks its interface up through the HOSTNAME, which on a container whose name does not resolve can stall every rank for minutes
            os.environ.setdefault('GLOO_SOCKET_IFNAME', 'lo')
        if backend == 'nccl':
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


def world_size():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def shard_chunks(num_chunks, rank, world):
    """Round-robin chunk ownership: rank r owns r, r+W, r+2W, ...."""
    return list(range(rank, num_chunks, world))


class GradSync:
    """Flat-bucket gradient averaging: one all-reduce per step over all trainable parameters.
    At 3.9 MB the message is latency-bound on xGMI, so a single bucket (not per-layer buckets
    sized for NVSwitch) is the right granularity.

    __call__(weight_sum=None).  The reference computes SegLoss ONCE on the gathered full batch (outside DataParallel):
    weighted cross entropy with ignore_index normalises by the sum of w[y] over the valid points, so the full-batch gradient
    is  sum_r (W_r / W_total) g_r  with g_r the gradient of rank r's mean loss and W_r its weight mass.  Pass the rank's
    W_r (`SegLoss.last_weight_sum`, a 0-dim tensor) to get exactly that -- it travels in the same flat buffer, still ONE
    collective.  Without it the plain mean over ranks is taken (equal to the above only for equal weight masses)."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        self.numel = sum(p.numel() for p in self.params)

    def __call__(self, weight_sum=None):
        w = world_size()
        if w == 1 or not self.params:
            return
        grads = []
        for p in self.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            grads.append(p.grad)
        parts = [g.reshape(-1) for g in grads]
        if weight_sum is not None:
            parts.append(weight_sum.detach().to(device=grads[0].device, dtype=grads[0].dtype).reshape(1))
        flat = torch.cat(parts)                                      # one kernel in, ...
        if weight_sum is not None:
            flat[:-1].mul_(flat[-1])                                 # g_r * W_r  (the last element stays W_r)
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        if weight_sum is not None:
            flat = flat[:-1] / flat[-1].clamp_min(torch.finfo(flat.dtype).tiny)
        else:
            flat.div_(w)
        chunks = [c.view_as(g) for c, g in zip(flat.split([g.numel() for g in grads]), grads)]
        torch._foreach_copy_(grads, chunks)                          # ... one multi-tensor kernel out


def broadcast_parameters(module, src=0):
    """Make every rank start from rank `src`'s weights (DataParallel replicates per step)."""
    if world_size() == 1:
        return
    with torch.no_grad():
        for t in list(module.parameters()) + list(module.buffers()):
            dist.broadcast(t, src=src)
    # Collectives write the storage without bumping the tensors' version counters, so nothing that caches by version sees the new
    # values: drop the cached column-slice operands of the rows kernels and rebuild the folded runtime copy of a frozen 2D network
    # (not a registered sub-module: the loop above did not reach it) from the weights just received.
    from . import rows as R
    R.weight_slices.invalidate()
    for m in module.modules():
        if m.__dict__.get('_fast') is not None and hasattr(m, '_refold'):
            m._refold()


def all_gather_logits(local_logits, num_chunks):
    """local_logits: (n_local, C, N) for the chunks `shard_chunks(num_chunks, rank, W)` in that order (n_local may be 0:
    the tensor must still carry the common C and N).  Returns (num_chunks, C, N) in global chunk order on every rank.
    Ranks with fewer chunks pad.  N must be the same on every rank: ragged chunks are cut / padded to the scene-wide
    maximum of their VALID lengths by the caller (scene.infer_scene), which every rank knows from the chunk index lists."""
    w = world_size()
    if w == 1:
        return local_logits
    per = (num_chunks + w - 1) // w
    if local_logits.size(0) > per:
        raise RuntimeError('all_gather_logits: {} local chunks but at most {} per rank'.format(local_logits.size(0), per))
    pad = per - local_logits.size(0)
    if pad:
        local_logits = torch.cat([local_logits, local_logits.new_zeros((pad,) + tuple(local_logits.shape[1:]))])
    out = local_logits.new_empty((w * per,) + tuple(local_logits.shape[1:]))
    dist.all_gather_into_tensor(out, local_logits.contiguous())
    # out is rank-major [r][j] -> chunk r + j*W
    out = out.view(w, per, *local_logits.shape[1:]).transpose(0, 1).reshape(w * per, *local_logits.shape[1:])
    return out[:num_chunks]


_VOTE_PLANS = {}


def _vote_plan(chunk_inds, n_pts, dev):
    """The transposed index of a scene's chunk lists (for every scene point the flat positions, chunk-major, that name it): one counting
    sort (mvp_csr_build_i64) per scene, cached on the identity of the index tensors."""
    from . import _lib as L
    from . import rows as R
    key = (n_pts, tuple((int(i.data_ptr()), int(i.numel()), int(i._version)) for i in chunk_inds))
    plan = _VOTE_PLANS.get(key)
    if plan is None:
        for ind in chunk_inds:
            L.require_gpu(ind)
        lens = [int(ind.numel()) for ind in chunk_inds]
        flat = torch.cat([ind.reshape(-1) for ind in chunk_inds]) if len(chunk_inds) > 1 else chunk_inds[0].reshape(-1)
        offs = [0]
        for n in lens:
            offs.append(offs[-1] + n)
        pt_offsets, pt_slots = R.build_csr(flat.view(1, -1), n_pts)  # built once per scene; the gather kernel orders each point's slots itself (ascending = chunk order)
        plan = {'chunk_offsets': torch.tensor(offs, dtype=torch.int64).to(dev), 'pt_offsets': pt_offsets, 'pt_slots': pt_slots,
                'max_len': max(lens), 'keep': list(chunk_inds)}  # (the index tensors stay alive: their addresses are the key)
        _VOTE_PLANS.clear()  # one scene at a time
        _VOTE_PLANS[key] = plan
    return plan


def vote_scene(logits, chunk_inds, n_pts):
    """logits: (num_chunks, C, N) on the GPU; chunk_inds: list of int64 tensors (n_i <= N) of scene
    point ids per chunk.  Returns mean logits (n_pts, C), labels (n_pts,) with `count==0 -> C`,
    and the vote count -- the GPU restatement of mvpnet/test_mvpnet_3d.py:136-174."""
    from . import _lib as L
    from .ops.vote import vote_finish
    C = logits.size(1)
    s = torch.zeros(n_pts, C, dtype=torch.float32, device=logits.device)
    cnt = torch.zeros(n_pts, dtype=torch.int32, device=logits.device)  # (no chunks: every point is "no prediction")
    # ONE accumulation launch for the whole scene (the reference loops over the chunks on the host: test_mvpnet_3d.py:142-174), without
    # atomics and adding in chunk order (bit-identical on every rank): every scene point gathers through the transposed index of the
    # concatenated chunk lists.  That index depends on the scene only and is kept for the next call on the same lists.
    if len(chunk_inds):
        if len(chunk_inds) > logits.size(0):  # (the per-chunk loop this launch replaced raised IndexError on the host here)
            raise RuntimeError('vote_scene: {} chunk index lists but logits of {} chunks'.format(len(chunk_inds), logits.size(0)))
        plan = _vote_plan(chunk_inds, n_pts, logits.device)
        if plan['max_len'] > logits.size(2):
            raise RuntimeError('vote_scene: a chunk lists {} points but its logits have {} columns'.format(plan['max_len'], logits.size(2)))
        L.call('mvp_vote_gather_f32', s, L.ptr(logits), logits.stride(0), logits.stride(2), logits.stride(1), L.ptr(plan['chunk_offsets']),
               len(chunk_inds), L.ptr(plan['pt_offsets']), L.ptr(plan['pt_slots']), n_pts, C, L.ptr(s), L.ptr(cnt))
    return (*vote_finish(s, cnt), cnt)

"""The optimizer step and the gradient clip of a training iteration on this library's kernels.

`FusedAdam` (csrc/adam.hip, mvp_adam_step_f32) IS a torch.optim.Adam -- same constructor, same param_groups, same per-parameter state
('step', 'exp_avg', 'exp_avg_sq'), so `state_dict()` / `load_state_dict()` interchange with torch.optim.Adam checkpoints (the reference
saves the optimizer through its Checkpointer, common/utils/checkpoint.py:48-53) and learning-rate schedulers drive it as they drive the
reference's (common/solver/build.py:7-41) -- whose `step()` hands the four pointer lists of all float32 GPU parameters to one kernel
instead of ATen's three multi_tensor_apply launches at the end of the training step's critical stream.

`FusedSGD` (csrc/solver.hip, mvp_sgd_step_f32) is the same for torch.optim.SGD, the optimizer of the 2D stage
(configs/scannet/unet_resnet34.yaml): momentum, dampening, Nesterov and weight decay in one launch per 124 tensors.
`total_grad_norm` / `clip_grad_norm_` are nn.utils.clip_grad_norm_ (train_2d.py:181-185) as two launches per 240 tensors, without
atomics or a host synchronisation, the same bits in every run; FusedSGD.step(grad_scale=coef) applies the clip coefficient while it reads
the gradients, which then are never rewritten."""
import ctypes

import torch

from . import _lib as L


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, **kwargs):
        if amsgrad or kwargs.get('maximize') or kwargs.get('capturable') or kwargs.get('differentiable'):
            raise ValueError('FusedAdam covers plain Adam (no amsgrad / maximize / capturable / differentiable)')
        kwargs.pop('fused', None)
        kwargs.pop('foreach', None)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False, fused=False, **kwargs)
        self._plans = {}  # group index -> cached pointer arrays (parameters and moments do not move; gradients are re-read every step)
        self._step_bufs = {}  # group index -> (host buffer of the group's step counts, its 0-dim views = the states' 'step' tensors)

    def _plan(self, gi, plist):
        key = tuple(id(p) for p in plist)
        plan = self._plans.get(gi)
        if plan is not None and plan['key'] == key and all(p.data_ptr() == q for p, q in zip(plist, plan['pptr'])) \
                and all(self.state[p]['exp_avg'] is m and self.state[p]['exp_avg_sq'] is v for p, m, v in zip(plist, *plan['keep'])):
            return plan  # (load_state_dict replaces the moment tensors: the identity check above then rebuilds the lists)
        n = len(plist)
        arr = lambda vals: (ctypes.c_void_p * n)(*vals)
        moments1 = [self.state[p]['exp_avg'] for p in plist]
        moments2 = [self.state[p]['exp_avg_sq'] for p in plist]
        plan = {'key': key, 'pptr': [p.data_ptr() for p in plist], 'p': arr([p.data_ptr() for p in plist]),
                'm': arr([t.data_ptr() for t in moments1]), 'v': arr([t.data_ptr() for t in moments2]), 'g': (ctypes.c_void_p * n)(),
                'numel': (ctypes.c_int64 * n)(*[p.numel() for p in plist]), 'keep': (moments1, moments2)}
        self._plans[gi] = plan
        return plan

    def _advance_steps(self, gi, plist):
        """+1 on every parameter's step count -> the counts as floats.  Every parameter keeps its OWN host-side float32 step tensor, as
        torch.optim.Adam does (state_dict / checkpoints interchange), but the tensors of a group are 0-dim VIEWS of one host buffer: one
        in-place add and one tolist() per step instead of a 77-tensor foreach add and 77 float() calls (0.3 ms of the step's host time).
        load_state_dict / anybody replacing a state's 'step' is noticed by identity and the buffer rebuilt from the values found."""
        cache = self._step_bufs.get(gi)
        state = self.state
        if cache is None or len(cache[1]) != len(plist) or any(state[p]['step'] is not v for p, v in zip(plist, cache[1])):
            base = torch.tensor([float(state[p]['step']) for p in plist], dtype=torch.float32)
            views = [base[i] for i in range(len(plist))]
            for p, v in zip(plist, views):
                state[p]['step'] = v
            cache = self._step_bufs[gi] = (base, views)
        cache[0].add_(1.0)
        return cache[0].tolist()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group['params'] if p.grad is not None]
            if not plist:
                continue
            for p in plist:
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()) or p.grad.is_sparse:
                    raise RuntimeError('FusedAdam: parameters must be dense contiguous float32 tensors on the GPU (use torch.optim.Adam otherwise)')
                st = self.state[p]
                if len(st) == 0:  # torch.optim.Adam's own lazy state: a float32 step count on the host, zero moments
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            counts = self._advance_steps(gi, plist)
            plan = self._plan(gi, plist)
            grads = []
            g_arr = plan['g']
            for i, p in enumerate(plist):
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():
                    g = g.float().contiguous()
                grads.append(g)
                g_arr[i] = g.data_ptr()
            beta1, beta2 = group['betas']
            dev = plist[0].device
            if any(p.device != dev for p in plist):
                raise RuntimeError('FusedAdam: the parameters of a group must live on one device')
            # The bias corrections depend on the parameter's OWN step count (torch.optim.Adam keeps one per parameter): parameters that
            # skipped an iteration (grad None), were added later or came from a checkpoint with unequal counts get their own launch --
            # one launch per DISTINCT count, i.e. one launch in the usual case.
            if all(c == counts[0] for c in counts):
                buckets = [(counts[0], plan['p'], g_arr, plan['m'], plan['v'], plan['numel'], len(plist))]
            else:
                buckets = []
                for c in sorted(set(counts)):
                    ids = [i for i, ci in enumerate(counts) if ci == c]
                    sub = lambda arr, typ: (typ * len(ids))(*[arr[i] for i in ids])
                    buckets.append((c, sub(plan['p'], ctypes.c_void_p), sub(g_arr, ctypes.c_void_p), sub(plan['m'], ctypes.c_void_p),
                                    sub(plan['v'], ctypes.c_void_p), sub(plan['numel'], ctypes.c_int64), len(ids)))
            with torch.cuda.device(dev):
                for count, p_arr, gg_arr, m_arr, v_arr, n_arr, n in buckets:
                    code = L._fn('mvp_adam_step_f32')(p_arr, gg_arr, m_arr, v_arr, n_arr, n, float(group['lr']), float(beta1), float(beta2),
                                                      float(group['eps']), float(group['weight_decay']), count,
                                                      torch.cuda.current_stream(dev).cuda_stream)
                    if code != 0:
                        L.check(code, 'mvp_adam_step_f32')
            del grads
        return loss


SGD_TENSORS_PER_LAUNCH = 124      # (csrc/solver.hip: kSgdMax)
NORM_TENSORS_PER_LAUNCH = 240     # kNormMax
NORM_THREADS = 256                # lanes of a workgroup of the two norm kernels: a tree of log2(256) = 8 levels
NORM_ELEMENTS_PER_BLOCK = 8192    # gradient elements per partial sum: 32 per lane, added one after the other


class FusedSGD(torch.optim.SGD):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **kwargs):
        if kwargs.get('maximize') or kwargs.get('differentiable'):
            raise ValueError('FusedSGD covers minimising SGD (no maximize / differentiable)')
        # Dropped, not forced to False as FusedAdam does: torch.optim.SGD's own defaults are None, so the param_groups -- and a checkpoint
        # loaded into a plain torch.optim.SGD -- stay those of a default torch optimizer, which then picks its foreach path itself.
        kwargs.pop('fused', None)
        kwargs.pop('foreach', None)
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, **kwargs)
        self._plans = {}  # group index -> cached pointer arrays (parameters and buffers do not move; gradients are re-read every step)

    def _plan(self, gi, plist, use_momentum):
        key = tuple(id(p) for p in plist)
        plan = self._plans.get(gi)
        state = self.state
        if plan is not None and plan['key'] == key and plan['momentum'] == use_momentum \
                and all(p.data_ptr() == q for p, q in zip(plist, plan['pptr'])) \
                and (not use_momentum or all(state[p].get('momentum_buffer') is b for p, b in zip(plist, plan['keep']))):
            return plan  # (load_state_dict replaces the buffers: the identity check above then rebuilds the lists)
        n = len(plist)
        dev = plist[0].device
        for p in plist:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError('FusedSGD: parameters must be dense contiguous float32 tensors on the GPU (use torch.optim.SGD otherwise)')
            if p.device != dev:
                raise RuntimeError('FusedSGD: the parameters of a group must live on one device')
        first = (ctypes.c_uint8 * n)()
        bufs = []
        if use_momentum:
            found = [state[p].get('momentum_buffer') for p in plist]
            for p, b in zip(plist, found):  # (every check before any state is created)
                if b is not None and not (b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.shape == p.shape and b.device == p.device):
                    raise RuntimeError('FusedSGD: momentum buffers must be dense contiguous float32 tensors on the parameter\'s GPU')
            for i, (p, b) in enumerate(zip(plist, found)):
                if b is None:  # torch.optim.SGD's first step of this parameter: the buffer becomes a copy of the gradient (the kernel writes it)
                    b = state[p]['momentum_buffer'] = torch.empty_like(p, memory_format=torch.contiguous_format)
                    first[i] = 1
                bufs.append(b)
        arr = lambda vals: (ctypes.c_void_p * n)(*vals)
        plan = {'key': key, 'momentum': use_momentum, 'pptr': [p.data_ptr() for p in plist], 'p': arr([p.data_ptr() for p in plist]),
                'b': arr([b.data_ptr() for b in bufs]) if use_momentum else None, 'g': (ctypes.c_void_p * n)(),
                'numel': (ctypes.c_int64 * n)(*[p.numel() for p in plist]), 'first': first, 'fresh': any(first), 'keep': bufs}
        self._plans[gi] = plan
        return plan

    def _forget_fresh(self, gi, plist, plan):
        """A step that fails before its launch wrote anything: the buffers made for it hold no values yet, so they and the plan go.
        (A group of more than 124 tensors takes several launches: should a later one fail after an earlier one ran, the earlier tensors
        are already updated and their fresh buffers, which that launch did write, go as well -- they restart from the next gradient.)"""
        for p, f in zip(plist, plan['first']):
            if f:
                del self.state[p]['momentum_buffer']
        self._plans.pop(gi, None)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        """grad_scale: None, or a one-element float32 tensor on the parameters' device (the `coef` of total_grad_norm): every gradient is
        multiplied by it as the kernel reads it."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if grad_scale is not None and not (torch.is_tensor(grad_scale) and grad_scale.is_cuda and grad_scale.dtype == torch.float32
                                           and grad_scale.numel() == 1):
            raise RuntimeError('FusedSGD: grad_scale must be a one-element float32 tensor on the GPU')
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group['params'] if p.grad is not None]
            if not plist:
                continue
            dev = plist[0].device
            if grad_scale is not None and grad_scale.device != dev:
                raise RuntimeError('FusedSGD: grad_scale must live on the parameters\' device')
            momentum = float(group['momentum'])
            plan = self._plan(gi, plist, momentum != 0)  # (checks the parameters whenever one of them is new or has moved)
            grads = []
            g_arr = plan['g']
            for i, p in enumerate(plist):  # the gradients are new tensors every step
                g = p.grad
                if g.dtype != torch.float32 or g.layout != torch.strided or g.device != dev:
                    self._forget_fresh(gi, plist, plan)
                    raise RuntimeError('FusedSGD: gradients must be dense float32 tensors on the parameters\' GPU (use torch.optim.SGD otherwise)')
                if not g.is_contiguous():
                    g = g.contiguous()
                    grads.append(g)  # (kept alive until the launch is enqueued)
                g_arr[i] = g.data_ptr()
            with torch.cuda.device(dev):
                code = L._fn('mvp_sgd_step_f32')(plan['p'], g_arr, plan['b'], plan['numel'], plan['first'], len(plist), float(group['lr']), momentum,
                                                 float(group['dampening']), float(group['weight_decay']), int(bool(group['nesterov'])),
                                                 None if grad_scale is None else grad_scale.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream)
            if code != 0:
                self._forget_fresh(gi, plist, plan)
                L.check(code, 'mvp_sgd_step_f32')
            if plan['fresh']:  # the buffers exist now: later steps take the momentum rule
                ctypes.memset(plan['first'], 0, len(plist))
                plan['fresh'] = False
            del grads
        return loss


_NORM_WORKSPACE = {}


def _norm_workspace(count, device):
    """The partial sums of one call, one buffer per (size, device).  Safe for calls issued on ONE stream per device (the launches run in
    stream order)."""
    ws = _NORM_WORKSPACE.get((count, device))
    if ws is None:
        ws = _NORM_WORKSPACE[(count, device)] = torch.empty(max(count, 1), dtype=torch.float32, device=device)
    return ws


def _dense_grads(parameters, who):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        if g.is_sparse or not g.is_cuda or g.dtype != torch.float32:
            raise RuntimeError('{}: gradients must be dense float32 tensors on the GPU (use torch.nn.utils.clip_grad_norm_ otherwise)'.format(who))
        if g.device != grads[0].device:
            raise RuntimeError('{}: the gradients must live on one device'.format(who))
    return grads


def _norm_launches(grads, max_norm, scale):
    """partials (one launch per 240 tensors) + finish -> (total_norm, coef), 0-dim views of one fresh device tensor."""
    n = len(grads)
    dev = grads[0].device
    g_arr = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
    numel = (ctypes.c_int64 * n)(*[g.numel() for g in grads])
    count = int(L.lib().mvp_grad_clip_partials_count(numel, n))
    if count < 0:
        L.check(count, 'mvp_grad_clip_partials_count')
    ws = _norm_workspace(count, dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        code = L._fn('mvp_grad_sqnorm_partials_f32')(g_arr, numel, n, ws.data_ptr(), None, stream)
        if code != 0:
            L.check(code, 'mvp_grad_sqnorm_partials_f32')
        code = L._fn('mvp_grad_clip_finish_f32')(g_arr if scale else None, numel, n, ws.data_ptr(), count, float(max_norm), out.data_ptr(),
                                                 out.data_ptr() + 4, stream)
        if code != 0:
            L.check(code, 'mvp_grad_clip_finish_f32')
    return out[0], out[1]


def _max_norm(max_norm, who):
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError('{}: max_norm must be >= 0, not {!r}'.format(who, max_norm))
    return max_norm


@torch.no_grad()
def total_grad_norm(parameters, max_norm=None):
    """-> (total_norm, coef), 0-dim float32 tensors on the gradients' device: the 2-norm of all gradients taken as one vector and
    coef = clamp(max_norm / (total_norm + 1e-6), max=1), the factor nn.utils.clip_grad_norm_ would multiply them by (1 when max_norm is
    None).  The gradients are only read: hand `coef` to FusedSGD.step(grad_scale=).  No gradient at all: (0, 1) on the host, as torch.
    The partial sums live in a buffer cached per (count, device) and never freed: issue these calls on ONE stream per device."""
    grads = _dense_grads(parameters, 'total_grad_norm')
    if not grads:
        return torch.tensor(0.0), torch.tensor(1.0)
    return _norm_launches([g if g.is_contiguous() else g.contiguous() for g in grads], -1.0 if max_norm is None else _max_norm(max_norm, 'total_grad_norm'),
                          False)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm):
    """nn.utils.clip_grad_norm_(parameters, max_norm) for the 2-norm: the gradients are scaled in place by
    clamp(max_norm / (total_norm + 1e-6), max=1) -- always, as torch does -- and the total norm comes back as a 0-dim device tensor.
    The partial sums live in a buffer cached per (count, device) and never freed: issue these calls on ONE stream per device."""
    max_norm = _max_norm(max_norm, 'clip_grad_norm_')
    grads = _dense_grads(parameters, 'clip_grad_norm_')
    if not grads:
        return torch.tensor(0.0)
    work = [g if g.is_contiguous() else g.contiguous() for g in grads]
    total, _ = _norm_launches(work, max_norm, True)
    for g, w in zip(grads, work):
        if w is not g:
            g.copy_(w)
    return total

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
the gradients, which then are never rewritten.

`FusedAdam(capturable=True)` + `DeviceMultiStepLR` (csrc/adam.hip: mvp_adam_advance_f32, mvp_adam_step_dev_f32, mvp_lr_multistep_f64) keep
the step number and the learning rate on the device, so clip, step and schedule can be nodes of a captured training step
(mvpnet3d.GraphedTrainStep(solver='captured')): every replay takes the next update at the scheduled rate.  Opt-in; nothing else changes."""
import ctypes

import torch

from . import _lib as L

HYPER_F32 = L.LIMITS['MVP_SOLVER_HYPER_F32']              # floats of a group's hyper block (mvp_adam_advance_f32)
MILESTONE_SLOTS = L.LIMITS['MVP_SOLVER_MILESTONE_SLOTS']  # distinct milestones mvp_lr_multistep_f64 carries by value


class FusedAdam(torch.optim.Adam):
    """capturable=True: the step number and the learning rate live ON THE DEVICE (mvp_adam_advance_f32 + mvp_adam_step_dev_f32), so a
    captured graph that holds step() takes update t + 1 at the current learning rate on every replay.  Then
      * state[p]['step'] is a 0-dim float32 tensor on the parameter's device (torch's own capturable convention), the counts of a group
        being views of one device buffer;
      * group['lr'] stays a Python float for readers, but the LIVE value is device_lr(group_index), one device double per group, which
        DeviceMultiStepLR multiplies in place; state_dict() reads it back into group['lr'] (a synchronisation point);
      * materialize() creates every state and device value eagerly: call it before a capture, where the gradients step() will see exist;
      * step(grad_scale=coef) multiplies every gradient by the device coefficient of total_grad_norm as the kernel reads it.
    param_groups keep torch's `capturable: False`: state_dict() is what a plain torch.optim.Adam loads."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, **kwargs):
        capturable = bool(kwargs.pop('capturable', False))
        if amsgrad or kwargs.get('maximize') or kwargs.get('differentiable'):
            raise ValueError('FusedAdam covers plain Adam (no amsgrad / maximize / differentiable)')
        kwargs.pop('fused', None)
        kwargs.pop('foreach', None)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False, fused=False, **kwargs)
        self.capturable = capturable
        self._plans = {}  # group index -> cached pointer arrays (parameters and moments do not move; gradients are re-read every step)
        self._step_bufs = {}  # group index -> (host buffer of the group's step counts, its 0-dim views = the states' 'step' tensors)
        self._lr_buf = None  # capturable: (n_groups,) float64 on the device, the live learning rates
        self._hyper = None  # capturable: (n_groups, MVP_SOLVER_HYPER_F32) float32 on the device, written by mvp_adam_advance_f32

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

    # ---- capturable=True: counts, learning rates and bias corrections on the device ----
    def _require_capturable(self, what):
        if not self.capturable:
            raise RuntimeError('FusedAdam.{} needs capturable=True'.format(what))

    def _device_values(self):
        """The live learning rates and the hyper blocks, created from group['lr'] (a host-to-device copy: never inside a capture)."""
        n = len(self.param_groups)
        if self._lr_buf is not None and self._lr_buf.numel() == n:
            return self._lr_buf, self._hyper
        devs = {p.device for g in self.param_groups for p in g['params']}
        if len(devs) != 1 or next(iter(devs)).type != 'cuda':
            raise RuntimeError('FusedAdam(capturable=True): all parameters must live on one GPU')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedAdam(capturable=True): call materialize() before the capture')
        dev = next(iter(devs))
        lr = torch.tensor([float(g['lr']) for g in self.param_groups], dtype=torch.float64).to(dev)
        if self._lr_buf is not None:  # add_param_group: the earlier groups keep their live values
            k = min(n, self._lr_buf.numel())
            lr[:k].copy_(self._lr_buf[:k])
        self._lr_buf, self._hyper = lr, torch.zeros(n, HYPER_F32, dtype=torch.float32, device=dev)
        return self._lr_buf, self._hyper

    def device_lr(self, group_index):
        """The live learning rate of a group: a 0-dim float64 view of the device buffer (float() of it synchronises)."""
        self._require_capturable('device_lr')
        return self._device_values()[0][group_index]

    def _new_state(self, p):
        st = self.state[p]
        st['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
        st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _device_counts(self, gi, plist):
        """The step counts of `plist` as ONE float32 device buffer whose 0-dim views are the states' 'step' tensors.  Found by identity, as
        the host buffer of the plain mode; rebuilding it reads the counts back (so never inside a capture) and requires them equal: the
        bias corrections of a launch come from the first."""
        cache = self._step_bufs.get(gi)
        state = self.state
        if cache is not None and len(cache[1]) == len(plist) and all(state[p]['step'] is v for p, v in zip(plist, cache[1])):
            return cache[0]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedAdam(capturable=True): the step counts of the parameters with gradients are not one device buffer yet: '
                               'call materialize() before the capture, where those gradients exist')
        dev = plist[0].device
        base = torch.stack([state[p]['step'].detach().to(device=dev, dtype=torch.float32).reshape(()) for p in plist])
        values = base.tolist()
        if any(v != values[0] for v in values):
            raise RuntimeError('FusedAdam(capturable=True): the parameters of a group that have gradients must have equal step counts '
                               '(found {} to {}); use the non-capturable mode for such a state'.format(min(values), max(values)))
        views = [base[i] for i in range(len(plist))]
        for p, v in zip(plist, views):
            state[p]['step'] = v
        self._step_bufs[gi] = (base, views)
        return base

    @torch.no_grad()
    def materialize(self):
        """capturable=True: creates, eagerly, what step() would create lazily -- moments and counts of EVERY parameter, the device learning
        rates, and each group's count buffer over the parameters that have gradients now (over all of them when none has).  State created
        inside a capture would be zeroed again by every replay, so step() refuses to create any there."""
        self._require_capturable('materialize')
        self._device_values()
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                if len(self.state[p]) == 0:
                    self._check_param(p)
                    self._new_state(p)
            plist = [p for p in group['params'] if p.grad is not None] or list(group['params'])
            if plist:
                self._device_counts(gi, plist)

    @staticmethod
    def _check_param(p):
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()) or (p.grad is not None and p.grad.is_sparse):
            raise RuntimeError('FusedAdam: parameters must be dense contiguous float32 tensors on the GPU (use torch.optim.Adam otherwise)')

    def _step_capturable(self, grad_scale):
        if grad_scale is not None and not (torch.is_tensor(grad_scale) and grad_scale.is_cuda and grad_scale.dtype == torch.float32
                                           and grad_scale.numel() == 1):
            raise RuntimeError('FusedAdam: grad_scale must be a one-element float32 tensor on the GPU')
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group['params'] if p.grad is not None]
            if not plist:
                continue
            dev = plist[0].device
            for p in plist:
                self._check_param(p)
                if p.device != dev:
                    raise RuntimeError('FusedAdam: the parameters of a group must live on one device')
            if grad_scale is not None and grad_scale.device != dev:
                raise RuntimeError('FusedAdam: grad_scale must live on the parameters\' device')
            missing = [p for p in plist if len(self.state[p]) == 0]
            if missing:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError('FusedAdam(capturable=True): a parameter has no optimizer state yet and the stream is capturing (every '
                                       'replay would zero it again): call materialize() before the capture')
                for p in missing:
                    self._new_state(p)
            lr_buf, hyper = self._device_values()
            counts = self._device_counts(gi, plist)
            plan = self._plan(gi, plist)
            grads = []
            g_arr = plan['g']
            for i, p in enumerate(plist):
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():
                    g = g.float().contiguous()
                    grads.append(g)  # (kept alive until the launch is enqueued)
                g_arr[i] = g.data_ptr()
            beta1, beta2 = group['betas']
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                hyper_ptr = hyper.data_ptr() + gi * HYPER_F32 * 4
                code = L._fn('mvp_adam_advance_f32')(counts.data_ptr(), len(plist), lr_buf.data_ptr() + gi * 8, float(beta1), float(beta2),
                                                     hyper_ptr, stream)
                if code != 0:
                    L.check(code, 'mvp_adam_advance_f32')
                code = L._fn('mvp_adam_step_dev_f32')(plan['p'], g_arr, plan['m'], plan['v'], plan['numel'], len(plist), hyper_ptr,
                                                      None if grad_scale is None else grad_scale.data_ptr(), float(beta1), float(beta2),
                                                      float(group['eps']), float(group['weight_decay']), stream)
                if code != 0:
                    L.check(code, 'mvp_adam_step_dev_f32')
            del grads

    def state_dict(self):
        """capturable=True: the plain form -- `lr` a float read back from the device (into group['lr'] as well) and the counts as host
        tensors --, so a torch.optim.Adam loads it.  A SYNCHRONISATION POINT: it waits for the stream."""
        if not self.capturable:
            return super().state_dict()
        if self._lr_buf is not None and self._lr_buf.numel() == len(self.param_groups):
            for group, lr in zip(self.param_groups, self._lr_buf.tolist()):
                group['lr'] = lr
        sd = super().state_dict()
        keys = [k for k, v in sd['state'].items() if torch.is_tensor(v.get('step')) and v['step'].is_cuda]
        if keys:
            host = torch.stack([sd['state'][k]['step'].detach().reshape(()) for k in keys]).cpu()
            for i, k in enumerate(keys):
                sd['state'][k] = dict(sd['state'][k], step=host[i].clone())
        return sd

    def load_state_dict(self, state_dict):
        """Takes the plain form (host counts, `lr` a float) and torch's capturable form (device counts) alike; capturable=True pushes the
        learning rates and the counts to the device.  The group's count buffer is rebuilt -- and the counts required equal -- by the next
        step() or materialize()."""
        super().load_state_dict(state_dict)
        if not self.capturable:
            return
        self._plans.clear()
        self._step_bufs.clear()
        for group in self.param_groups:
            group['capturable'] = False  # (a checkpoint of torch's capturable Adam says True: the flag of this class is self.capturable)
            for p in group['params']:
                st = self.state.get(p)
                if st and 'step' in st:
                    st['step'] = torch.as_tensor(st['step'], dtype=torch.float32).detach().reshape(()).to(p.device)
        self._lr_buf = None
        if any(p.is_cuda for g in self.param_groups for p in g['params']):
            self._device_values()

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        """grad_scale (capturable=True only): None, or a one-element float32 tensor on the parameters' device (the `coef` of
        total_grad_norm): every gradient is multiplied by it as the kernel reads it; the gradients themselves stay unscaled."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.capturable:
            self._step_capturable(grad_scale)
            return loss
        if grad_scale is not None:
            raise ValueError('FusedAdam: grad_scale needs capturable=True (mvp_adam_step_f32 takes no scale)')
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


def multistep_table(milestones, gamma):
    """-> (the distinct milestones, ascending; gamma ** multiplicity of each): the host half of MultiStepLR, whose chainable form multiplies
    the learning rate by gamma ** milestones[epoch] (a Counter) when it reaches a milestone."""
    from collections import Counter
    count = Counter(int(m) for m in milestones)
    distinct = sorted(count)
    return distinct, [float(gamma) ** count[m] for m in distinct]


class DeviceMultiStepLR:
    """torch.optim.lr_scheduler.MultiStepLR on the DEVICE learning rates of a capturable FusedAdam: step() is one launch
    (mvp_lr_multistep_f64) that counts the epoch and multiplies the rates in the doubles torch uses, so a captured graph that holds it
    follows the schedule on every replay.  Nothing is written to param_groups: the optimizer's state_dict() reads the rates back.
    last_epoch=-1 starts at epoch 0 with the optimizer's current rates; a resumed last_epoch takes the current rates as they are, as
    torch does.  `last_epoch` reads the device counter (a synchronisation point)."""

    def __init__(self, optimizer, milestones, gamma=0.1, last_epoch=-1):
        from collections import Counter
        if not (isinstance(optimizer, FusedAdam) and optimizer.capturable):
            raise ValueError('DeviceMultiStepLR drives a FusedAdam(capturable=True): its learning rates live on the device')
        self.optimizer = optimizer
        self.milestones = Counter(int(m) for m in milestones)
        self.gamma = gamma
        if last_epoch == -1:
            for group in optimizer.param_groups:
                group.setdefault('initial_lr', group['lr'])
        elif any('initial_lr' not in g for g in optimizer.param_groups):
            raise KeyError("param 'initial_lr' is not specified in param_groups when resuming an optimizer")
        self.base_lrs = [g['initial_lr'] for g in optimizer.param_groups]
        self._table()
        lr_buf, _ = optimizer._device_values()
        self._epoch = torch.tensor([0 if last_epoch == -1 else int(last_epoch)], dtype=torch.int64).to(lr_buf.device)

    def _table(self):
        distinct, factors = multistep_table(self.milestones.elements(), self.gamma)
        if len(distinct) > MILESTONE_SLOTS:
            raise ValueError('DeviceMultiStepLR holds {} distinct milestones, not {}'.format(MILESTONE_SLOTS, len(distinct)))
        n = len(distinct)
        self._args = ((ctypes.c_int64 * n)(*distinct), (ctypes.c_double * n)(*factors), n)

    @property
    def last_epoch(self):
        return int(self._epoch.item())

    def step(self):
        lr_buf, _ = self.optimizer._device_values()
        dev = lr_buf.device
        with torch.cuda.device(dev):
            code = L._fn('mvp_lr_multistep_f64')(self._epoch.data_ptr(), lr_buf.data_ptr(), lr_buf.numel(), self._args[0], self._args[1],
                                                 self._args[2], torch.cuda.current_stream(dev).cuda_stream)
        if code != 0:
            L.check(code, 'mvp_lr_multistep_f64')

    def get_last_lr(self):
        """-> the live rates, 0-dim float64 device views (one per group)."""
        return [self.optimizer.device_lr(i) for i in range(len(self.optimizer.param_groups))]

    def state_dict(self):
        return {'last_epoch': self.last_epoch, 'milestones': self.milestones, 'gamma': self.gamma, 'base_lrs': list(self.base_lrs)}

    def load_state_dict(self, state_dict):
        """Takes its own form and a torch MultiStepLR.state_dict() of the same schedule; the learning rates are the optimizer's."""
        from collections import Counter
        milestones = Counter({int(k): int(v) for k, v in dict(state_dict['milestones']).items()})
        if milestones != self.milestones or state_dict['gamma'] != self.gamma:
            raise ValueError('DeviceMultiStepLR.load_state_dict: another schedule (milestones {} gamma {}) than this one ({} / {})'.format(
                sorted(milestones.elements()), state_dict['gamma'], sorted(self.milestones.elements()), self.gamma))
        self.base_lrs = list(state_dict['base_lrs'])
        self._epoch.copy_(torch.tensor([int(state_dict['last_epoch'])], dtype=torch.int64))


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

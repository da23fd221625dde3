"""Host side of the stage-one solver (csrc/solver.hip, mvpnet_amd.optim.FusedSGD / total_grad_norm / clip_grad_norm_): argument checks that
return before any launch, the workspace size, and what config.build_optimizer hands a model that is not on the GPU.  No kernel runs."""
import ctypes
import json
import os

import pytest
import torch
import yaml

from tests.conftest import GOLDEN


def test_argument_errors_do_not_launch():
    """Precondition failures of the solver entry points return MVP_E* before any HIP call (safe without a GPU)."""
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    ptrs = (ctypes.c_void_p * 1)(16)
    numel = (ctypes.c_int64 * 1)(8)
    first = (ctypes.c_uint8 * 1)(0)
    sgd = lib.mvp_sgd_step_f32
    #            params grads bufs  numel  first  n   lr    mom  damp  wd  nesterov scale stream
    assert sgd(ptrs, ptrs, ptrs, numel, first, -1, 0.1, 0.9, 0.0, 0.0, 0, None, None) == -1   # n < 0: MVP_EINVAL
    assert sgd(ptrs, ptrs, ptrs, numel, first, 1, 0.1, -0.5, 0.0, 0.0, 0, None, None) == -1   # momentum < 0
    assert sgd(ptrs, ptrs, ptrs, numel, first, 1, -0.1, 0.9, 0.0, 0.0, 0, None, None) == -1   # lr < 0
    assert sgd(ptrs, ptrs, ptrs, numel, first, 1, 0.1, 0.0, 0.0, 0.0, 1, None, None) == -1    # nesterov without momentum
    assert sgd(ptrs, ptrs, ptrs, numel, first, 1, 0.1, 0.9, 0.1, 0.0, 1, None, None) == -1    # nesterov with dampening
    assert sgd(None, ptrs, ptrs, numel, first, 1, 0.1, 0.9, 0.0, 0.0, 0, None, None) == -3    # MVP_ENULL
    assert sgd(ptrs, None, ptrs, numel, first, 1, 0.1, 0.9, 0.0, 0.0, 0, None, None) == -3
    assert sgd(ptrs, ptrs, None, numel, first, 1, 0.1, 0.9, 0.0, 0.0, 0, None, None) == -3    # momentum needs its buffers ...
    assert sgd(ptrs, ptrs, ptrs, numel, None, 1, 0.1, 0.9, 0.0, 0.0, 0, None, None) == -3     # ... and the first-step bytes
    assert sgd(ptrs, ptrs, ptrs, (ctypes.c_int64 * 1)(-1), first, 1, 0.1, 0.9, 0.0, 0.0, 0, None, None) == -1
    assert sgd(ptrs, ptrs, ptrs, (ctypes.c_int64 * 1)(1 << 31), first, 1, 0.1, 0.9, 0.0, 0.0, 0, None, None) == -1
    assert sgd(ptrs, ptrs, ptrs, numel, first, 0, 0.1, 0.9, 0.0, 0.0, 0, None, None) == 0     # nothing to do
    assert sgd(ptrs, ptrs, None, (ctypes.c_int64 * 1)(0), None, 1, 0.1, 0.0, 0.0, 0.0, 0, None, None) == 0  # an empty tensor, no momentum: no launch
    part = lib.mvp_grad_sqnorm_partials_f32
    assert part(ptrs, numel, -1, d, None, None) == -1
    assert part(ptrs, None, 1, d, None, None) == -3
    assert part(None, numel, 1, d, None, None) == -3
    assert part(ptrs, numel, 1, None, None, None) == -3
    assert part(ptrs, (ctypes.c_int64 * 1)(-2), 1, d, None, None) == -1
    count = ctypes.c_int64(-7)
    assert part(ptrs, numel, 0, d, ctypes.byref(count), None) == 0 and count.value == 0      # nothing to do
    fin = lib.mvp_grad_clip_finish_f32
    assert fin(None, None, 0, d, -1, 1.0, d, d, None) == -1                                   # n_partials < 0
    assert fin(None, None, 0, d, 1, float('nan'), d, d, None) == -1
    assert fin(None, None, 0, None, 1, 1.0, d, d, None) == -3
    assert fin(None, None, 0, d, 1, 1.0, None, d, None) == -3
    assert fin(None, None, 0, d, 1, 1.0, d, None, None) == -3
    assert fin(ptrs, numel, 1, d, 2, 1.0, d, d, None) == -1                                   # 8 elements make one partial, not two
    assert fin(ptrs, numel, -1, d, 1, 1.0, d, d, None) == -1


def test_partials_count():
    """one partial sum per 8192 gradient elements of each tensor, rounded up"""
    from mvpnet_amd import _lib, optim
    lib = _lib.lib()
    assert optim.NORM_ELEMENTS_PER_BLOCK == 8192
    sizes = [1, 8191, 8192, 8193, 0, 33000, 3 * 8192]
    assert lib.mvp_grad_clip_partials_count((ctypes.c_int64 * len(sizes))(*sizes), len(sizes)) == 1 + 1 + 1 + 2 + 0 + 5 + 3
    assert lib.mvp_grad_clip_partials_count(None, 0) == 0
    assert lib.mvp_grad_clip_partials_count(None, 1) == -3
    assert lib.mvp_grad_clip_partials_count((ctypes.c_int64 * 1)(8), -1) == -1
    assert lib.mvp_grad_clip_partials_count((ctypes.c_int64 * 1)(-8), 1) == -1
    assert lib.mvp_grad_clip_partials_count((ctypes.c_int64 * 1)(1 << 31), 1) == -1


def test_fused_sgd_constructor():
    from mvpnet_amd.optim import FusedSGD
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        FusedSGD(p, lr=0.1, maximize=True)
    with pytest.raises(ValueError):
        FusedSGD(p, lr=0.1, differentiable=True)
    with pytest.raises(ValueError):
        FusedSGD(p, lr=0.1, nesterov=True)  # torch's own check: Nesterov needs a momentum
    opt = FusedSGD(p, lr=0.1, momentum=0.9, weight_decay=1e-4, foreach=True, fused=False)  # dropped: the step is this library's
    ref = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9, weight_decay=1e-4)
    assert isinstance(opt, torch.optim.SGD)
    assert opt.state_dict()['param_groups'] == ref.state_dict()['param_groups'] and opt.state_dict()['state'] == {}
    p[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match='FusedSGD'):  # no CPU fallback
        opt.step()


def test_host_tensors_are_refused_by_the_clip():
    from mvpnet_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    assert float(optim.clip_grad_norm_([p], 1.0)) == 0.0  # no gradient at all: torch's answer
    total, coef = optim.total_grad_norm([p])
    assert float(total) == 0.0 and float(coef) == 1.0
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match='clip_grad_norm_'):
        optim.clip_grad_norm_([p], 1.0)
    with pytest.raises(RuntimeError, match='total_grad_norm'):
        optim.total_grad_norm(p, 1.0)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([p], -1.0)


def test_build_optimizer_keeps_torch_sgd_on_the_host():
    from mvpnet_amd import config as C
    from mvpnet_amd.optim import FusedSGD
    with open(os.path.join(GOLDEN, 'configs_2d.json')) as f:
        cfg = C.load_cfg(text=yaml.safe_dump(json.load(f)['unet_resnet34']))
    assert cfg.OPTIMIZER.TYPE == 'SGD'
    opt = C.build_optimizer(cfg, torch.nn.Linear(4, 4))
    assert type(opt) is torch.optim.SGD and not isinstance(opt, FusedSGD)
    assert opt.defaults['lr'] == 0.005 and opt.defaults['momentum'] == 0.9 and opt.defaults['weight_decay'] == 1e-4

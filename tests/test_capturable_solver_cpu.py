"""Host side of the capturable solver (csrc/adam.hip: mvp_adam_advance_f32, mvp_adam_step_dev_f32, mvp_lr_multistep_f64;
mvpnet_amd.optim.FusedAdam(capturable=True), DeviceMultiStepLR, multistep_table): the schedule's host half against torch's MultiStepLR in
exact doubles, the argument checks that answer before any launch (null or host pointers only), and the constructor rules.  No GPU."""
import ctypes
import json
import os

import pytest
import torch
import yaml

from tests.conftest import ROOT

EPOCHS = 12


@pytest.mark.parametrize('base_lr', [0.002, 0.004])
@pytest.mark.parametrize('gamma', [0.1, 0.3])
@pytest.mark.parametrize('milestones', [[3], [2, 2, 4], [1, 5, 5, 5], ()])
def test_schedule_table_equals_torch_multisteplr(milestones, gamma, base_lr):
    """What mvp_lr_multistep_f64 does on the device, folded here in Python doubles over optim.multistep_table: the same doubles as torch's
    MultiStepLR stepping an SGD, `==`."""
    from mvpnet_amd.optim import multistep_table
    distinct, factors = multistep_table(milestones, gamma)
    assert distinct == sorted(set(milestones)) and len(factors) == len(distinct)
    assert all(isinstance(f, float) for f in factors)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(milestones), gamma=gamma)
    lr, epoch = base_lr, 0
    for _ in range(EPOCHS):
        opt.step()
        sched.step()
        epoch += 1                      # the kernel's rule: e = *epoch + 1; every milestone == e multiplies; *epoch = e
        for m, f in zip(distinct, factors):
            if m == epoch:
                lr = lr * f
        assert lr == opt.param_groups[0]['lr'] == sched.get_last_lr()[0], (epoch, lr, opt.param_groups[0]['lr'])
    assert epoch == sched.last_epoch


def test_argument_errors_answer_before_any_launch():
    """MVP_EUNSUPPORTED -2, MVP_EINVAL -1, MVP_ENULL -3; every call here fails a check (or has nothing to do), so nothing is launched."""
    from mvpnet_amd import _lib as L
    lib = L.lib()
    assert L.LIMITS['MVP_SOLVER_MILESTONE_SLOTS'] == 16 and L.LIMITS['MVP_SOLVER_HYPER_F32'] == 4
    d = ctypes.c_void_p(16)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    f64 = lambda *v: (ctypes.c_double * len(v))(*v)
    # mvp_lr_multistep_f64(epoch, lr, n_groups, milestones, factors, n_milestones, stream)
    ms = lib.mvp_lr_multistep_f64
    assert ms(d, d, 1, i64(*range(1, 18)), f64(*[0.1] * 17), 17, None) == -2
    assert ms(d, d, 1, i64(4, 2), f64(0.1, 0.1), 2, None) == -1           # descending
    assert ms(d, d, 1, i64(2, 2), f64(0.1, 0.1), 2, None) == -1           # duplicate
    assert ms(d, d, 1, i64(2, 4), f64(0.1, float('nan')), 2, None) == -1  # a NaN factor
    assert ms(d, d, 0, i64(2), f64(0.1), 1, None) == -1                   # n_groups < 1
    assert ms(d, d, 1, i64(2), f64(0.1), -1, None) == -1                  # a negative count
    assert ms(None, d, 1, i64(2), f64(0.1), 1, None) == -3                # epoch
    assert ms(d, None, 1, i64(2), f64(0.1), 1, None) == -3                # lr
    assert ms(d, d, 1, None, f64(0.1), 1, None) == -3
    # mvp_adam_advance_f32(step_counts, n_counts, lr, beta1, beta2, hyper, stream)
    adv = lib.mvp_adam_advance_f32
    assert adv(d, 1, d, 1.0, 0.999, d, None) == -1                        # beta1 = 1
    assert adv(d, 1, d, 0.9, -0.1, d, None) == -1
    assert adv(d, 0, d, 0.9, 0.999, d, None) == -1                        # n_counts = 0
    assert adv(d, -3, d, 0.9, 0.999, d, None) == -1
    assert adv(d, 1, d, 0.9, 0.999, None, None) == -3                     # hyper
    assert adv(d, 1, None, 0.9, 0.999, d, None) == -3                     # lr
    assert adv(None, 1, d, 0.9, 0.999, d, None) == -3
    # mvp_adam_step_dev_f32(params, grads, exp_avg, exp_avg_sq, numel, n, hyper, grad_scale, beta1, beta2, eps, weight_decay, stream)
    step = lib.mvp_adam_step_dev_f32
    ptrs, numel = (ctypes.c_void_p * 1)(16), i64(8)
    assert step(None, None, None, None, None, 0, d, None, 0.9, 0.999, 1e-8, 0.0, None) == 0   # n = 0: nothing to do
    assert step(ptrs, ptrs, ptrs, ptrs, numel, -1, d, None, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert step(ptrs, ptrs, ptrs, ptrs, numel, 1, d, None, 1.0, 0.999, 1e-8, 0.0, None) == -1
    assert step(ptrs, ptrs, ptrs, ptrs, numel, 1, None, None, 0.9, 0.999, 1e-8, 0.0, None) == -3   # hyper
    assert step(ptrs, None, ptrs, ptrs, numel, 1, d, None, 0.9, 0.999, 1e-8, 0.0, None) == -3
    assert step(ptrs, ptrs, ptrs, ptrs, i64(2 ** 31), 1, d, None, 0.9, 0.999, 1e-8, 0.0, None) == -1   # numel < 2^31 - 2048
    assert step(ptrs, ptrs, (ctypes.c_void_p * 1)(None), ptrs, numel, 1, d, None, 0.9, 0.999, 1e-8, 0.0, None) == -3


def test_constructor_rules():
    from mvpnet_amd import config as C
    from mvpnet_amd.optim import DeviceMultiStepLR, FusedAdam
    params = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        FusedAdam(params, capturable=True, amsgrad=True)
    plain = FusedAdam(params, lr=0.002)
    assert plain.capturable is False and plain.param_groups[0]['capturable'] is False
    with pytest.raises(ValueError):
        DeviceMultiStepLR(plain, milestones=[2])
    with pytest.raises(ValueError):
        DeviceMultiStepLR(torch.optim.Adam(params, lr=0.002), milestones=[2])
    with pytest.raises(ValueError):
        plain.step(grad_scale=torch.ones(1))
    cap = FusedAdam(params, lr=0.002, capturable=True)      # constructing needs no GPU; its param_groups stay those of a plain Adam
    assert cap.capturable is True and cap.param_groups[0]['capturable'] is False and cap.param_groups[0]['lr'] == 0.002
    with open(os.path.join(ROOT, 'tests', 'golden', 'configs_2d.json')) as f:
        sgd_cfg = C.load_cfg(text=yaml.safe_dump(json.load(f)['unet_resnet34']))
    assert sgd_cfg.OPTIMIZER.TYPE == 'SGD'
    model = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError):
        C.build_optimizer(sgd_cfg, model, capturable=True)
    with pytest.raises(ValueError):
        C.build_scheduler(sgd_cfg, plain, capturable=True)   # MultiStepLR, but not on a capturable FusedAdam
    assert isinstance(C.build_optimizer(sgd_cfg, model), torch.optim.SGD)   # the default switch: today's path


def test_the_milestone_limit_is_checked_on_the_host_too():
    from mvpnet_amd.optim import MILESTONE_SLOTS, multistep_table
    distinct, factors = multistep_table(list(range(1, MILESTONE_SLOTS + 2)) * 2, 0.5)
    assert len(distinct) == MILESTONE_SLOTS + 1 and factors == [0.25] * (MILESTONE_SLOTS + 1)

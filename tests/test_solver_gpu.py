"""The stage-one solver on the device (csrc/solver.hip): mvpnet_amd.optim.FusedSGD against torch.optim.SGD and a float64 replay of the
rule, optim.total_grad_norm / clip_grad_norm_ against float64 and nn.utils.clip_grad_norm_, config.build_optimizer on the real U-Net and
mvpnet2d.train_step_2d (the reference: common/solver/build.py:7-22, train_2d.py:158-185)."""
import copy
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml
from torch import nn

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

# (momentum, dampening, nesterov, weight_decay): the YAML's, dampening, Nesterov, no momentum
CONFIGS = [(0.9, 0.0, False, 1e-4), (0.9, 0.1, False, 0.0), (0.9, 0.0, True, 1e-2), (0.0, 0.0, False, 1e-2)]
# one element; a tail only; less than a vector per lane; one SGD workgroup exactly; workgroups + a 3-element tail; several workgroups of
# either kernel with a partial last one; one norm workgroup exactly; norm workgroups + a 3-element tail
SHAPES = [(1,), (3,), (64,), (2048,), (4099,), (1000, 33), (5, 7, 3), (128, 259), (8192,), (16387,)]
NONCONTIG = 5   # index of the (1000, 33) parameter: it gets a non-contiguous gradient at one step
SKIPS = 6       # index of the parameter that has no gradient on the first two iterations


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _params(dev, seed, many):
    g = torch.Generator(device='cpu').manual_seed(seed)
    shapes = list(SHAPES)
    if many:
        shapes += [(17 + i,) for i in range(300)]  # more tensors than the argument block of either kernel holds: several launches
    ps = [nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in shapes]
    base = torch.randn(1001, generator=g).to(dev)
    ps.append(nn.Parameter(base[1:]))  # contiguous, but 4 bytes off a 16-byte boundary: the scalar path
    ps.append(nn.Parameter(torch.randn(10, generator=g).to(dev)))  # never receives a gradient
    assert ps[-2].data_ptr() % 16 == 4
    return ps


class Replay:
    """The rule of torch.optim.SGD in the precision of the arrays it is given (float64 NumPy arrays, or float64 tensors)."""

    def __init__(self, values, momentum, dampening, nesterov, weight_decay):
        self.p, self.buf = list(values), [None] * len(values)
        self.momentum, self.dampening, self.nesterov, self.weight_decay = momentum, dampening, nesterov, weight_decay

    def step(self, grads, lr, scale=None):
        for i, g in enumerate(grads):
            if g is None:
                continue
            if scale is not None:
                g = g * scale
            if self.weight_decay != 0:
                g = g + self.weight_decay * self.p[i]
            if self.momentum != 0:
                self.buf[i] = g if self.buf[i] is None else self.momentum * self.buf[i] + (1 - self.dampening) * g
                g = g + self.momentum * self.buf[i] if self.nesterov else self.buf[i]
            self.p[i] = self.p[i] - lr * g


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _maxerr(t, want):
    return float(np.abs(_f64(t).reshape(-1) - np.asarray(want).reshape(-1)).max())


def _hold_to_the_bar(fused, torch_side, want, what):
    """FusedSGD's maximum absolute error to the float64 replay <= 2 x torch.optim.SGD(foreach=False)'s + 1e-12, per tensor.  The kernel
    writes each `x + alpha y` of the rule as one fused multiply-add, 4 roundings per element and step; torch's momentum buffers were
    observed bit-equal to it, so torch appears to round as often, and the factor 2 is then headroom (with every operation rounded on its
    own it would be 6 roundings against 4, a worst-case bound 1.5 x torch's)."""
    worst = 0.0
    for k, (a, b, w) in enumerate(zip(fused, torch_side, want)):
        ea, eb = _maxerr(a, w), _maxerr(b, w)
        worst = max(worst, ea / (eb + 1e-30))
        assert ea <= 2 * eb + 1e-12, (what, k, tuple(a.shape), ea, eb)
    return worst


def _run_sgd(dev, many, momentum, dampening, nesterov, weight_decay, seed=5):
    from mvpnet_amd.optim import FusedSGD
    pa, pb = _params(dev, seed, many), _params(dev, seed, many)
    kw = dict(lr=0.05, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=weight_decay)
    oa, ob = FusedSGD(pa, **kw), torch.optim.SGD(pb, foreach=False, **kw)
    assert isinstance(oa, torch.optim.SGD)
    sa = torch.optim.lr_scheduler.MultiStepLR(oa, milestones=[3], gamma=0.1)
    sb = torch.optim.lr_scheduler.MultiStepLR(ob, milestones=[3], gamma=0.1)
    ref = Replay([_f64(p) for p in pa], momentum, dampening, nesterov, weight_decay)
    gen = torch.Generator(device='cpu').manual_seed(9)
    for it in range(6):
        grads = []
        for k, (a, b) in enumerate(zip(pa[:-1], pb[:-1])):
            gr = torch.randn(a.shape, generator=gen) * (10.0 ** (it % 3 - 1))
            if k == SKIPS and it < 2:  # its first momentum step comes when the others are on their third
                a.grad, b.grad = None, None
                grads.append(None)
                continue
            grads.append(gr.numpy().astype(np.float64))
            a.grad, b.grad = gr.to(dev), gr.to(dev)
        grads.append(None)
        if it == 4:  # a non-contiguous gradient
            pa[NONCONTIG].grad = pa[NONCONTIG].grad.t().contiguous().t()
            assert not pa[NONCONTIG].grad.is_contiguous()
        assert oa.param_groups[0]['lr'] == ob.param_groups[0]['lr']
        ref.step(grads, ob.param_groups[0]['lr'])
        oa.step()
        ob.step()
        sa.step()
        sb.step()
    return pa, pb, oa, ob, ref


@pytest.mark.parametrize('many', [False, True], ids=['few', 'many'])
@pytest.mark.parametrize('momentum,dampening,nesterov,weight_decay', CONFIGS)
def test_fused_sgd_against_torch_and_float64(dev, momentum, dampening, nesterov, weight_decay, many):
    pa, pb, oa, ob, ref = _run_sgd(dev, many, momentum, dampening, nesterov, weight_decay)
    assert oa.param_groups[0]['lr'] == ob.param_groups[0]['lr'] == pytest.approx(0.005)
    worst = _hold_to_the_bar(pa, pb, ref.p, 'parameter')
    if momentum != 0:
        keep = [k for k in range(len(pa) - 1)]
        worst_b = _hold_to_the_bar([oa.state[pa[k]]['momentum_buffer'] for k in keep], [ob.state[pb[k]]['momentum_buffer'] for k in keep],
                                   [ref.buf[k] for k in keep], 'momentum buffer')
        print('worst error ratio to torch: parameters %.3f, buffers %.3f' % (worst, worst_b))
    else:
        print('worst error ratio to torch: parameters %.3f' % worst)
    assert len(oa.state.get(pa[-1], {})) == 0 and pa[-1] not in ob.state  # no gradient, no state
    for a, b in zip(pa, pb):  # the state is exactly what torch leaves (momentum 0: none at all)
        assert set(oa.state.get(a, {}).keys()) == set(ob.state.get(b, {}).keys())
    sd_a, sd_b = oa.state_dict(), ob.state_dict()
    assert sd_a['state'].keys() == sd_b['state'].keys()
    if momentum == 0:
        assert len(sd_a['state']) == 0


def test_fused_sgd_checkpoints_interchange_with_torch_sgd(dev):
    """state_dict() of either optimizer loads into the other and training continues on the same trajectory (the reference's Checkpointer
    stores optimizer.state_dict(): common/utils/checkpoint.py:48-53)."""
    from mvpnet_amd.optim import FusedSGD
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-3)
    pa, pb = _params(dev, 6, False), _params(dev, 6, False)
    oa, ob = FusedSGD(pa, **kw), torch.optim.SGD(pb, foreach=False, **kw)
    ref = Replay([_f64(p) for p in pa], 0.9, 0.0, False, 1e-3)
    gen = torch.Generator(device='cpu').manual_seed(1)

    def run(opts, plists, steps):
        for _ in range(steps):
            grads = [torch.randn(p.shape, generator=gen) for p in plists[0][:-1]]
            ref.step([g.numpy().astype(np.float64) for g in grads] + [None], 0.05)
            for opt, ps in zip(opts, plists):
                for p, gr in zip(ps[:-1], grads):
                    p.grad = gr.to(dev)
                opt.step()

    run((oa, ob), (pa, pb), 3)
    sd_a, sd_b = copy.deepcopy(oa.state_dict()), copy.deepcopy(ob.state_dict())
    assert sd_a['param_groups'][0].keys() == sd_b['param_groups'][0].keys()
    assert sd_a['state'].keys() == sd_b['state'].keys() and set(sd_a['state'][0].keys()) == set(sd_b['state'][0].keys()) == {'momentum_buffer'}
    # cross-load: the fused optimizer continues from torch's state and vice versa
    pc, pd = [nn.Parameter(p.detach().clone()) for p in pb], [nn.Parameter(p.detach().clone()) for p in pa]
    oc, od = FusedSGD(pc, **kw), torch.optim.SGD(pd, foreach=False, **kw)
    oc.load_state_dict(sd_b)
    od.load_state_dict(sd_a)
    run((oa, ob, oc, od), (pa, pb, pc, pd), 2)
    cached = oc.state[pc[0]]['momentum_buffer']
    oc.load_state_dict(copy.deepcopy(oc.state_dict()))  # a load in the middle of training replaces the buffers the step had cached
    assert oc.state[pc[0]]['momentum_buffer'] is not cached
    run((oa, ob, oc, od), (pa, pb, pc, pd), 1)
    for name, ps, opt in (('fused', pa, oa), ('fused from torch\'s state', pc, oc), ('torch from the fused state', pd, od)):
        _hold_to_the_bar(ps, pb, ref.p, name)
        _hold_to_the_bar([opt.state[p]['momentum_buffer'] for p in ps[:-1]], [ob.state[p]['momentum_buffer'] for p in pb[:-1]], ref.buf[:-1],
                         name + ': momentum buffer')
    assert not torch.equal(oc.state[pc[0]]['momentum_buffer'], cached)  # the step wrote the loaded buffer, not the one it replaced


def _grads(dev, many, seed=21):
    """parameters with seeded gradients (the last one without) + the float64 norm of all of them"""
    ps = _params(dev, 3, many)
    gen = torch.Generator(device='cpu').manual_seed(seed)
    sq = 0.0
    for k, p in enumerate(ps[:-1]):
        g = torch.randn(p.shape, generator=gen) * (10.0 ** (k % 3 - 1))
        p.grad = g.to(dev)
        sq += float((g.numpy().astype(np.float64) ** 2).sum())
    return ps, math.sqrt(sq)


def _clone(ps):
    out = [nn.Parameter(p.detach().clone()) for p in ps]
    for p, q in zip(ps, out):
        q.grad = None if p.grad is None else p.grad.clone()
    return out


def _norm_bar(ps):
    """(chain + 2) * 2^-24, chain = the longest run of dependent additions in the two kernels: a lane's elements one after the other, the
    workgroup tree, a lane's partials one after the other, the tree again."""
    from mvpnet_amd import _lib, optim
    sizes = [p.grad.numel() for p in ps if p.grad is not None]
    n_partials = _lib.lib().mvp_grad_clip_partials_count((ctypes.c_int64 * len(sizes))(*sizes), len(sizes))
    assert n_partials == sum(-(-s // optim.NORM_ELEMENTS_PER_BLOCK) for s in sizes)
    tree = int(math.log2(optim.NORM_THREADS))
    chain = optim.NORM_ELEMENTS_PER_BLOCK // optim.NORM_THREADS + tree + -(-n_partials // optim.NORM_THREADS) + tree
    bar = (chain + 2) * 2.0 ** -24
    assert bar <= 1e-5
    return bar


@pytest.mark.parametrize('many', [False, True], ids=['few', 'many'])
@pytest.mark.parametrize('factor', [0.5, 10.0], ids=['clips', 'leaves'])
def test_norm_and_clip_against_float64(dev, factor, many):
    from mvpnet_amd import optim
    ps, norm64 = _grads(dev, many)
    if many:
        assert len(ps) - 1 > optim.NORM_TENSORS_PER_LAUNCH
    bar = _norm_bar(ps)
    max_norm = factor * norm64
    coef64 = min(max_norm / (norm64 + 1e-6), 1.0)
    before = [None if p.grad is None else _f64(p.grad) for p in ps]
    pt = _clone(ps)
    pn = _clone(ps)
    total = optim.clip_grad_norm_(ps, max_norm)
    assert total.is_cuda and total.dim() == 0 and total.dtype == torch.float32 and ps[-1].grad is None
    rel = abs(float(total) - norm64) / norm64
    print('total norm: relative error %.3g, bar %.3g' % (rel, bar))
    assert rel <= bar
    total_t = nn.utils.clip_grad_norm_(pt, max_norm)
    assert abs(float(total) - float(total_t)) <= bar * norm64
    worst = 0.0
    for p, q, g0 in zip(ps[:-1], pt[:-1], before[:-1]):
        want = g0 * coef64
        got = _f64(p.grad)
        scale = np.maximum(np.abs(want), 1e-300)
        worst = max(worst, float((np.abs(got - want) / scale).max()))
        assert np.all(np.abs(got - want) <= (bar + 2.0 ** -23) * np.abs(want)), tuple(p.shape)
        assert np.all(np.abs(got - _f64(q.grad)) <= (bar + 2.0 ** -23) * np.abs(want)), tuple(p.shape)
    print('scaled gradients: worst relative error %.3g, bar %.3g' % (worst, bar + 2.0 ** -23))
    # the read-only form: same norm, same coefficient, gradients untouched
    keep = [None if p.grad is None else p.grad.clone() for p in pn]
    total_n, coef = optim.total_grad_norm(pn, max_norm)
    assert total_n.is_cuda and coef.is_cuda and total_n.dim() == 0 and coef.dim() == 0
    assert float(total_n) == float(total) and abs(float(coef) - coef64) <= (bar + 2.0 ** -23) * coef64
    assert (float(coef) == 1.0) == (factor > 1)
    assert all(torch.equal(p.grad, k) for p, k in zip(pn[:-1], keep[:-1]))
    total_n, coef = optim.total_grad_norm(pn)
    assert float(total_n) == float(total) and float(coef) == 1.0


def test_non_finite_propagates_as_in_torch(dev):
    from mvpnet_amd import optim
    ps, _ = _grads(dev, False)
    ps[4].grad[77] = float('inf')
    pt = _clone(ps)
    total = optim.clip_grad_norm_(ps, 1.0)
    total_t = nn.utils.clip_grad_norm_(pt, 1.0)
    assert math.isinf(float(total)) and float(total) == float(total_t)
    nans = 0
    for p, q in zip(ps[:-1], pt[:-1]):
        assert torch.allclose(p.grad, q.grad, rtol=0.0, atol=0.0, equal_nan=True), tuple(p.shape)
        nans += int(torch.isnan(p.grad).sum())
        assert int((p.grad != 0).sum()) == int(torch.isnan(p.grad).sum())  # zeros and the one NaN
    assert nans == 1 and bool(torch.isnan(ps[4].grad[77]))
    total_n, coef = optim.total_grad_norm(pt, 1.0)  # (of torch's result: a NaN among the gradients)
    assert math.isnan(float(total_n)) and math.isnan(float(coef))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize('many', [False, True], ids=['few', 'many'])
def test_the_clip_is_bit_reproducible(dev, many):
    from mvpnet_amd import optim
    ps, norm64 = _grads(dev, many)
    pa, pb, pc = _clone(ps), _clone(ps), _clone(ps)
    ta, tb = optim.clip_grad_norm_(pa, 0.5 * norm64), optim.clip_grad_norm_(pb, 0.5 * norm64)
    assert torch.equal(_bits(ta), _bits(tb))
    for a, b in zip(pa[:-1], pb[:-1]):
        assert torch.equal(_bits(a.grad), _bits(b.grad))
    # the order of the additions does not depend on a gradient's alignment either
    for k, p in enumerate(pc[:-1]):
        if k % 2 == 0:
            off = torch.empty(p.grad.numel() + 1, device=dev)[1:].view(p.grad.shape)
            off.copy_(p.grad)
            p.grad = off
    tc = optim.clip_grad_norm_(pc, 0.5 * norm64)
    assert pc[0].grad.data_ptr() % 16 == 4 and torch.equal(_bits(tc), _bits(ta))
    for a, c in zip(pa[:-1], pc[:-1]):
        assert torch.equal(_bits(a.grad), _bits(c.grad))


def test_the_deferred_scale_is_the_same_arithmetic(dev):
    """clip_grad_norm_ + step() and total_grad_norm + step(grad_scale=coef) round alike: the scaled gradient is one rounded product in
    both, whether it is stored in between or not."""
    from mvpnet_amd import optim
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-2)
    pa, pb = _params(dev, 8, True), _params(dev, 8, True)
    oa, ob = optim.FusedSGD(pa, **kw), optim.FusedSGD(pb, **kw)
    gen = torch.Generator(device='cpu').manual_seed(4)
    for it in range(3):
        for a, b in zip(pa[:-1], pb[:-1]):
            gr = torch.randn(a.shape, generator=gen).to(dev)
            a.grad, b.grad = gr.clone(), gr.clone()
        keep = [b.grad.clone() for b in pb[:-1]]
        total_a = optim.clip_grad_norm_(pa, 3.0)
        oa.step()
        total_b, coef = optim.total_grad_norm(pb, 3.0)
        ob.step(grad_scale=coef)
        assert torch.equal(_bits(total_a), _bits(total_b)) and 0.0 < float(coef) < 1.0
        for b, k in zip(pb[:-1], keep):
            assert torch.equal(_bits(b.grad), _bits(k))  # read twice, never rewritten
    for a, b in zip(pa, pb):
        assert torch.equal(_bits(a), _bits(b))
    for a, b in zip(pa[:-1], pb[:-1]):
        assert torch.equal(_bits(oa.state[a]['momentum_buffer']), _bits(ob.state[b]['momentum_buffer']))


def test_build_optimizer_gives_the_fused_sgd_on_the_gpu(dev):
    """the 2D stage's own config on the real U-Net: the launch split at the model's true tensor count"""
    from mvpnet_amd import config as C
    from mvpnet_amd import optim
    with open(os.path.join(GOLDEN, 'configs_2d.json')) as f:
        cfg = C.load_cfg(text=yaml.safe_dump(json.load(f)['unet_resnet34']))
    model = C.build_model_sem_seg_2d(cfg).to(dev)
    opt = C.build_optimizer(cfg, model)
    assert isinstance(opt, optim.FusedSGD) and isinstance(opt, torch.optim.SGD)
    group = opt.param_groups[0]
    assert group['lr'] == 0.005 and group['weight_decay'] == 1e-4 and group['momentum'] == 0.9
    pa = [p for p in model.parameters()]
    assert len(pa) > optim.SGD_TENSORS_PER_LAUNCH
    pb = [nn.Parameter(p.detach().clone()) for p in pa]
    ob = torch.optim.SGD(pb, lr=0.005, momentum=0.9, weight_decay=1e-4, foreach=False)
    ref = Replay([p.detach().double() for p in pa], 0.9, 0.0, False, 1e-4)  # (float64 on the device: 23.6 M parameters)
    gen = torch.Generator(device=dev).manual_seed(13)
    for it in range(2):
        grads = [torch.randn(p.shape, generator=gen, device=dev) for p in pa]
        for a, b, g in zip(pa, pb, grads):
            a.grad, b.grad = g.clone(), g.clone()
        ref.step([g.double() for g in grads], 0.005)
        opt.step()
        ob.step()
    err = lambda t, w: float((t.detach().double() - w).abs().max())
    for k, (a, b) in enumerate(zip(pa, pb)):
        ea, eb = err(a, ref.p[k]), err(b, ref.p[k])
        assert ea <= 2 * eb + 1e-12, ('parameter', k, tuple(a.shape), ea, eb)
        ea, eb = err(opt.state[a]['momentum_buffer'], ref.buf[k]), err(ob.state[b]['momentum_buffer'], ref.buf[k])
        assert ea <= 2 * eb + 1e-12, ('momentum buffer', k, tuple(a.shape), ea, eb)


class _TwoConvs(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(3, 8, 3, padding=1), nn.Conv2d(8, 5, 1)

    def forward(self, data_batch):
        return {'seg_logit': self.conv2(torch.relu(self.conv1(data_batch['image'])))}


def test_train_step_2d(dev):
    """One deferred-scale step against one hand-written nn.utils.clip_grad_norm_ + torch.optim.SGD step.  Each side is held to the float64
    replay of a clipped step from ITS OWN fp32 gradients (the two backward passes are tied together by the replays agreeing to 1e-6
    absolute): the fused side's error <= 2 x torch's + 1e-12 (the bar of the FusedSGD tests) PLUS a slack that those tests do not have,
    lr * coef * max|g| * (norm bar + 2^-23) -- what the fp32 norm's error (the bar of the norm tests) may move the update by."""
    from mvpnet_amd import optim
    from mvpnet_amd.mvpnet2d import train_step_2d
    from mvpnet_amd.mvpnet3d import SegLoss
    torch.manual_seed(2)
    ma = _TwoConvs().to(dev)
    mb, mc = copy.deepcopy(ma), copy.deepcopy(ma)
    gen = torch.Generator(device='cpu').manual_seed(17)
    batch = {'image': torch.randn(2, 3, 8, 8, generator=gen).to(dev), 'seg_label': torch.randint(0, 5, (2, 8, 8), generator=gen).to(dev)}
    loss_fn = SegLoss()
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
    max_norm = 0.05
    start = [_f64(p) for p in ma.parameters()]

    def replay(grads):
        """one clipped step in float64 from the fp32 gradients -> (parameters, norm, coefficient)"""
        g64 = [_f64(g) for g in grads]
        norm = math.sqrt(sum(float((g ** 2).sum()) for g in g64))
        coef = min(max_norm / (norm + 1e-6), 1.0)
        ref = Replay(start, 0.9, 0.0, False, 1e-4)
        ref.step(g64, 0.05, scale=coef)
        return ref.p, norm, coef

    # the deferred scale: FusedSGD
    oa = optim.FusedSGD(ma.parameters(), **kw)
    sa = torch.optim.lr_scheduler.MultiStepLR(oa, milestones=[1], gamma=0.1)
    loss_a, preds = train_step_2d(ma, loss_fn, oa, batch, scheduler=sa, max_grad_norm=max_norm)
    assert loss_a.dim() == 0 and not loss_a.requires_grad and tuple(preds['seg_logit'].shape) == (2, 5, 8, 8)
    assert oa.param_groups[0]['lr'] == pytest.approx(0.005)  # the scheduler stepped
    want_a, norm_a, coef_a = replay([p.grad for p in ma.parameters()])  # (the gradients were not rewritten: these are the unclipped ones)
    assert coef_a < 1.0
    # by hand: nn.utils.clip_grad_norm_ + torch.optim.SGD
    ob = torch.optim.SGD(mb.parameters(), foreach=False, **kw)
    ob.zero_grad()
    loss_b = loss_fn(mb(batch), batch)['seg_loss']
    loss_b.backward()
    want_b, norm_b, _ = replay([p.grad for p in mb.parameters()])
    nn.utils.clip_grad_norm_(mb.parameters(), max_norm)
    ob.step()
    assert float(loss_a) == pytest.approx(float(loss_b.detach()), rel=1e-6) and norm_a == pytest.approx(norm_b, rel=1e-5)
    bar = _norm_bar(list(ma.parameters())) + 2.0 ** -23  # of the scaled gradient (test_norm_and_clip_against_float64)
    for a, b, wa, wb in zip(ma.parameters(), mb.parameters(), want_a, want_b):
        ea, eb = _maxerr(a, wa), _maxerr(b, wb)
        slack = 0.05 * float(np.abs(_f64(a.grad)).max()) * coef_a * bar  # what the fp32 norm may move lr * coef * g by
        assert ea <= 2 * eb + 1e-12 + slack, (tuple(a.shape), ea, eb, slack)
        assert float(np.abs(wa - wb).max()) <= 1e-6  # both steps started from the same gradients (two backward passes)
    # any other optimizer: the in-place clip
    oc = torch.optim.Adam(mc.parameters(), lr=1e-3)
    train_step_2d(mc, loss_fn, oc, batch, max_grad_norm=max_norm)
    clipped = math.sqrt(sum(float((_f64(p.grad) ** 2).sum()) for p in mc.parameters()))
    assert clipped == pytest.approx(max_norm, rel=1e-4) and norm_a > 2 * max_norm
    assert all(len(oc.state[p]) > 0 for p in mc.parameters())
    # no clipping asked for: a plain step
    md = copy.deepcopy(mb)
    od = optim.FusedSGD(md.parameters(), **kw)
    train_step_2d(md, loss_fn, od, batch)
    assert all(p.grad is not None and 'momentum_buffer' in od.state[p] for p in md.parameters())

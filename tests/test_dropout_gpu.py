"""The dropout-on training path against an INDEPENDENT keep mask (tests/dropout_oracle.py, confirmed against csrc/dropout.h by
tests/test_dropout_cpu.py): the four kernels that regenerate the mask -- mvp_bn_rows_forward_dropout_f32, mvp_bn_rows_backward_dropout_f32,
mvp_mlp_input_grad_dropout_f32 and mode 2 of mvp_mlp_layer_backward_wide -- must all use the same element index r * C + c, the same 64 -> 32-bit
seed fold and the same 1 / (1 - p).  (a) the three row kernels through the C ABI against float64 torch, (b) the chain as the segmentation
head runs it (merged chain, hand-over to the logit layer, one-pass wide backward), (c) PN2SSG at its default dropout_prob = 0.5."""
import functools

import numpy as np
import pytest
import torch

from tests import dropout_oracle as D

pytestmark = pytest.mark.gpu
HI = torch.float64
SEEDS = (987654321012345, 2 ** 63 - 1, 2 ** 32)   # (2^32 folds to 1; 2^63 - 1 has every bit of both halves set)
LOOSE = {0: 1.0, 6: 1.0, 3: 16.0, 1: 4096.0}      # per contraction precision, as tests/test_ops_gpu.py::test_mlp_kernels_vs_torch


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mvpnet_amd import _lib
    _lib.lib()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device('cuda:0')


class entry_points:
    """The recorder of tests/test_ops_gpu.py, keeping each call's arguments as well: which libmvp_hip.so entry points ran inside the block
    (names as `_lib.call` / `_lib.call_on` get them) and with what -- `args` are the entry point's own arguments, without the leading
    tensor / stream that picks the device."""

    def __enter__(self):
        from mvpnet_amd import _lib as L
        self.L, self.calls = L, []
        self.orig = (L.call, L.call_on)
        orig_call, orig_on, calls = L.call, L.call_on, self.calls

        def call(name, t, *a, **k):
            calls.append((name, a, k))
            return orig_call(name, t, *a, **k)

        def call_on(stream, name, *a, **k):
            calls.append((name, a, k))
            return orig_on(stream, name, *a, **k)

        L.call, L.call_on = call, call_on
        return self

    def __exit__(self, *exc):
        self.L.call, self.L.call_on = self.orig

    def args(self, prefix):
        return [a for n, a, _ in self.calls if n.startswith(prefix)]

    def ran(self, prefix):
        return bool(self.args(prefix))

    def forward_dropout(self):
        """(p, seed, R, C) of the one mvp_bn_rows_forward_dropout_f32 call inside the block."""
        calls = self.args('mvp_bn_rows_forward_dropout')
        assert len(calls) == 1, [n for n, _, _ in self.calls]
        a = calls[0]   # (y, gamma, beta, R, C, training, eps, momentum, relu, running_mean, running_var, stat, mean, invstd, out, partial, p, seed)
        return float(a[16]), int(a[17]), int(a[3]), int(a[4])

    def backward_dropout_ps(self):
        """The drop_p of every mvp_bn_rows_backward_dropout_f32 call (p = 0: the sums-only pass in front of a mode-2 wide backward)."""
        return [float(a[15]) for a in self.args('mvp_bn_rows_backward_dropout')]   # (dsrc, y, 4 x bn, R, C, relu, training, stat, dy, dgamma, dbeta, partial, p, seed)

    def wide_mode2_dropout(self):
        """[(p, seed)] of the one-pass wide backward calls in mode 2 with a dropout to regenerate."""
        # (dsrc, y, mean, invstd, gamma, beta, stat, dgamma, dbeta, training, mode, K, p, seed, ...)
        return [(float(a[12]), int(a[13])) for a in self.args('mvp_mlp_layer_backward_wide_pooled') if a[10] == 2 and a[12] > 0]


@functools.lru_cache(maxsize=None)
def _oracle(p, seed, R, C):
    keep, scale = D.keep_mask(p, seed, R, C)
    return keep, float(scale)


def oracle_mask(p, seed, R, C, dev):
    """-> (keep bool (R, C), keep * scale float64 (R, C)) on the device; scale is the oracle's float32 value."""
    keep, scale = _oracle(float(p), int(seed), int(R), int(C))
    k = torch.from_numpy(keep).to(dev)
    return k, k.to(HI) * scale


# ---------------------------------------------------------------- (a) the row kernels that take (p, seed) directly
_ROWS = {}


def rows_case(R, C, dev, grid=False):
    """y, mean, invstd, gamma, beta (given inputs: the kernels run in eval form or with `stat` of their own) with no float64 bn(y) within
    1e-3 of zero -- the stated condition under which a ReLU decision cannot differ between float32 and float64, so the comparison can be
    element-wise.  grid: every value a small multiple of 1/16, so ((y - mean) * invstd) * gamma + beta is EXACT in float32 (16 significant
    bits at most) and the forward's only rounding is the multiplication by 1 / (1 - p): rtol 1e-6 then holds against float64 itself.
    Built once per shape and never written to."""
    key = (R, C, grid)
    if key not in _ROWS:
        gen = torch.Generator().manual_seed(R * 131 + C + int(grid))
        rnd = lambda *s: torch.randn(*s, generator=gen)
        uni = lambda *s: torch.rand(*s, generator=gen)
        if grid:
            q = lambda t: torch.round(t * 16) / 16
            y, mean, beta = q(rnd(R, C).clamp(-4, 4)), q((rnd(C) * 0.3).clamp(-1, 1)), q((rnd(C) * 0.3).clamp(-1, 1))
            invstd, gamma = q(uni(C) + 0.5), q(uni(C) + 0.5)
        else:
            y, mean, beta = rnd(R, C) * 1.2 + 0.1, rnd(C) * 0.3, rnd(C) * 0.2
            invstd, gamma = uni(C) + 0.5, uni(C) + 0.5
        y, mean, invstd, gamma, beta = [t.to(dev) for t in (y, mean, invstd, gamma, beta)]
        bn = lambda: ((y.to(HI) - mean.to(HI)) * invstd.to(HI)) * gamma.to(HI) + beta.to(HI)
        near = bn().abs() < 1e-3
        if bool(near.any()):
            sign = torch.where(bn() >= 0, 1.0, -1.0)
            if grid:   # one grid step: bn moves by invstd * gamma / 16 >= 1 / 64
                y = torch.where(near, y + sign.float() / 16, y)
            else:      # to +-2e-3 (float64 solve, rounded to float32: bn lands within ~1e-6 of the target)
                target = mean.to(HI) + (sign * 2e-3 - beta.to(HI)) / (gamma.to(HI) * invstd.to(HI))
                y = torch.where(near, target.float(), y)
        assert float(bn().abs().min()) >= 1e-3
        if grid:   # float32, one rounding per operation in the kernel's order: nothing is rounded
            assert torch.equal((((y - mean) * invstd) * gamma + beta).to(HI), bn())
        xh = (y.to(HI) - mean.to(HI)) * invstd.to(HI)
        _ROWS[key] = dict(y=y, mean=mean, invstd=invstd, gamma=gamma, beta=beta, xh=xh, on=bn() > 0, bn=bn())
    return _ROWS[key]


SHAPES = [(333, 32), (4097, 128), (70001, 128)]   # R no multiple of 8, 64 or 128; the last beyond 65536 rows: the input gradient's partials buffer


@pytest.mark.parametrize('p', [0.5, 0.3])          # (0.3 is not dyadic: the float32 rounding of p is in the threshold and in the scale)
@pytest.mark.parametrize('R,C', SHAPES)
def test_forward_kernel_against_the_oracle_mask(dev, R, C, p):
    """mvp_bn_rows_forward_dropout_f32: out == where(keep, relu(bn(y)) * scale, 0) with the oracle's keep and scale -- the zero pattern exactly,
    the values within rtol 1e-6 of float64 (grid inputs: bn(y) is exact in float32, see rows_case)."""
    from mvpnet_amd import _lib as L
    t = rows_case(R, C, dev, grid=True)
    assert torch.equal(t['bn'].float().to(HI), t['bn'])   # the float32 evaluation has nothing to round
    for seed in SEEDS:
        keep, ks = oracle_mask(p, seed, R, C, dev)
        out = torch.full((R, C), float('nan'), device=dev)
        L.call('mvp_bn_rows_forward_dropout_f32', out, L.ptr(t['y']), L.ptr(t['gamma']), L.ptr(t['beta']), R, C, 0, 1e-5, 0.1, 1, None, None, None,
               L.ptr(t['mean']), L.ptr(t['invstd']), L.ptr(out), None, p, seed)
        ref = torch.relu(t['bn']) * ks
        assert torch.equal(out != 0, keep & t['on']), (seed, int(((out != 0) != (keep & t['on'])).sum()))
        np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=1e-6, atol=0, err_msg=str(seed))


@pytest.mark.parametrize('p', [0.5, 0.3])
@pytest.mark.parametrize('R,C', SHAPES)
def test_backward_kernel_against_the_oracle_mask(dev, R, C, p):
    """mvp_bn_rows_backward_dropout_f32 against float64: dz = dsrc * keep * scale * [bn(y) > 0], its two column sums, and
    dy = gamma * invstd * (dz - sum dz / R - xhat * sum(dz * xhat) / R) in training form, gamma * invstd * dz in eval form; also the
    sums-only form (dy == NULL) that runs in front of the one-pass wide backward.  Tolerances of test_mlp_kernels_vs_torch /
    test_input_gradient_with_the_dropout_of_the_layer_in_front (no contraction here: loose = 1)."""
    from mvpnet_amd import _lib as L
    t = rows_case(R, C, dev)
    dsrc = torch.randn(R, C, device=dev, generator=torch.Generator(device=dev).manual_seed(R + C))
    part = lambda: torch.empty(L.lib().mvp_colstats_partial_count(R, C), dtype=HI, device=dev)
    big = max(1.0, R / 5000.0)
    for seed in SEEDS:
        _, ks = oracle_mask(p, seed, R, C, dev)
        dz = torch.where(t['on'], dsrc.to(HI) * ks, torch.zeros((), dtype=HI, device=dev))
        s0, s1 = dz.sum(0), (dz * t['xh']).sum(0)
        sz = max(1.0, float(dz.abs().max()))
        for training in (1, 0, None):   # None: the sums alone
            stat = torch.full((2 * C,), float('nan'), dtype=HI, device=dev)
            dy = torch.full((R, C), float('nan'), device=dev) if training is not None else None
            dgb = torch.full((2, C), float('nan'), device=dev) if training is not None else (None, None)
            L.call('mvp_bn_rows_backward_dropout_f32', dsrc, L.ptr(dsrc), L.ptr(t['y']), L.ptr(t['mean']), L.ptr(t['invstd']), L.ptr(t['gamma']),
                   L.ptr(t['beta']), R, C, 1, int(bool(training)), L.ptr(stat), L.ptr(dy), L.ptr(dgb[0]), L.ptr(dgb[1]), L.ptr(part()), p, seed)
            tag = 'seed={} training={}'.format(seed, training)
            np.testing.assert_allclose(stat[:C].cpu().numpy(), s0.cpu().numpy(), rtol=1e-5, atol=1e-3 * big * sz, err_msg=tag)
            np.testing.assert_allclose(stat[C:].cpu().numpy(), s1.cpu().numpy(), rtol=1e-5, atol=1e-3 * big * sz, err_msg=tag)
            if training is None:
                continue
            ref = (t['gamma'].to(HI) * t['invstd'].to(HI)) * ((dz - s0 / R) - t['xh'] * (s1 / R) if training else dz)
            if not training:   # eval form: the zero pattern is the mask's
                assert torch.equal(dy != 0, ref != 0), tag
            np.testing.assert_allclose(dy.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=2e-5 * max(1.0, float(ref.abs().max())), err_msg=tag)
            np.testing.assert_allclose(dgb[0].cpu().numpy(), s1.cpu().numpy(), rtol=1e-5, atol=1e-3 * big * sz, err_msg=tag)   # dgamma
            np.testing.assert_allclose(dgb[1].cpu().numpy(), s0.cpu().numpy(), rtol=1e-5, atol=1e-3 * big * sz, err_msg=tag)   # dbeta


@pytest.mark.parametrize('precision', ['default', 'bf16x6'])
@pytest.mark.parametrize('p', [0.5, 0.3])
@pytest.mark.parametrize('R,C', SHAPES)
def test_input_gradient_kernel_against_the_oracle_mask(dev, R, C, p, precision):
    """mvp_mlp_input_grad_dropout_f32 (the logit layer's input gradient behind the head: 20 classes) against float64:
    dZ = (dY . W) * keep * scale * [bn(y_prev) > 0] and its two column sums.  atol 2e-5 * max(1, |ref|max) * loose, rtol 1e-5 * loose,
    sums atol 1e-3 * loose * max(1, R / 5000) * max(1, |ref|max) -- test_mlp_kernels_vs_torch's bars with the magnitude factor of
    test_input_gradient_with_the_dropout_of_the_layer_in_front (the kept gradients are scaled up by 1 / (1 - p)); loose per precision
    as there: 1 for bf16x6, 16 for the default backward split bf16x3."""
    from mvpnet_amd import _lib as L
    Cout = 20
    t = rows_case(R, C, dev)
    gen = torch.Generator(device=dev).manual_seed(R + C + 1)
    gy = torch.randn(R, Cout, device=dev, generator=gen)
    w = torch.randn(Cout, C, device=dev, generator=gen) * 0.3
    prec = None if precision == 'default' else (L.MLP_PRECISIONS[precision],) * 2
    loose = LOOSE[L.current_precision()[1] if prec is None else prec[1]]
    plain = gy.to(HI) @ w.to(HI)
    big = max(1.0, R / 5000.0)
    for seed in SEEDS:
        keep, ks = oracle_mask(p, seed, R, C, dev)
        ref = torch.where(t['on'], plain * ks, torch.zeros((), dtype=HI, device=dev))
        dz = torch.full((R, C), float('nan'), device=dev)
        stat = torch.zeros(2 * C, dtype=HI, device=dev)   # accumulated into
        part = torch.empty(((R + 127) // 128) * 2 * C, dtype=HI, device=dev) if R > 65536 else None
        L.call('mvp_mlp_input_grad_dropout_f32', gy, L.ptr(gy), R, Cout, L.ptr(w), C, L.ptr(t['y']), L.ptr(t['mean']), L.ptr(t['invstd']), L.ptr(t['gamma']),
               L.ptr(t['beta']), p, seed, L.ptr(dz), L.ptr(stat), L.ptr(part), prec=prec)
        sz = max(1.0, float(ref.abs().max()))
        tag = 'seed={}'.format(seed)
        assert bool((dz[~(keep & t['on'])] == 0).all()), tag   # exactly zero where dropped or switched off
        np.testing.assert_allclose(dz.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5 * loose, atol=2e-5 * sz * loose, err_msg=tag)
        np.testing.assert_allclose(stat[:C].cpu().numpy(), ref.sum(0).cpu().numpy(), rtol=1e-5 * loose, atol=1e-3 * loose * big * sz, err_msg=tag)
        np.testing.assert_allclose(stat[C:].cpu().numpy(), (ref * t['xh']).sum(0).cpu().numpy(), rtol=1e-5 * loose, atol=1e-3 * loose * big * sz, err_msg=tag)


def test_the_kernels_refuse_what_the_header_refuses(dev):
    """p = 1 and p < 0 are MVP_EINVAL in all three (make_dropout); nothing is launched."""
    from mvpnet_amd import _lib as L
    t = rows_case(333, 32, dev)
    out = torch.empty(333, 32, device=dev)
    for p in (1.0, -0.25):
        with pytest.raises(RuntimeError):
            L.call('mvp_bn_rows_forward_dropout_f32', out, L.ptr(t['y']), L.ptr(t['gamma']), L.ptr(t['beta']), 333, 32, 0, 1e-5, 0.1, 1, None, None, None,
                   L.ptr(t['mean']), L.ptr(t['invstd']), L.ptr(out), None, p, 7)


# ---------------------------------------------------------------- (b) the chain as the head runs it
class switches:
    """Module switches set for a block and put back (no environment variables)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from mvpnet_amd import rows, pn2
        where = {'WIDE_BWD_MIN_ROWS': rows, 'FUSE_DROPOUT': rows, 'MERGE_HEAD': pn2, 'HEAD_HANDOVER': pn2, 'ENABLED': rows.ActivationHandOver}
        self.old = [(where[k], k, getattr(where[k], k)) for k in self.kw]
        for k, v in self.kw.items():
            setattr(where[k], k, v)

    def __exit__(self, *exc):
        for obj, k, v in self.old:
            setattr(obj, k, v)


WIDE = {'lowered': 64, 'off': 1 << 40}   # 'shipped': rows.WIDE_BWD_MIN_ROWS as it is


class HeadChain:
    """SharedMLP(cin, (c1, c2)) + a one-layer SharedMLPDO(c2, (ch,), p) run as ONE chain with the dropout behind the last layer alone, then
    the logit layer (20 x ch, bias) with the chain's ActivationHandOver: what PN2SSG's merged head is to rows.py."""

    def __init__(self, widths, R, bn_train, p, dev):
        from mvpnet_amd.nn import SharedMLP, SharedMLPDO
        cin, c1, c2, ch = widths
        torch.manual_seed(R + sum(widths) + int(bn_train))
        self.body = SharedMLP(cin, (c1, c2), ndim=1, bn=True).to(dev)
        self.head = SharedMLPDO(c2, (ch,), ndim=1, bn=True, p=p).to(dev)
        self.chain = list(self.body) + list(self.head)
        for l in self.chain:
            l.bn.weight.data.uniform_(0.5, 1.5)
            l.bn.bias.data.normal_(0, 0.2)
            l.bn.running_mean.normal_(0, 0.2)
            l.bn.running_var.uniform_(0.5, 1.5)
            l.train(bn_train)
        self.bn_train, self.p, self.R, self.widths, self.dev = bn_train, p, R, widths, dev
        self.W = (torch.randn(20, ch, device=dev) * 0.3).requires_grad_(True)
        self.b = torch.randn(20, device=dev).requires_grad_(True)
        self.x = torch.randn(R, cin, device=dev)
        self.up = torch.randn(R, 20, device=dev)
        self.buffers = [(l.bn.running_mean.clone(), l.bn.running_var.clone(), l.bn.num_batches_tracked.clone()) for l in self.chain]
        self.params = [q for l in self.chain for q in (l.conv.weight, l.bn.weight, l.bn.bias)] + [self.W, self.b]
        self.names = ['dx'] + ['{}{}'.format(n, i) for i in range(len(self.chain)) for n in ('w', 'gamma', 'beta')] + ['W', 'b']

    def run(self, drop_p, mask=None, training=True, backward=True):
        """-> (out, logit, [dx, parameter gradients ...], hand, recorder).  mask: applied to the chain's output by torch, and the logit layer then
        gets no hand-over (the reference form)."""
        from mvpnet_amd import rows as R
        for l, (rm, rv, nbt) in zip(self.chain, self.buffers):   # the same BatchNorm buffers before each run
            l.bn.running_mean.copy_(rm)
            l.bn.running_var.copy_(rv)
            l.bn.num_batches_tracked.copy_(nbt)
        for q in self.params:
            q.grad = None
        xi = self.x.clone().requires_grad_(True)
        hand = R.ActivationHandOver()
        with entry_points() as ep:
            out = R.shared_mlp_rows(xi, self.chain, dropout_p=drop_p, training=training, dropout_last_only=True, act_out=hand)
            info = hand.info
            a = out if mask is None else out * mask
            logit = R.linear_rows(a, self.W, self.b, act_src=hand if mask is None else None)
            if backward:
                logit.backward(self.up)
            torch.cuda.synchronize()
        grads = [xi.grad] + [q.grad for q in self.params] if backward else None
        return out.detach(), logit.detach(), grads, info, ep

    def float64(self, mask64):
        """Plain torch in float64: Linear, BatchNorm (batch statistics in train mode, the running ones in eval mode), ReLU per layer, the mask
        on the head's output only, Linear + bias; differentiated by autograd -> (logit, [dx, parameter gradients ...])."""
        leaf = lambda t: t.detach().to(HI).requires_grad_(True)
        x = leaf(self.x)
        ps = [leaf(q) for q in self.params]
        h = x
        for i, l in enumerate(self.chain):
            w, gamma, beta = ps[3 * i:3 * i + 3]
            y = h @ w.reshape(w.size(0), -1).t()
            if self.bn_train:
                mu, var = y.mean(0), y.var(0, unbiased=False)
            else:
                mu, var = self.buffers[i][0].to(HI), self.buffers[i][1].to(HI)
            h = torch.relu((y - mu) / torch.sqrt(var + l.bn.eps) * gamma + beta)
        logit = (h * mask64) @ ps[-2].t() + ps[-1]
        logit.backward(self.up.to(HI))
        return logit.detach(), [x.grad] + [q.grad for q in ps]


def wide_route_expected(widths, R):
    """rows.wide_backward_ok restated for the chain's layers behind the first, at the default precision (split-bf16, a two-piece backward
    split): more than 64 and at most 128 channels on either side, and enough rows."""
    from mvpnet_amd import rows
    cin, c1, c2, ch = widths
    return any(64 < max(co, ci) <= 128 for co, ci in ((c2, c1), (ch, c2))) and R >= rows.WIDE_BWD_MIN_ROWS


def max_err(a, e):
    return float((a.to(HI) - e.to(HI)).abs().max())


def rel_l2(a, e):
    return float((a.to(HI) - e.to(HI)).norm() / e.to(HI).norm().clamp_min(1e-30))


def route_cases(widths, R):
    """(hand-over, wide) per case.  The wide backward is reached by lowering WIDE_BWD_MIN_ROWS (the small R) and at the shipped threshold
    (R >= 16384), and switched off; the narrow chain (no layer beyond 64 channels) never takes it, whatever the threshold."""
    if max(widths) <= 64:
        wides = ['shipped']
    elif R < 16384:
        wides = ['lowered', 'shipped']
    else:
        wides = ['shipped', 'off']
    return [(hand, wide) for wide in wides for hand in (True, False)]


@pytest.mark.parametrize('bn_train', [True, False])
@pytest.mark.parametrize('R', [333, 4097, 16385, 70001])
@pytest.mark.parametrize('widths', [(64, 128, 128, 128), (32, 64, 64, 32)])
def test_head_chain_against_the_oracle_mask(dev, widths, R, bn_train):
    """The merged head as rows.py runs it, per route (hand-over to the logit layer on / off; one-pass wide backward reached through a
    lowered threshold, at the shipped one, or off), with (p, seed, R, C) read from the mvp_bn_rows_forward_dropout_f32 call and the mask
    built by the oracle from them:
    1. forward: the p = 0 chain times keep * scale (C of the element index = the LAST layer's width), a new mask per call;
    2. backward, element-wise: the p = 0 chain, `out * mask` by torch, the logit layer without hand-over, autograd -- same forward bits, so
       the same ReLU decisions; 2e-5 * |ref|max + 1e-9, times the per-precision `loose` (16: bf16x3) where the wide route ran;
    3. an independent float64 restatement of the whole chain: relative L2 2e-3 (dx) / 5e-3 (every parameter), logits 1e-4 * |ref|max;
    4. what must NOT fold: FUSE_DROPOUT off leaves the hand-over unset and drops through F.dropout; training=False with p > 0 is p = 0.
    Measured on MI355X (largest over all cases): item 2 at most 3.0e-6 of |ref|max on every route, the wide one included
    (2.9e-6); item 3 relative L2 4.0e-4 for dx, 4.3e-4 for a parameter (beta of the first layer, R = 70001), logits 3.9e-7 of |ref|max."""
    from mvpnet_amd import _lib as L
    p = 0.5
    hc = HeadChain(widths, R, bn_train, p, dev)
    ch = widths[-1]
    loose = LOOSE[L.current_precision()[1]]
    f64 = {}
    for hand_on, wide in route_cases(widths, R):
        tag = 'hand={} wide={}'.format(hand_on, wide)
        sw = dict(ENABLED=hand_on, FUSE_DROPOUT=True)
        if wide != 'shipped':
            sw['WIDE_BWD_MIN_ROWS'] = WIDE[wide]
        with switches(**sw):
            expect_wide = wide_route_expected(widths, R)
            assert expect_wide == (max(widths) > 64 and wide != 'off' and (wide == 'lowered' or R >= 16384)), tag   # the case reaches what it is named for
            torch.manual_seed(77)   # (the seed is drawn from torch's CPU generator: the same mask in every route of this test)
            out_d, logit_d, g_d, info, ep = hc.run(p)
            ps, seed, Rr, Cc = ep.forward_dropout()
            assert (ps, Rr, Cc) == (p, R, ch) and 0 <= seed < 2 ** 63, tag
            # which kernels this case covers
            assert ep.ran('mvp_mlp_input_grad_dropout') == hand_on, tag
            assert ep.backward_dropout_ps() == ([] if hand_on else [p]), tag
            assert ep.ran('mvp_mlp_layer_backward_wide') == expect_wide, tag
            assert ep.wide_mode2_dropout() == ([(p, seed)] if (expect_wide and not hand_on) else []), tag
            assert (info is not None) == hand_on and (info is None or (info[5], info[6]) == (p, seed)), tag
            out_0, logit_0, _, _, ep0 = hc.run(0.0, backward=False)
            assert not ep0.ran('mvp_bn_rows_forward_dropout'), tag
            keep, ks = oracle_mask(p, seed, R, ch, dev)
            # 1. forward
            pos = out_0 > 0
            assert torch.equal(out_d != 0, keep & pos), (tag, int(((out_d != 0) != (keep & pos)).sum()))
            np.testing.assert_allclose(out_d.cpu().numpy(), (out_0.to(HI) * ks).cpu().numpy(), rtol=1e-6, atol=0, err_msg=tag)
            with torch.no_grad():
                out_2, _, _, _, ep2 = hc.run(p, backward=False)
            seed2 = ep2.forward_dropout()[1]
            assert seed2 != seed and torch.equal(out_2 != 0, oracle_mask(p, seed2, R, ch, dev)[0] & pos) and not torch.equal(out_2 != 0, out_d != 0), tag
            # 2. backward against the undropped chain times the oracle mask (torch), same route switches
            _, _, g_r, _, epr = hc.run(0.0, mask=ks.float())
            assert not epr.ran('mvp_mlp_input_grad_dropout') and not any(epr.backward_dropout_ps()), tag
            for name, a, e in zip(hc.names, g_d, g_r):
                tol = (2e-5 * float(e.abs().max()) + 1e-9) * (loose if expect_wide else 1.0)
                err = max_err(a, e)
                print('chain {} R={} bn_train={} {} item 2 {}: {:.2e} of |ref|max (bar {:.1e})'.format(widths, R, bn_train, tag, name, err / max(float(e.abs().max()), 1e-30),
                                                                                                      tol / max(float(e.abs().max()), 1e-30)))
                assert err <= tol, (tag, name, err, tol)
        # 3. the float64 restatement (one per mask)
        if seed not in f64:
            f64[seed] = hc.float64(ks)
        logit_r, g_f = f64[seed]
        err = max_err(logit_d, logit_r) / float(logit_r.abs().max())
        print('chain {} R={} bn_train={} {} item 3 logits: {:.2e} of |ref|max'.format(widths, R, bn_train, tag, err))
        assert err <= 1e-4, (tag, err)
        for name, a, e in zip(hc.names, g_d, g_f):
            err = rel_l2(a.reshape(e.shape), e)
            print('chain {} R={} bn_train={} {} item 3 {}: relative L2 {:.2e}'.format(widths, R, bn_train, tag, name, err))
            assert err <= (2e-3 if name == 'dx' else 5e-3), (tag, name, err)
    # 4. what must not fold
    with switches(FUSE_DROPOUT=False):
        out_d, _, g_d, info, ep = hc.run(p)
        assert info is None and not ep.ran('mvp_mlp_input_grad_dropout') and not ep.ran('mvp_bn_rows_forward_dropout') and \
            not any(ep.backward_dropout_ps())
        out_0 = hc.run(0.0, backward=False)[0]
        pos, kept = out_0 > 0, out_d != 0
        assert not bool((kept & ~pos).any()) and abs(float(kept[pos].float().mean()) - (1 - p)) < 0.02
        mask = torch.where(pos, kept.float() / (1 - p), torch.zeros_like(out_0))
        expect_wide = wide_route_expected(widths, R)
        g_r = hc.run(0.0, mask=mask)[2]
        for name, a, e in zip(hc.names, g_d, g_r):
            tol = (2e-5 * float(e.abs().max()) + 1e-9) * (loose if expect_wide else 1.0)
            assert max_err(a, e) <= tol, ('unfused', name, max_err(a, e), tol)
    old = L.set_deterministic(True)   # (ordered reductions instead of float32 atomics: two runs of the same launches agree bit for bit)
    try:
        out_e, logit_e, g_e, _, ep = hc.run(p, training=False)
        out_0, logit_0, g_0, _, _ = hc.run(0.0, training=False)
        assert not ep.ran('mvp_bn_rows_forward_dropout') and not ep.ran('mvp_mlp_input_grad_dropout')
        assert torch.equal(out_e, out_0) and torch.equal(logit_e, logit_0)
        for name, a, e in zip(hc.names, g_e, g_0):
            assert torch.equal(a, e), ('training=False', name, max_err(a, e))
    finally:
        L.set_deterministic(old)


# ---------------------------------------------------------------- (c) the network
@pytest.fixture(scope='module')
def network(dev):
    """PN2SSG at its default dropout_prob (0.5) and its dropout-free twin with the same weights and buffers, the small configuration of
    tests/test_model_gpu.py, B = 2, N = 1024."""
    from mvpnet_amd.pn2 import PN2SSG
    from mvpnet_amd.synthetic import make_chunk
    from tests.conftest import load_golden
    from tests import test_model_gpu as M
    g = load_golden('pn2ssg_small')
    net = PN2SSG(0, 20, **M.CFG)
    assert net.mlp_seg.p == 0.5
    M.load_weights(net, g, 101)
    ref = PN2SSG(0, 20, dropout_prob=0.0, **M.CFG)
    ref.load_state_dict(net.state_dict())
    net, ref = net.to(dev), ref.to(dev)
    chunks = [make_chunk(10 + b, nb_pts=1024, nv=2, h=30, w=40, channels=8, with_feature=False) for b in range(2)]
    points = torch.from_numpy(np.stack([c['points'].T for c in chunks])).to(dev)
    label = torch.from_numpy(np.stack([c['seg_label'] for c in chunks])).to(dev)
    weight = torch.from_numpy(g['log_weights']).to(dev)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    return dict(net=net, ref=ref, points=points, label=label, weight=weight, state=state, refs={})


def _train_step(net, t, state):
    from mvpnet_amd.mvpnet3d import SegLoss
    net.load_state_dict(state)
    net.train()
    net.zero_grad(set_to_none=True)
    with entry_points() as ep:
        logit = net({'points': t['points']})['seg_logit']
        loss = SegLoss(weight=t['weight'])({'seg_logit': logit}, {'seg_label': t['label']})['seg_loss']
        loss.backward()
        torch.cuda.synchronize()
    return logit.detach().clone(), {k: q.grad.clone() for k, q in net.named_parameters()}, ep


@pytest.mark.parametrize('variant', ['merged', 'wide_mode2', 'unmerged'])
def test_pn2ssg_trains_with_the_default_dropout(dev, network, variant):
    """One training step of PN2SSG with dropout_prob left at 0.5 against its dropout-free twin whose mlp_seg output a forward hook multiplies
    by the oracle mask of the (p, seed, R = B * N, C = 128) the step really used (hooks switch the merged head and the hand-over off: the
    reference takes the plain route).  merged: the head inside the last propagation level's chain + the hand-over to the logit layer;
    wide_mode2: WIDE_BWD_MIN_ROWS lowered and the head's hand-over off, so the chain's last layer takes mode 2 of the one-pass backward
    with the dropout; unmerged: MERGE_HEAD off, the head as a chain of its own.  Logits within ATOL['train'], every parameter's gradient
    by assert_grad_close(..., 'train') and the gradient norms as test_pn2ssg_small, every BatchNorm advanced once, equal running statistics."""
    from tests import test_model_gpu as M
    t = network
    net, ref = t['net'], t['ref']
    B, N = t['points'].size(0), t['points'].size(2)
    sw = {'merged': {}, 'wide_mode2': dict(WIDE_BWD_MIN_ROWS=64, HEAD_HANDOVER=False), 'unmerged': dict(MERGE_HEAD=False)}[variant]
    with switches(**sw):
        torch.manual_seed(5)
        logit, grads, ep = _train_step(net, t, t['state'])
    p, seed, R, C = ep.forward_dropout()
    assert (p, R, C) == (0.5, B * N, 128)
    assert ep.ran('mvp_mlp_input_grad_dropout') == (variant == 'merged')
    assert ep.backward_dropout_ps() == ([] if variant == 'merged' else [p])
    assert ep.wide_mode2_dropout() == ([(p, seed)] if variant == 'wide_mode2' else [])
    bns = [m for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert bns and all(int(m.num_batches_tracked) == 1 for m in bns)
    if seed not in t['refs']:   # the reference step, once per mask
        _, ks = oracle_mask(p, seed, R, C, dev)
        mask = ks.float()
        seen = []
        handle = ref.mlp_seg.register_forward_hook(lambda mod, inp, out: (seen.append(tuple(out.shape)), out * mask)[1])
        try:
            rl, rg, rep = _train_step(ref, t, t['state'])
        finally:
            handle.remove()
        assert seen == [(R, C)] and not rep.ran('mvp_bn_rows_forward_dropout') and not rep.ran('mvp_mlp_input_grad_dropout')
        t['refs'][seed] = (rl, rg, {k: v.clone() for k, v in ref.state_dict().items()})
    rl, rg, rstate = t['refs'][seed]
    err = max_err(logit, rl)
    print('PN2SSG {}: logits {:.2e}'.format(variant, err))
    assert err <= M.ATOL['train'], err
    for k in grads:
        M.assert_grad_close(grads[k].cpu().numpy(), rg[k].double().cpu().numpy(), 'train')
    norms = np.asarray([float(grads[k].norm()) for k in grads])
    np.testing.assert_allclose(norms, np.asarray([float(rg[k].norm()) for k in grads]), rtol=5e-2, atol=1e-6)
    for k, v in net.state_dict().items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == 1 == int(rstate[k]), k
        elif 'running_' in k:
            np.testing.assert_allclose(v.cpu().numpy(), rstate[k].cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


def test_pn2ssg_eval_mode_ignores_the_dropout(dev, network):
    """In eval mode the default network's logits are bit-equal to the dropout-free twin's, and no dropout kernel runs."""
    t = network
    for n in (t['net'], t['ref']):
        n.load_state_dict(t['state'])
        n.eval()
    with torch.no_grad(), entry_points() as ep:
        a = t['net']({'points': t['points']})['seg_logit']
    with torch.no_grad():
        b = t['ref']({'points': t['points']})['seg_logit']
    assert not ep.ran('mvp_bn_rows_forward_dropout') and torch.equal(a, b)


def test_forward_hooks_on_the_head_see_and_replace_its_output(dev, network):
    """A forward hook on mlp_seg switches the merged chain off (pn2._has_hooks) -- and then really runs, on the head's (B * N, C) rows: what it
    returns is what the logit layer reads."""
    t = network
    net = t['ref']
    net.load_state_dict(t['state'])
    net.eval()
    with torch.no_grad():
        plain = net({'points': t['points']})['seg_logit']
        seen = []
        handle = net.mlp_seg.register_forward_hook(lambda mod, inp, out: seen.append((mod, tuple(inp[0].shape), out)))   # an observer: returns None
        try:
            watched = net({'points': t['points']})['seg_logit']
        finally:
            handle.remove()
        assert len(seen) == 1 and seen[0][0] is net.mlp_seg and seen[0][1] == (2048, 128) and tuple(seen[0][2].shape) == (2048, 128)
        assert torch.equal(watched, plain)
        handle = net.mlp_seg.register_forward_hook(lambda mod, inp, out: torch.zeros_like(out))
        try:
            zeroed = net({'points': t['points']})['seg_logit']
        finally:
            handle.remove()
        assert torch.equal(zeroed, net.seg_logit.bias.view(1, -1, 1).expand_as(zeroed))
        assert torch.equal(net({'points': t['points']})['seg_logit'], plain)   # (and gone with the hook)

"""The small reductions of the training stream: the two-dimensional statistics reduce (csrc/stats_reduce.h: column slices x row groups),
the column-statistics passes in front of it (csrc/rows.hip) and the wave-coalesced rows path of the loss kernels (csrc/seg.hip).
Shapes sit on the boundaries of the new layouts: 16 row-lanes, 8 loads per lane (128 partial rows per load round), at most 16 row
groups (2048 partial rows), 16-column slices; 64 rows per wave and 256 per workgroup in the loss kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _close(got, want, rtol, atol, what):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    err = np.abs(got - want)
    print('{}: max abs err {:.3e}, max err / (atol + rtol |want|) {:.3f}'.format(what, float(err.max()), float((err / (atol + rtol * np.abs(want))).max())))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


# ---- statistics reduce + BatchNorm finalize behind the tile GEMM -----------------------------------------------------------------

# (partial rows = 128-row tiles, Cout): 1, 15 / 16 / 17 (row-lanes), 127 / 128 / 129 (one load round = one row group), 257 (three groups),
# 2047 / 2048 / 2049 (the 16-group cap: a second round per lane), 3001 (prime); 2 Cout = 8 (less than a slice), 72 (ragged last slice),
# 128, 256, 1024
FINALIZE_CASES = [(1, 4), (1, 512), (15, 36), (16, 64), (17, 128), (127, 512), (128, 36), (129, 64), (129, 4), (257, 128), (2047, 4),
                  (2048, 36), (2049, 64), (3001, 36), (3001, 128)]


@pytest.mark.parametrize('tiles,C', FINALIZE_CASES)
def test_reduce_with_finalize_against_float64(dev, tiles, C):
    """mvp_mlp_forward_bn_p_f32 on the tile GEMM with scratch slots: mean, invstd and the running statistics against float64 of the y
    the call returned (the bar test_ops_gpu.py::test_mlp_forward_with_bn_finalize applies to this entry point: rtol 2e-6, atol 1e-7);
    num_batches_tracked + 1, the ticket slot zero again, a second call on the same arena gives the same, and the forms without running
    statistics and without the finalize (sums only: the eval-mode chain) still work."""
    from mvpnet_amd import _lib as L
    R, Cin = tiles * 128 - (37 if tiles > 1 else 0), 16
    assert (R + 127) // 128 == tiles
    g = torch.Generator().manual_seed(1000 * tiles + C)
    x = (torch.randn(R, Cin, generator=g) + 0.5).to(dev)
    w = (torch.randn(C, Cin, generator=g) * 0.2).to(dev)
    rm0, rv0 = torch.randn(C, generator=g).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
    old = L.lib().mvp_set_mlp_stream(0)  # the tile GEMM, not the persistent streaming kernel
    try:
        part = torch.full((tiles * 2 * C,), float('nan'), dtype=torch.float64, device=dev)
        y = torch.empty(R, C, device=dev)
        stat = torch.zeros(2 * C + 1, dtype=torch.float64, device=dev)
        mean, invstd, rm, rv = torch.empty(C, device=dev), torch.empty(C, device=dev), rm0.clone(), rv0.clone()
        nbt = torch.full((), 5, dtype=torch.int64, device=dev)
        args = lambda m, i, a, b, n: (L.ptr(x), R, Cin, Cin, L.ptr(w), Cin, C, None, None, None, None, L.ptr(y), L.ptr(stat), L.ptr(part), 1e-5, 0.1,
                                      L.ptr(m), L.ptr(i), L.ptr(a), L.ptr(b), L.ptr(n))
        L.call('mvp_mlp_forward_bn_f32', x, *args(mean, invstd, rm, rv, nbt), prec=(-1, -1))
        y64 = y.double()
        m64, v64 = y64.mean(0), y64.var(0, unbiased=False)
        unb = v64 * (R / (R - 1.0))
        bar = dict(rtol=2e-6, atol=1e-7)
        _close(mean, m64, what='mean', **bar)
        _close(invstd, 1.0 / torch.sqrt(v64 + 1e-5), what='invstd', **bar)
        _close(rm, 0.9 * rm0.double() + 0.1 * m64, what='running_mean', **bar)
        _close(rv, 0.9 * rv0.double() + 0.1 * unb, what='running_var', **bar)
        _close(stat[:C], y64.sum(0), rtol=1e-6, atol=1e-3, what='sum y')
        _close(stat[C:2 * C], (y64 * y64).sum(0), rtol=1e-6, atol=1e-3, what='sum y^2')
        assert int(nbt) == 6
        assert stat[-1].item() == 0.0  # the ticket behind the sums
        # the same arena again (sums cleared by the caller, the ticket as the kernel left it), without running statistics
        stat[:2 * C].zero_()
        mean2, invstd2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
        L.call('mvp_mlp_forward_bn_f32', x, *args(mean2, invstd2, None, None, None), prec=(-1, -1))
        _close(mean2, mean, what='mean, second call', **bar)
        _close(invstd2, invstd, what='invstd, second call', **bar)
        assert stat[-1].item() == 0.0 and int(nbt) == 6
        # sums only (mvp_mlp_forward_f32 with scratch slots: what the chain calls outside training): the plain reduce
        stat3 = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        L.call('mvp_mlp_forward_f32', x, L.ptr(x), R, Cin, Cin, L.ptr(w), Cin, C, None, None, None, None, None, L.ptr(y), L.ptr(stat3), L.ptr(part),
               prec=(-1, -1))
        _close(stat3, stat[:2 * C], rtol=1e-12, atol=1e-9 * R, what='plain reduce against the finalize form')
    finally:
        L.lib().mvp_set_mlp_stream(old)


# ---- plain reduce behind the column statistics ------------------------------------------------------------------------------------

# workgroups of the scratch variant = partial rows (one per 16 KB of rows, 16 .. 1024); C / 4 divides 256 in these passes
@pytest.mark.parametrize('slots,C', [(16, 4), (16, 512), (17, 64), (127, 128), (128, 8), (129, 64), (257, 512), (1023, 64), (1024, 128), (997, 8)])
def test_plain_reduce_behind_colstats(dev, slots, C):
    """mvp_colstats_f32 with a scratch buffer (per-workgroup slots + the reduce) against float64 and against the fp64-atomics variant,
    with the bars of test_ops_gpu.py::test_column_statistics_scratch_variant."""
    from mvpnet_amd import _lib as L
    R = slots * 16 * 1024 // (4 * C) - 3 if slots > 16 else 45
    if slots == 1024:
        R = 3 * R + 1  # beyond the cap: three passes per workgroup and a ragged last one
    n = L.lib().mvp_colstats_partial_count(R, C)
    assert n == slots * 2 * C
    y = (torch.randn(R, C, generator=torch.Generator().manual_seed(slots + C)) * 2 + 0.5).to(dev)
    ref = torch.cat([y.double().sum(0), (y.double() ** 2).sum(0)])
    got = []
    for use in (True, False):
        part = torch.full((n,), float('nan'), dtype=torch.float64, device=dev) if use else None
        st = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        L.call('mvp_colstats_f32', y, L.ptr(y), R, C, L.ptr(st), L.ptr(part))
        L.call('mvp_colstats_f32', y, L.ptr(y), R, C, L.ptr(st), L.ptr(part))  # accumulated into
        _close(st, 2 * ref, rtol=1e-6, atol=1e-3, what='sums, scratch' if use else 'sums, atomics')
        got.append(st)
    _close(got[0], got[1], rtol=1e-6, atol=1e-3, what='scratch against atomics')


# ---- BatchNorm-backward column sums -----------------------------------------------------------------------------------------------

def _bn_inputs(G, K, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(G * K, C, generator=g) * 1.5 + 0.2).to(dev)
    dsrc = torch.randn(G, C, generator=g).to(dev)
    mean, invstd = (torch.randn(C, generator=g) * 0.3).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.2).to(dev)
    return y, dsrc, mean, invstd, gamma, beta


def _both_variants(call, R_for_count, C, dev):
    """call(stat, partial) with the scratch slots and with the fp64 atomics -> the two (2C) sums"""
    from mvpnet_amd import _lib as L
    out = []
    for use in (True, False):
        part = torch.full((L.lib().mvp_colstats_partial_count(R_for_count, C),), float('nan'), dtype=torch.float64, device=dev) if use else None
        st = torch.full((2 * C,), float('nan'), dtype=torch.float64, device=dev)  # (re)initialised by the call
        call(st, part)
        out.append(st)
    return out


# rows per pass of a workgroup = 256 / (C / 4): 256, 16, 4.  One group; fewer rows than one workgroup's share; R no multiple of
# K x rows per pass; a few thousand groups
@pytest.mark.parametrize('relu', [1, 0])
@pytest.mark.parametrize('G,K,C', [(1, 3, 4), (1, 1, 64), (37, 3, 64), (3001, 3, 64), (1001, 3, 256), (3001, 1, 256), (5003, 1, 4), (2500, 3, 4)])
def test_backward_sums_of_a_sum_over_the_neighbours(dev, G, K, C, relu):
    """mvp_bn_rows_backward_f32 with dy == NULL: K = 3 (BwdSum: every row of a group receives the group's gradient) and K = 1."""
    from mvpnet_amd import _lib as L
    y, dsrc, mean, invstd, gamma, beta = _bn_inputs(G, K, C, dev, G * K + C)
    R = G * K
    call = lambda st, part: L.call('mvp_bn_rows_backward_f32', y, L.ptr(dsrc), None, None, L.ptr(y), L.ptr(mean), L.ptr(invstd), L.ptr(gamma),
                                   L.ptr(beta), G, K, C, relu, 1, L.ptr(st), None, None, None, L.ptr(part))
    scratch, atomics = _both_variants(call, R, C, dev)
    xh32 = (y - mean) * invstd  # the ReLU decision in float32, as the kernel takes it
    mask = (xh32 * gamma + beta > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    dz = torch.where(mask, dsrc.double().repeat_interleave(K, 0), torch.zeros((), dtype=torch.float64, device=dev))
    xh = (y.double() - mean.double()) * invstd.double()
    ref = torch.cat([dz.sum(0), (dz * xh).sum(0)])
    _close(scratch, ref, rtol=1e-6, atol=1e-3, what='scratch against float64')
    _close(atomics, ref, rtol=1e-6, atol=1e-3, what='atomics against float64')
    _close(scratch, atomics, rtol=1e-6, atol=1e-4, what='scratch against atomics')


@pytest.mark.parametrize('G,K,C', [(1, 8, 64), (37, 8, 4), (3001, 4, 64), (1001, 4, 256)])
def test_backward_sums_of_a_max_over_the_neighbours(dev, G, K, C):
    """BwdMax (mvp_bn_rows_backward_f32 with the arg-max of the forward) and BwdMaxSel (mvp_pool_backward_stats_f32) from the same layer."""
    from mvpnet_amd import _lib as L
    y, dsrc, _, _, gamma, beta = _bn_inputs(G, K, C, dev, G + K + C)
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    out, arg = torch.empty(G, C, device=dev), torch.empty(G, C, dtype=torch.uint8, device=dev)
    st0 = torch.empty(2 * C, dtype=torch.float64, device=dev)
    L.call('mvp_bn_rows_forward_f32', y, L.ptr(y), L.ptr(gamma), L.ptr(beta), G, K, C, 1, 1e-5, 0.1, 1, None, None, L.ptr(st0), L.ptr(mean),
           L.ptr(invstd), L.ptr(out), L.ptr(arg), None)
    dy = torch.empty(G * K, C, device=dev)
    call = lambda st, part: L.call('mvp_bn_rows_backward_f32', y, L.ptr(dsrc), L.ptr(out), L.ptr(arg), L.ptr(y), L.ptr(mean), L.ptr(invstd),
                                   L.ptr(gamma), L.ptr(beta), G, K, C, 1, 1, L.ptr(st), L.ptr(dy), None, None, L.ptr(part))
    scratch, atomics = _both_variants(call, G, C, dev)
    ysel = torch.gather(y.view(G, K, C), 1, arg.long().unsqueeze(1)).squeeze(1).contiguous()  # the pre-BN value behind the pooled output
    dz = torch.where(out > 0, dsrc.double(), torch.zeros((), dtype=torch.float64, device=dev))
    xh = (ysel.double() - mean.double()) * invstd.double()
    ref = torch.cat([dz.sum(0), (dz * xh).sum(0)])
    _close(scratch, ref, rtol=1e-6, atol=1e-3, what='BwdMax, scratch against float64')
    _close(atomics, ref, rtol=1e-6, atol=1e-3, what='BwdMax, atomics against float64')
    _close(scratch, atomics, rtol=1e-6, atol=1e-4, what='BwdMax, scratch against atomics')
    call = lambda st, part: L.call('mvp_pool_backward_stats_f32', y, L.ptr(dsrc), L.ptr(out), L.ptr(ysel), L.ptr(mean), L.ptr(invstd), G, C, 1, L.ptr(st),
                                   L.ptr(part))
    scratch, atomics = _both_variants(call, G, C, dev)
    _close(scratch, ref, rtol=1e-6, atol=1e-3, what='BwdMaxSel, scratch against float64')
    _close(atomics, ref, rtol=1e-6, atol=1e-3, what='BwdMaxSel, atomics against float64')
    _close(scratch, atomics, rtol=1e-6, atol=1e-4, what='BwdMaxSel, scratch against atomics')


# ---- loss on channels-last rows ----------------------------------------------------------------------------------------------------

def _loss_and_grad(logit, label, weight):
    from mvpnet_amd.mvpnet3d import SegLoss
    a = logit.detach().requires_grad_(True)
    loss = SegLoss(weight=weight)({'seg_logit': a}, {'seg_label': label})['seg_loss']
    (loss * 1.5).backward()
    return loss.detach(), a.grad


@pytest.mark.parametrize('C', [20, 4])
@pytest.mark.parametrize('B,N', [(1, 1), (1, 63), (1, 64), (1, 65), (1, 64 * 5 + 17), (1, 256 * 3 + 17), (3, 337), (1, 10007), (2, 5003)])
def test_loss_on_rows_against_float64(dev, B, N, C):
    """Rows layout ((B,N,C) memory viewed as (B,C,N)): loss and gradient against F.cross_entropy in float64 and against the (B,C,N)
    layout of the same logits (the strided path), with the bars of test_seg_gpu.py (loss rtol 1e-5; gradient rtol 1e-4, atol 1e-10).
    Ignored and out-of-range labels (skipped like ignored ones); an unaligned base pointer takes the strided path."""
    g = torch.Generator().manual_seed(B * N + C)
    rows = (torch.randn(B, N, C, generator=g) * 2).to(dev)
    label = torch.randint(0, C, (B, N), generator=g)
    drop = torch.rand(B, N, generator=g)
    label[drop < 0.1] = -100
    if N > 4:
        label[drop > 0.97] = C + 3  # out of range above
        label[(drop > 0.94) & (drop <= 0.97)] = -5  # and below
        label[0, 0] = 0  # at least one valid point
    else:
        label[:] = C - 1
    label = label.to(dev)
    weight = (torch.rand(C, generator=g) + 0.5).to(dev)
    valid = (label >= 0) & (label < C)
    ref_label = torch.where(valid, label, torch.full_like(label, -100))
    shifted = torch.empty(B * N * C + 1, device=dev)[1:].view(B, N, C)  # base pointer 4 bytes off a 16-byte boundary
    shifted.copy_(rows)
    assert rows.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    for w in (weight, None):
        ref_in = rows.transpose(1, 2).double().contiguous().requires_grad_(True)
        ref = F.cross_entropy(ref_in, ref_label, weight=None if w is None else w.double(), ignore_index=-100)
        (ref * 1.5).backward()
        la, ga = _loss_and_grad(rows.transpose(1, 2), label, w)
        assert ga.stride() == rows.transpose(1, 2).stride()  # the gradient comes back as rows
        lb, gb = _loss_and_grad(rows.transpose(1, 2).contiguous(), label, w)
        lc, gc = _loss_and_grad(shifted.transpose(1, 2), label, w)
        for name, l, gr in (('rows', la, ga), ('(B,C,N)', lb, gb), ('unaligned rows', lc, gc)):
            _close(l, ref, rtol=1e-5, atol=0.0, what='loss, ' + name)
            _close(gr, ref_in.grad, rtol=1e-4, atol=1e-10, what='gradient, ' + name)
        _close(la, lb, rtol=1e-5, atol=0.0, what='loss, rows against (B,C,N)')
        _close(ga, gb, rtol=1e-4, atol=1e-10, what='gradient, rows against (B,C,N)')
        assert float(ga.transpose(1, 2)[~valid].abs().sum()) == 0.0  # skipped points get exact zeros


@pytest.mark.parametrize('C', [20, 4])
def test_loss_on_rows_with_nothing_valid(dev, C):
    """Every label ignored: 0 / 0 = nan, as torch; one whole wave of ignored rows next to valid ones."""
    from mvpnet_amd.mvpnet3d import SegLoss
    rows = torch.randn(1, 200, C, device=dev)
    label = torch.full((1, 200), -100, dtype=torch.int64, device=dev)
    loss = SegLoss()({'seg_logit': rows.transpose(1, 2)}, {'seg_label': label})['seg_loss']
    assert torch.isnan(loss) and torch.isnan(F.cross_entropy(rows.transpose(1, 2), label))
    label[0, 130] = C - 1  # rows 0 .. 127: two waves with nothing valid
    loss, grad = _loss_and_grad(rows.transpose(1, 2), label, None)
    ref = -torch.log_softmax(rows[0, 130].double(), 0)[C - 1]
    _close(loss, ref, rtol=1e-5, atol=0.0, what='loss of the one valid row')
    gz = grad.transpose(1, 2).clone()
    gz[0, 130] = 0
    assert float(gz.abs().sum()) == 0.0


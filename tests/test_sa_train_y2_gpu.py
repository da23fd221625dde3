"""The fused training level with y_2 STORED once (mvp_sa_train_forward_y2_f32 / mvp_sa_train_backward_y2_f32, csrc/sa_train.hip) against
the same passes re-creating it: the entry points called directly with FIXED BatchNorm-1 / BatchNorm-2 constants, so nothing depends on
the arrival order of another pass' atomics.  What a pass writes per row or per ball (the pooled extremes, dz) must be the same bit for
bit; what it sums with atomics over the workgroups follows the convention of tests/test_ops_gpu.py (rtol 1e-4, atol 1e-5 * max)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 32
# widths, B, N, M, fraction of empty slots: the two shipped instances, widths that are no multiple of the 32-channel block (the column
# masks of the store and of the loads), (64, 64, 64); 14 balls = not a multiple of the four waves; B * M > 4096; empty slots (-1)
CASES = {
    'level1': ((32, 32, 64), 2, 300, 7, 0.0),
    'level2': ((64, 64, 128), 2, 300, 7, 0.0),
    'masked': ((12, 20, 40), 2, 300, 7, 0.0),
    'w64': ((64, 64, 64), 2, 300, 7, 0.0),
    'many': ((64, 64, 128), 2, 512, 2500, 0.0),
    'holes1': ((32, 32, 64), 2, 300, 50, 0.2),
    'holes2': ((64, 64, 128), 2, 300, 50, 0.2),
}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mvpnet_amd import _lib
    _lib.lib()
    return torch.device('cuda:0')


def bn_constants(C, dev):
    return [torch.randn(C, device=dev) * 0.3, torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2]


@functools.lru_cache(maxsize=None)
def level(name):
    """The level's inputs and what the FORWARD leaves for the other tests: Y2 from a storing stage 2, BatchNorm 3 from a re-computing stage 3."""
    from mvpnet_amd import _lib as L
    dev = torch.device('cuda:0')
    (C1, C2, C3), B, N, M, holes = CASES[name]
    gen = torch.Generator(device='cpu').manual_seed(sum(map(ord, name)))
    torch.manual_seed(sum(map(ord, name)))
    c = dict(name=name, dims=(B, N, M, C1, C2, C3), G=B * M, R=B * M * K)
    c['zf'] = torch.randn(B, N, C1, device=dev)
    c['xyz'] = torch.rand(B, N, 3, device=dev)
    c['centre'] = torch.rand(B, M, 3, device=dev)
    index = torch.randint(0, N, (B, M, K), generator=gen)
    if holes:
        hole = torch.rand(index.shape, generator=gen) < holes
        hole[..., 0] = False
        index[hole] = -1
        index[0, 3] = -1   # a ball without any neighbour
    c['index'] = index.to(dev)
    c['wxyz'] = torch.randn(C1, 3, device=dev) * 0.5
    c['bn1'] = bn_constants(C1, dev)
    c['W2'] = torch.randn(C2, C1, device=dev) * 0.2
    c['bn2'] = bn_constants(C2, dev)
    c['W3'] = torch.randn(C3, C2, device=dev) * 0.2
    c['Y2'] = torch.full((c['R'], C2), float('nan'), device=dev)
    c['stage2'] = forward(c, 2, c['Y2'])
    c['stage3'] = forward(c, 3, None)
    torch.cuda.synchronize()
    return c


def level_args(c):
    from mvpnet_amd import _lib as L
    B, N, M, C1, C2, C3 = c['dims']
    return (L.ptr(c['zf']), L.ptr(c['xyz']), L.ptr(c['centre']), L.ptr(c['index']), L.ptr(c['wxyz']), B, N, M, K, C1, *map(L.ptr, c['bn1']),
            L.ptr(c['W2']), C2)


def forward(c, stage, y2):
    """-> dict(mean, invstd[, ymax, ymin, amax, amin]) of forward pass `stage`; y2: the tensor stage 2 writes / stage 3 reads, or None."""
    from mvpnet_amd import _lib as L
    B, N, M, C1, C2, C3 = c['dims']
    dev = c['zf'].device
    C = C2 if stage == 2 else C3
    stat = torch.zeros(2 * C + 1, dtype=torch.float64, device=dev)
    o = dict(mean=torch.empty(C, device=dev), invstd=torch.empty(C, device=dev))
    if stage == 3:
        for k, dt in (('ymax', torch.float32), ('ymin', torch.float32), ('amax', torch.uint8), ('amin', torch.uint8)):
            o[k] = torch.empty((c['G'], C3), dtype=dt, device=dev)
        own = (*map(L.ptr, c['bn2']), L.ptr(c['W3']), C3)
        ext = (L.ptr(o['ymax']), L.ptr(o['ymin']), L.ptr(o['amax']), L.ptr(o['amin']))
    else:
        own, ext = (None, None, None, None, None, 0), (None, None, None, None)
    L.call('mvp_sa_train_forward_f32', c['zf'], stage, *level_args(c), *own, L.ptr(stat), 1e-5, 0.1, L.ptr(o['mean']), L.ptr(o['invstd']), None, None,
           None, *ext, prec=(6, 3), y2=L.ptr(y2))
    assert int(stat[2 * C:].view(torch.int64)[0]) == 0   # the completion counter is zero again
    return o


def backward(c, layer, bwd, y2, G=None):
    """-> dict(dZ, dW, stat_prev[, tsum]) of the backward pass of `layer` with fixed inputs; y2: the stored y_2 or None (re-compute)."""
    from mvpnet_amd import _lib as L
    B, N, M, C1, C2, C3 = c['dims']
    dev = c['zf'].device
    C, Cp = (C3, C2) if layer == 3 else (C2, C1)
    g = torch.Generator(device='cpu').manual_seed(layer + C)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    stat_i = (rnd(2 * C).double() * c['R'] * 0.01).to(dev)
    gamma_i = (torch.rand(C, generator=g) + 0.5).to(dev)
    o = dict(dZ=torch.full((c['R'], Cp), float('nan'), device=dev), dW=torch.zeros(C, Cp, device=dev),
             stat_prev=torch.zeros(2 * Cp, dtype=torch.float64, device=dev))
    if layer == 3:
        mean_i, invstd_i = c['stage3']['mean'], c['stage3']['invstd']
        dout, pout = rnd(c['G'], C3).to(dev), rnd(c['G'], C3).to(dev)
        parg = torch.randint(0, K, (c['G'], C3), generator=g, dtype=torch.uint8).to(dev)
        own = (L.ptr(c['W3']), C3)
        src = (None, L.ptr(dout), L.ptr(pout), L.ptr(parg))
        tsum = None
    else:
        mean_i, invstd_i = c['bn2'][0], c['bn2'][1]
        own = (None, 0)
        src = (L.ptr(G), None, None, None)
        tsum = o['tsum'] = torch.zeros(16, C1, 4, device=dev)
    L.call('mvp_sa_train_backward_f32', c['zf'], layer, *level_args(c), *map(L.ptr, c['bn2']), *own, L.ptr(mean_i), L.ptr(invstd_i), L.ptr(gamma_i),
           L.ptr(stat_i), None, None, 1, *src, L.ptr(o['dW']), Cp, L.ptr(o['dZ']), L.ptr(o['stat_prev']), L.ptr(tsum),
           prec=(6, L.MLP_PRECISIONS[bwd]), y2=L.ptr(y2))
    torch.cuda.synchronize()
    return o


def summed_close(a, b, what):
    """Outputs the workgroups sum with atomics: the convention of tests/test_ops_gpu.py."""
    np.testing.assert_allclose(a.double().cpu().numpy(), b.double().cpu().numpy(), rtol=1e-4, atol=1e-5 * float(b.abs().max()), err_msg=what)


@pytest.mark.parametrize('name', sorted(CASES))
def test_stored_y2_is_the_level_s_second_layer(dev, name):
    """What stage 2 stores is y_2 = relu(bn_1(y_1)) . W_2^T of every row, empty slots (an all-zero y_1 row) included: against float64 torch.
    Bound: the 3-piece split keeps each operand to 2^-24 relative and the products accumulate in fp32 over <= 64 terms, so the
    contraction is within 2 * 64 * 2^-24 < 2^-17 of sum_k |a_1k| |w_k|; the fp32 y_1 and BatchNorm arithmetic in front of it (a few ulp of
    values of the same size, scaled by invstd * gamma <= 2.25) get the same again: 2^-16 * sum_k |a_1k| |w_k|, + 1e-6 absolute for rows
    whose a_1 is all zero.  Storing does not change the statistics: the same mean / invstd as a stage 2 that stores nothing (rtol 1e-6)."""
    c = level(name)
    B, N, M, C1, C2, C3 = c['dims']
    hi = torch.float64
    idx = c['index']
    ok = (idx >= 0).unsqueeze(-1)
    j = idx.clamp(min=0)
    gat = lambda t: torch.gather(t.to(hi).unsqueeze(1).expand(B, M, N, t.size(-1)), 2, j.unsqueeze(-1).expand(B, M, K, t.size(-1)))
    d = gat(c['xyz']) - c['centre'].to(hi).unsqueeze(2)
    y1 = torch.where(ok, gat(c['zf']) + d @ c['wxyz'].to(hi).t(), torch.zeros((), dtype=hi, device=dev))
    m, i, g, b = (t.to(hi) for t in c['bn1'])
    a1 = torch.relu((y1 - m) * i * g + b).reshape(-1, C1)
    ref = a1 @ c['W2'].to(hi).t()
    bound = 2.0 ** -16 * (a1.abs() @ c['W2'].to(hi).abs().t()) + 1e-6
    err = (c['Y2'].to(hi) - ref).abs()
    print('{}: largest |Y2 - float64| / bound = {:.3f}'.format(name, float((err / bound).max())))
    assert not bool(torch.isnan(c['Y2']).any())
    assert bool((err <= bound).all()), float((err / bound).max())
    plain = forward(c, 2, None)
    for k in ('mean', 'invstd'):
        np.testing.assert_allclose(c['stage2'][k].cpu().numpy(), plain[k].cpu().numpy(), rtol=1e-6, err_msg=k)


@pytest.mark.parametrize('name', sorted(CASES))
def test_stage_3_from_the_stored_y2(dev, name):
    """Forward pass 3 reading the stored y_2 against forward pass 3 re-creating it: the per-ball extremes and their rows bit for bit, the
    finalized BatchNorm to rtol 1e-6 (fp64 sums whose order is free)."""
    c = level(name)
    ref, got = c['stage3'], forward(c, 3, c['Y2'])
    torch.cuda.synchronize()
    for k in ('ymax', 'ymin', 'amax', 'amin'):
        assert torch.equal(got[k], ref[k]), k
    for k in ('mean', 'invstd'):
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k].cpu().numpy(), rtol=1e-6, err_msg=k)


@pytest.mark.parametrize('bwd', ['bf16x3', 'bf16x6'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_backward_passes_from_the_stored_y2(dev, name, bwd):
    """The layer-3 and the layer-2 backward reading the stored y_2 against the same passes re-creating it: dz_2 / dz_1 bit for bit; the weight
    gradients, the column sums for the previous BatchNorm and the coordinate-column operand (atomics over the workgroups) to the convention
    for summed outputs."""
    c = level(name)
    ref3, got3 = backward(c, 3, bwd, None), backward(c, 3, bwd, c['Y2'])
    assert not bool(torch.isnan(ref3['dZ']).any())
    assert torch.equal(got3['dZ'], ref3['dZ'])
    for k in ('dW', 'stat_prev'):
        summed_close(got3[k], ref3[k], 'layer 3 ' + k)
    ref2, got2 = backward(c, 2, bwd, None, G=ref3['dZ']), backward(c, 2, bwd, c['Y2'], G=ref3['dZ'])
    assert not bool(torch.isnan(ref2['dZ']).any())
    assert torch.equal(got2['dZ'], ref2['dZ'])
    for k in ('dW', 'stat_prev'):
        summed_close(got2[k], ref2[k], 'layer 2 ' + k)
    summed_close(got2['tsum'].sum(0), ref2['tsum'].sum(0), 'layer 2 tsum')   # (16 slots by workgroup: their sum is the operand)


def test_a_misaligned_y2_is_refused(dev):
    """MVP_EUNSUPPORTED (before any launch) for a Y2 that is not 16-byte aligned."""
    from mvpnet_amd import _lib as L
    c = level('level1')
    with pytest.raises(RuntimeError, match='code -2'):
        forward(c, 3, c['Y2'].view(-1)[1:])

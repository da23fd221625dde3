"""Operand isolation of the libmvp_hip.so entry points (run with -m gpu on an MI355X): every case runs an entry point TWICE through the
C ABI -- on operands carved from a poisoned arena (tests/arena.py: guard bands, NaN pad columns, odd float64 offsets, scratch sized
exactly by its size function) and on separate, exactly sized, zero-padded allocations -- and asserts that both calls succeed, that no
guard, pad or input changed, that every result element was written and is finite, and that the two results are EQUAL (bit for bit
where no floating-point atomic lies between input and result, else within the tolerance of the entry point's existing test, named at
each use).  The shared-MLP contractions (family A) are also held to their float64 formula with the tolerances of
test_ops_gpu.py::test_mlp_kernels_vs_torch / test_mlp_layer_backward_fused / test_mlp_layer_backward_wide / test_mlp_input_grad_wide /
test_weight_gradient_with_the_finish_on_load.

A case is (id, builder, arguments): the builder declares the operands on the arena and returns the call and what to compare.  Shapes
are the smallest at which the addressing can still go wrong: one row, one full row tile plus a ragged tail, a K tail, every leading
dimension wider than its matrix, and the row count of every routing threshold plus a ragged tail."""
import os

import numpy as np
import pytest
import torch

from tests.arena import Arena

pytestmark = pytest.mark.gpu
HI = torch.float64
PREC = {'mixed': ('bf16x6', 'bf16x3'), 'fp32': ('fp32', None), 'bf16x3': ('bf16x3', 'bf16x3'), 'bf16x6': ('bf16x6', 'bf16x6'), 'bf16': ('bf16', 'bf16')}
LOOSE = {'fp32': 1.0, 'bf16x6': 1.0, 'bf16x3': 16.0, 'bf16': 4096.0}  # test_mlp_kernels_vs_torch
SEED = 987654321012345


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mvpnet_amd import _lib
    _lib.lib()  # fail loudly if libmvp_hip.so is missing
    return torch.device('cuda:0')


def L():
    from mvpnet_amd import _lib
    return _lib


def ptr(t):
    return None if t is None else t.data_ptr()


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 17)


def rn(g, *shape):
    return torch.randn(*shape, generator=g)


def ru(g, *shape):
    return torch.rand(*shape, generator=g)


def bn_inputs(a, g, C, tag):
    """mean, invstd, gamma, beta of a BatchNorm as inputs -> (names, float64 values)"""
    vals = [rn(g, C) * 0.3, ru(g, C) + 0.5, ru(g, C) + 0.5, rn(g, C) * 0.2]
    names = [tag + s for s in ('_mean', '_invstd', '_gamma', '_beta')]
    for n, v in zip(names, vals):
        a.inp(n, v)
    return names, [v.to(HI) for v in vals]


def bn_outputs(a, g, C):
    """mean, invstd written; running_mean, running_var, num_batches_tracked updated in place"""
    a.out('mean', (C,)).out('invstd', (C,))
    a.acc('running_mean', rn(g, C)).acc('running_var', ru(g, C) + 0.5).acc('nbt', torch.full((1,), 5, dtype=torch.int64))
    return ['mean', 'invstd', 'running_mean', 'running_var', 'nbt']


def act_f32(x, vals):
    """relu(bn(x)) > 0 as the kernels decide it: float32, one rounding per operation (the ReLU mask is a DECISION: see test_mlp_layer_backward_wide)"""
    m, i, ga, be = (v.float() for v in vals)
    return (((x - m) * i) * ga + be) > 0


def close(got, want, rtol, atol, what):
    np.testing.assert_allclose(got.double().cpu().numpy(), want.double().cpu().numpy(), rtol=rtol, atol=atol, err_msg=what)


# tolerances of the existing tests for results that a floating-point atomic reaches
STAT_FWD = (1e-6, 1e-4)     # test_mlp_kernels_vs_torch: stat of mvp_mlp_forward_f32 (fp64 atomics without `partial`)
BN_FIN = (2e-6, 1e-7)       # test_mlp_forward_with_bn_finalize: mean / invstd / running statistics from such sums
COLSTAT = (1e-6, 1e-3)      # test_column_statistics_scratch_variant: fp64-atomic column sums against the scratch variant


def run_case(dev, prec, build, kw):
    """build(a, **kw) -> dict(call=f(t), exact=[names], close={name: (rtol, atol) or f(got, want, name)}, post=f(a) or None)"""
    lib = L()
    a = Arena(dev)
    case = build(a, **kw)
    a.build()
    assert sum(f.numel() * f.element_size() for f in a.flat.values()) < 50e6  # (+ the snapshot: well under 100 MB)
    fwd, bwd = PREC[prec] if prec else (None, None)
    # (the reproducible mode would re-route the weight-gradient calls; the A/B switches below change the routes the cases name)
    assert not lib.DW_WORKSPACE and not any(os.environ.get(k) for k in ('MVP_STREAM_TAIL', 'MVP_CSR_LDS', 'MVP_DW_WORKGROUPS', 'MVP_DW_WIDE_MIN_ROWS'))
    with lib.mlp_precision(fwd, bwd):
        case['call'](a)  # (_lib.call raises on a non-zero return code, MVP_EUNSUPPORTED included)
        torch.cuda.synchronize()
        # A finding ENDS the case here: the arena's guards hold a stray access, the exactly sized clean operands below have nothing
        # around them, and a kernel that has just been shown to leave its operands is not launched where that lands in foreign memory.
        found = a.check()
        assert found == [], '\n'.join(found)
        c = a.clean()
        case['call'](c)
        torch.cuda.synchronize()
    for name in case.get('exact', ()):
        got, want = a.result(name), c.result(name)
        assert torch.equal(got, want), '{}: arena and clean operands differ, first at flat index {}'.format(
            name, int(torch.nonzero((got != want).reshape(-1))[0]))
    for name, tol in case.get('close', {}).items():
        if callable(tol):
            tol(a.result(name), c.result(name), name)
        else:
            close(a.result(name), c.result(name), tol[0], tol[1], name)
    if case.get('post'):
        case['post'](a)


# =====================================================================================================================================
# A. shared-MLP contractions
# =====================================================================================================================================
def stream_route_on():
    lib = L().lib()
    old = lib.mvp_set_mlp_stream(1)
    lib.mvp_set_mlp_stream(old)
    return old == 1


def forward(a, R, Cin, ldx, ldw, Cout, kind, act, partial, prec, stream=False):
    """mvp_mlp_forward_f32 (kind 'plain': bias, stat a running sum), _bn_f32 ('bn') and _rel_bn_f32 ('rel', 'rel-inference')"""
    lib = L()
    g = gen(R, Cin, Cout)
    x, w = rn(g, R, Cin), rn(g, Cout, Cin) * 0.2
    a.inp('X', x, ld=ldx).inp('W', w, ld=ldw)
    actn, actv = bn_inputs(a, g, Cin, 'act') if act else ([None] * 4, None)
    xin = x.to(HI)
    if act:
        xin = torch.relu(((xin - actv[0]) * actv[1]) * actv[2] + actv[3])
    ref = xin @ w.to(HI).t()
    pn = 'partial' if partial else None
    if partial:
        a.scratch('partial', ((R + 127) // 128) * 2 * Cout)  # include/mvp_hip.h: ceil(R/128) * 2 * (output columns) float64
    if stream:  # the persistent streaming kernel (mlp_stream.hip).  The conditions restate the library's, so they cannot notice a changed
        # threshold; what can is `partial`: the streaming kernel adds its sums to `stat` itself and leaves the slots untouched, the
        # per-tile kernel fills one slot per row tile (post() below looks at it -- the C ABI has no recorder of the kernel that ran)
        assert R >= 32768 and max(Cin, Cout) <= 128 and Cin % 4 == 0 and Cout % 4 == 0 and ldx % 4 == 0 and partial and prec != 'fp32'
        assert stream_route_on()
    # the sums are bit-reproducible when ONE workgroup adds each of them: through `partial` with at most 128 partial rows (stats_reduce.h)
    ordered = partial and not stream and (R + 127) // 128 <= 128
    a.out('Y', (R, Cout))
    out = dict(exact=['Y'], close={})
    if kind == 'plain':
        bias, stat0 = rn(g, Cout), rn(g, 2 * Cout).to(HI) * 3.0
        ref = ref + bias.to(HI)
        a.inp('bias', bias).acc('stat', stat0)  # accumulated into: a running sum
        out['call'] = lambda t: lib.call('mvp_mlp_forward_f32', t['X'], ptr(t['X']), R, Cin, ldx, ptr(t['W']), ldw, Cout, *[ptr(t[n]) for n in actn],
                                         ptr(t['bias']), ptr(t['Y']), ptr(t['stat']), ptr(t[pn]))
    else:
        if kind.startswith('rel'):
            rel, wrel = rn(g, R, 4) * 0.3, rn(g, Cout, 4) * 0.2
            a.inp('rel', rel).inp('wrel', wrel)
            ref = ref + rel.to(HI) @ wrel.to(HI).t()
        infer = kind == 'rel-inference'
        if not infer:
            stat0 = torch.zeros(2 * Cout + 1, dtype=HI)  # "ALL zero on entry": sums + the launch's completion counter
            a.acc('stat', stat0)
            fin = bn_outputs(a, g, Cout)
        sn, fn = (None, [None] * 5) if infer else ('stat', fin)
        if kind == 'bn':
            out['call'] = lambda t: lib.call('mvp_mlp_forward_bn_f32', t['X'], ptr(t['X']), R, Cin, ldx, ptr(t['W']), ldw, Cout, *[ptr(t[n]) for n in actn],
                                             ptr(t['Y']), ptr(t['stat']), ptr(t[pn]), 1e-5, 0.1, *[ptr(t[n]) for n in fin])
        else:
            out['call'] = lambda t: lib.call('mvp_mlp_forward_rel_bn_f32', t['X'], ptr(t['X']), R, Cin, ldx, ptr(t['W']), ldw, Cout, ptr(t['rel']),
                                             ptr(t['wrel']), ptr(t['Y']), ptr(t[sn]), ptr(t[pn]), 1e-5, 0.1, *[ptr(t[n]) for n in fn])
        if not infer and ordered:
            out['exact'] += fin
        elif not infer:
            out['close'].update({n: BN_FIN for n in fin[:4]})
            out['exact'].append('nbt')
    if kind != 'rel-inference':
        if ordered:
            out['exact'].append('stat')
        else:
            out['close']['stat'] = STAT_FWD
    loose = LOOSE[prec]

    def post(a):  # float64 reference: tolerances of test_mlp_kernels_vs_torch
        y = a.result('Y')
        if partial:   # which kernel ran: see `stream` above
            assert bool(torch.isnan(a.result('partial')).all()) == bool(stream), 'the streaming route was {}taken'.format('' if not stream else 'not ')
        close(y, ref, 1e-5 * loose, 2e-5 * max(1.0, float(ref.abs().max())) * loose, 'Y vs float64')
        if kind != 'rel-inference':
            st = a.result('stat').cpu() - stat0
            close(st[:Cout], y.double().sum(0), 1e-6, 1e-4, 'stat: column sums of y')
            close(st[Cout:2 * Cout], (y.double() ** 2).sum(0), 1e-6, 1e-4, 'stat: column sums of y^2')
            if kind != 'plain':
                assert float(st[2 * Cout]) == 0.0 and int(a.result('nbt')) == 6  # the counter is zero again
    out['post'] = post
    return out


FWD_SHAPES = [(1, 128, 132, 132, 512), (129, 68, 72, 72, 20), (77, 131, 132, 132, 128), (64, 3, 4, 4, 32)]
CASES = []
for _p in ('fp32', 'bf16x3'):
    for _s in FWD_SHAPES + [(32768 + 37, 64, 68, 68, 128)]:
        for _kind, _act, _part in (('plain', False, False), ('plain', True, True), ('bn', False, True), ('bn', True, False)):
            # (the streaming kernel takes ldx > Cin, so ONE shape reaches it -- with `partial`, split-bf16 -- and, without, the per-tile kernel)
            _stream = _s[0] > 32768 and _part and _p != 'fp32'
            CASES.append(('A-forward-{}{}{}-{}x{}x{}-{}'.format(_kind, '-act' if _act else '', '-partial' if _part else '', _s[0], _s[1], _s[4], _p), _p, forward,
                          dict(R=_s[0], Cin=_s[1], ldx=_s[2], ldw=_s[3], Cout=_s[4], kind=_kind, act=_act, partial=_part, prec=_p, stream=_stream)))
    # _rel_bn needs multiples of 4 and 16-byte rows: ldw = Cin + 4 relation columns + 4 pad
    for _kind, _part in (('rel', True), ('rel', False), ('rel-inference', False)):
        CASES.append(('A-forward-{}{}-129x68x36-{}'.format(_kind, '-partial' if _part else '', _p), _p, forward,
                      dict(R=129, Cin=68, ldx=72, ldw=76, Cout=36, kind=_kind, act=False, partial=_part, prec=_p)))


def input_grad(a, R, Cout, Cin, kind, partial, prec):
    """mvp_mlp_input_grad_f32 ('plain', 'mask': ReLU mask + BatchNorm-backward sums in the epilogue) and _dropout_f32 ('dropout')"""
    lib = L()
    g = gen(R, Cout, Cin, 3)
    dy, w = rn(g, R, Cout), rn(g, Cout, Cin) * 0.2
    a.inp('dY', dy).inp('W', w)
    refx = dy.to(HI) @ w.to(HI)
    a.out('dZ', (R, Cin))
    out = dict(exact=['dZ'], close={})
    loose = LOOSE[prec]
    if kind == 'plain':
        out['call'] = lambda t: lib.call('mvp_mlp_input_grad_f32', t['dY'], ptr(t['dY']), R, Cout, ptr(t['W']), Cin, None, None, None, None, None, ptr(t['dZ']), None, None)
        out['post'] = lambda a: close(a.result('dZ'), refx, 1e-5 * loose, 2e-5 * max(1.0, float(refx.abs().max())) * loose, 'dZ vs float64')
        return out
    yprev = rn(g, R, Cin)
    a.inp('y_prev', yprev)
    bn, bnv = bn_inputs(a, g, Cin, 'bn')
    stat0 = rn(g, 2 * Cin).to(HI) * 3.0
    a.acc('stat', stat0)
    pn = 'partial' if partial else None
    if partial:
        a.scratch('partial', ((R + 127) // 128) * 2 * Cin)
    if partial and (R + 127) // 128 <= 128:
        out['exact'].append('stat')
    else:
        out['close']['stat'] = (1e-5 * loose, 1e-3 * loose)  # test_mlp_kernels_vs_torch: the sums of the epilogue (R <= 5000)
    if kind == 'mask':
        out['call'] = lambda t: lib.call('mvp_mlp_input_grad_f32', t['dY'], ptr(t['dY']), R, Cout, ptr(t['W']), Cin, ptr(t['y_prev']), *[ptr(t[n]) for n in bn],
                                         ptr(t['dZ']), ptr(t['stat']), ptr(t[pn]))
    else:
        out['call'] = lambda t: lib.call('mvp_mlp_input_grad_dropout_f32', t['dY'], ptr(t['dY']), R, Cout, ptr(t['W']), Cin, ptr(t['y_prev']), *[ptr(t[n]) for n in bn],
                                         0.25, SEED, ptr(t['dZ']), ptr(t['stat']), ptr(t[pn]))
    on = act_f32(yprev, bnv)
    refz = torch.where(on, refx, torch.zeros_like(refx))
    xh = ((yprev - bnv[0].float()) * bnv[1].float()).to(HI)

    def post(a):
        dz = a.result('dZ').cpu()
        tol = (1e-5 * loose, 2e-5 * max(1.0, float(refx.abs().max())) * loose)
        if kind == 'mask':
            close(dz, refz, *tol, 'dZ vs float64')
        else:  # the keep mask is the library's own hash: every element is 0 or the masked gradient / (1 - p), about 3 in 4 of them kept
            kept = dz != 0
            close(torch.where(kept, dz.to(HI), refz / 0.75), refz / 0.75, *tol, 'dZ vs float64 on the kept elements')
            if R * Cin >= 4096:
                assert abs(float(kept.sum()) / max(1.0, float((refz != 0).sum())) - 0.75) < 0.08
        st = a.result('stat').cpu() - stat0
        close(st[:Cin], dz.double().sum(0), 1e-5 * loose, 1e-3 * loose, 'stat: sum dZ')
        close(st[Cin:], (dz.double() * xh).sum(0), 1e-5 * loose, 1e-3 * loose, 'stat: sum dZ * xhat')
    out['post'] = post
    return out


for _p in ('fp32', 'bf16x3'):
    for _s in ((1, 512, 128), (129, 20, 68), (300, 256, 259)):  # (Cin = 259 is accepted: no replacement by 260)
        for _kind, _part in (('plain', False), ('mask', True), ('mask', False), ('dropout', True)):
            CASES.append(('A-input_grad-{}{}-{}x{}x{}-{}'.format(_kind, '-partial' if _part else '', *_s, _p), _p, input_grad,
                          dict(R=_s[0], Cout=_s[1], Cin=_s[2], kind=_kind, partial=_part, prec=_p)))


def weight_grad(a, R, Cout, Cin, ldx, lddw, act, ws, prec, route=None):
    """mvp_mlp_weight_grad_f32 / _ws_f32: dW (Cout, lddw)[:, :Cin] += dY^T . act(X), dW a running sum inside a wider gradient"""
    lib = L()
    g = gen(R, Cout, Cin, 5)
    dy, x = rn(g, R, Cout), rn(g, R, Cin)
    a.inp('dY', dy).inp('X', x, ld=ldx)
    actn, actv = bn_inputs(a, g, Cin, 'act') if act else ([None] * 4, None)
    dw0 = rn(g, Cout, Cin)
    a.acc('dW', dw0, ld=lddw)
    nws = int(lib.lib().mvp_mlp_weight_grad_workspace_floats())
    if ws:
        a.scratch('workspace', nws, dtype=torch.float32)
    if route == 'lds-tile':   # mlp_bwd_wide.hip, the DWO instances: multiples of 128 on both sides, >= 16384 rows, split-bf16, no workspace.
        # (The library's conditions restated: nothing at the C ABI tells this kernel from mlp_dw_bf_kernel, so a changed MVP_DW_WIDE_MIN_ROWS
        # default would fall back unnoticed here.)
        assert R >= 16384 and Cout % 128 == 0 and Cin % 128 == 0 and ldx % 4 == 0 and prec != 'fp32' and not ws
    if route == 'row-split':  # more than one row split of at least 256 rows (weight_grad_impl): the partial tiles meet in dW or in the workspace;
        assert R > 256        # with the workspace post() sees that the split happened: only then is the workspace written
    xin = x.to(HI)
    if act:
        xin = torch.relu(((xin - actv[0]) * actv[1]) * actv[2] + actv[3])
    ref = dw0.to(HI) + dy.to(HI).t() @ xin
    loose = LOOSE[prec]
    name = 'mvp_mlp_weight_grad_ws_f32' if ws else 'mvp_mlp_weight_grad_f32'
    tail = (lambda t: (ptr(t['workspace']), nws)) if ws else (lambda t: ())
    out = dict(call=lambda t: lib.call(name, t['dY'], ptr(t['dY']), ptr(t['X']), R, Cout, Cin, ldx, *[ptr(t[n]) for n in actn], ptr(t['dW']), lddw, *tail(t)))
    # one row split (at least 128 rows per block on the fp32 kernel, 256 on the split-bf16 one) adds once per element; several meet through
    # fp32 atomics unless the workspace orders them
    single = R <= 128 or (R <= 256 and prec != 'fp32' and Cin >= 8)
    if single or ws:
        out['exact'] = ['dW']
    else:   # test_mlp_kernels_vs_torch: dW against float64 (the order of the fp32 atomics is all that differs between two runs)
        out['close'] = {'dW': (1e-4 * loose, 2e-5 * max(1.0, float(ref.abs().max())) * loose)}
    def post(a):
        if ws:   # one split: the kernel adds to dW itself and must leave the workspace alone; several: partial tiles + dw_reduce_kernel
            assert bool(torch.isnan(a.result('workspace')).all()) == (route != 'row-split'), 'workspace route'
        close(a.result('dW'), ref, 1e-4 * loose, 2e-5 * max(1.0, float(ref.abs().max())) * loose, 'dW vs float64')
    out['post'] = post
    return out


for _p in ('fp32', 'bf16x3'):
    for _s in FWD_SHAPES:  # (R, Cin, ldx, -, Cout) of the forward, lddw > Cin
        for _act, _ws in ((False, False), (True, True)):
            # (one row split at these row counts: a workspace that is handed over is NOT used and must stay untouched)
            CASES.append(('A-weight_grad{}{}-{}x{}x{}-{}'.format('-act' if _act else '', '-ws_unused' if _ws else '', _s[0], _s[4], _s[1], _p), _p, weight_grad,
                          dict(R=_s[0], Cout=_s[4], Cin=_s[1], ldx=_s[2], lddw=_s[1] + 5, act=_act, ws=_ws, prec=_p)))
    # 70001 rows cut to the smallest that still splits the rows: 4 x 5 tiles of 64 x 64 -> 52 splits asked for, at least 256 rows each -> 257 rows = 2 splits
    for _ws in (False, True):
        CASES.append(('A-weight_grad-rowsplit{}-257x256x260-{}'.format('-ws' if _ws else '', _p), _p, weight_grad,
                      dict(R=257, Cout=256, Cin=260, ldx=260, lddw=264, act=True, ws=_ws, prec=_p, route='row-split')))
CASES.append(('A-weight_grad-ldstile-16500x128x128-bf16x3', 'bf16x3', weight_grad,
              dict(R=16500, Cout=128, Cin=128, ldx=132, lddw=132, act=True, ws=False, prec='bf16x3', route='lds-tile')))
CASES.append(('A-weight_grad-ldstile-16500x128x128-bf16', 'bf16', weight_grad,
              dict(R=16500, Cout=128, Cin=128, ldx=132, lddw=132, act=False, ws=False, prec='bf16', route='lds-tile')))


def layer_backward(a, R, C, Cp, ldx, lddw, finish, act, want_dz, ws, prec, entry='fused', mode=None, drop_p=0.0, ticket=False, pool_k=1, ldw=None, pooled=False):
    """mvp_mlp_layer_backward_f32 / _ws_f32 (entry 'fused': Yi given = finish) and mvp_mlp_layer_backward_wide[_pooled]_p_f32 ('wide': modes 0, 1, 2)"""
    lib = L()
    ldw = ldw or Cp
    g = gen(R, C, Cp, 7)
    wide = entry == 'wide'
    mode = mode if wide else (1 if finish else 0)
    Rg = R // pool_k
    w, x, gsrc, yi = rn(g, C, Cp) * 0.2, rn(g, R, Cp), rn(g, Rg, C), rn(g, R, C) * 1.5 + 0.2
    a.inp('X', x, ld=ldx).inp('W', w, ld=ldw)
    pool = [None] * 3
    if pooled:   # the POOL front end of the fused kernel: G and Yi are NULL, y_i is re-computed from X, dz_i = pool_dout at the arg-max row where pool_out > 0
        assert not wide and mode == 1 and act and R % 32 == 0 and max(C, Cp) <= 64
        pool = ['pool_dout', 'pool_out', 'pool_arg']
        pdout, pout, parg = rn(g, R // 32, C), rn(g, R // 32, C), torch.randint(0, 32, (R // 32, C), generator=g)
        a.inp('pool_dout', pdout).inp('pool_out', pout).inp('pool_arg', parg.to(torch.uint8), fill=0)
    else:
        a.inp('G', gsrc)
    bi, biv = (None,) * 4, None
    if mode and not pooled:
        a.inp('Yi', yi)
    if mode:
        bi, biv = bn_inputs(a, g, C, 'bn_i')
        stat_i = rn(g, 2 * C).to(HI) * R * 0.01
        a.inp('stat_i', stat_i)
        a.out('dgamma', (C,)).out('dbeta', (C,))
    actn, actv = bn_inputs(a, g, Cp, 'act') if act else ([None] * 4, None)
    dw0 = rn(g, C, Cp)
    a.acc('dW', dw0, ld=lddw)
    if want_dz:
        a.out('dZ', (R, Cp))
    stats_prev = act and want_dz
    if stats_prev:
        sp0 = rn(g, 2 * Cp).to(HI) * 3.0
        a.acc('stat_prev', sp0)
        if not wide:
            a.scratch('partial', int(lib.lib().mvp_mlp_layer_backward_partial_count(R, Cp)))
    nws = int(lib.lib().mvp_mlp_weight_grad_workspace_floats())
    if ws:
        a.scratch('workspace', nws, dtype=torch.float32)
    if ticket:
        a.acc('ticket', torch.zeros(1, dtype=torch.int32))  # one zeroed int32 of caller memory
    opt = lambda t, n, have: ptr(t[n]) if have else None
    if wide:
        p = (lib.MLP_PRECISIONS[PREC[prec][0]], lib.MLP_PRECISIONS[PREC[prec][1]])
        head = lambda t: (ptr(t['G']), opt(t, 'Yi', mode), opt(t, bi[0], mode), opt(t, bi[1], mode), opt(t, bi[2], mode), opt(t, bi[3], mode == 2),
                          opt(t, 'stat_i', mode), opt(t, 'dgamma', mode), opt(t, 'dbeta', mode), 1, mode)
        mid = lambda t: (drop_p, SEED, ptr(t['X']), ldx, *[ptr(t[n]) for n in actn], ptr(t['W']), ldw, R, C, Cp, ptr(t['dW']), lddw, ptr(t['dZ']),
                         opt(t, 'stat_prev', stats_prev), opt(t, 'ticket', ticket), opt(t, 'workspace', ws), nws if ws else 0)
        if pool_k > 1:
            call = lambda t: lib.call('mvp_mlp_layer_backward_wide_pooled_p_f32', t['G'], *head(t), pool_k, *mid(t), *p)
        else:
            call = lambda t: lib.call('mvp_mlp_layer_backward_wide_p_f32', t['G'], *head(t), *mid(t), *p)
    else:
        name = 'mvp_mlp_layer_backward_ws_f32' if ws else 'mvp_mlp_layer_backward_f32'
        tail = (lambda t: (ptr(t['workspace']), nws)) if ws else (lambda t: ())
        call = lambda t: lib.call(name, t['X'], opt(t, 'G', not pooled), opt(t, 'Yi', mode and not pooled), opt(t, bi[0], mode), opt(t, bi[1], mode), opt(t, bi[2], mode),
                                  opt(t, 'stat_i', mode), opt(t, 'dgamma', mode), opt(t, 'dbeta', mode), 1, ptr(t['X']), ldx, *[ptr(t[n]) for n in actn],
                                  ptr(t['W']), ldw, R, C, Cp, ptr(t['dW']), lddw, opt(t, 'dZ', want_dz), opt(t, 'stat_prev', stats_prev),
                                  opt(t, 'partial', stats_prev), *[ptr(t[n]) for n in pool], *tail(t))
    # float64 (test_mlp_layer_backward_fused / test_mlp_layer_backward_wide)
    dzi = gsrc.to(HI).repeat_interleave(pool_k, 0)
    if pooled:
        yi = torch.relu(((x.to(HI) - actv[0]) * actv[1]) * actv[2] + actv[3]) @ w.to(HI).t()   # (only its xhat is used: no decision hangs on it)
        rows = torch.arange(R // 32).unsqueeze(1) * 32 + parg
        dzi = torch.zeros(R, C, dtype=HI).scatter_(0, rows, torch.where(pout > 0, pdout, torch.zeros_like(pdout)).to(HI))
    if mode == 2:
        dzi = torch.where(act_f32(yi, biv), dzi, torch.zeros_like(dzi))
    if mode:
        xh_i = (yi.to(HI) - biv[0]) * biv[1]
        dyr = (biv[2] * biv[1]) * ((dzi - stat_i[:C] / R) - xh_i * (stat_i[C:] / R))
    else:
        dyr = dzi
    xin = x.to(HI)
    xh = None
    if act:
        xh = (xin - actv[0]) * actv[1]
        xin = torch.relu(xh * actv[2] + actv[3])
    ref_dw = dw0.to(HI) + dyr.t() @ xin
    ref_dz = dyr @ w.to(HI)
    if act:
        ref_dz = torch.where(act_f32(x, actv), ref_dz, torch.zeros_like(ref_dz))
    loose = {'bf16x6': 4.0}.get(prec, LOOSE[prec]) if wide else LOOSE[prec]
    sw, sz = max(1.0, float(ref_dw.abs().max())), max(1.0, float(ref_dz.abs().max()))
    # One workgroup along the rows adds each dW element once; several meet through fp32 atomics, or -- with the workspace, which both entry
    # points use only THEN -- through partial tiles and the ordered dw_reduce_kernel, the launch that stores into dW with lddw.
    # With a ticket and several workgroups the tile order, hence the fp32 sum inside a workgroup, differs from run to run.
    grid = (R + 63) // 64 if wide else fused_backward_grid(R, C, Cp, pooled)   # (wide: min(row tiles, CUs or more))
    single, ws_used = grid == 1, ws and grid > 1
    out = dict(call=call, exact=(['dgamma', 'dbeta'] if mode else []) + (['dZ'] if want_dz else []), close={})
    if single or ws_used:
        out['exact'].append('dW')
    else:  # tolerance of the float64 comparison of test_mlp_layer_backward_fused / _wide
        out['close']['dW'] = (1e-4 * loose, 3e-5 * sw * loose)
    if stats_prev:  # fp64 atomics, one per column and workgroup (both entry points add to stat_prev directly)
        if single:
            out['exact'].append('stat_prev')
        else:
            out['close']['stat_prev'] = (1e-5 * loose, 2e-3 * loose * sz)

    def post(a):
        tag = 'mode={} act={} dz={} drop={}'.format(mode, act, want_dz, drop_p)
        if mode:
            assert torch.equal(a.result('dgamma').cpu(), stat_i[C:].float()) and torch.equal(a.result('dbeta').cpu(), stat_i[:C].float()), tag
        if ticket and R > 64 and not ws:
            assert int(a.result('ticket')) > 0   # tiles beyond each workgroup's first were taken by ticket
        if ws:   # the route the case is named after really ran: the partial tiles are in the workspace -- or it was left alone
            assert bool(torch.isnan(a.result('workspace')).all()) == (not ws_used), 'workspace route (grid = {})'.format(grid)
        if drop_p > 0:   # dz_i carries the library's own keep mask: covered by the arena / clean comparison and the guards, not by a formula
            return
        close(a.result('dW'), ref_dw, 1e-4 * loose, 3e-5 * sw * loose, 'dW vs float64 ' + tag)
        if want_dz:
            close(a.result('dZ'), ref_dz, 1e-5 * loose, 2e-5 * sz * loose, 'dZ vs float64 ' + tag)
            if stats_prev:
                st = a.result('stat_prev').cpu() - sp0
                close(st[:Cp], ref_dz.sum(0), 1e-5 * loose, 2e-3 * loose * sz, 'stat_prev: sum dZ ' + tag)
                close(st[Cp:], (ref_dz * xh).sum(0), 1e-5 * loose, 2e-3 * loose * sz, 'stat_prev: sum dZ * xhat ' + tag)
    out['post'] = post
    return out


def fused_backward_grid(R, C, Cp, pooled):
    """workgroups along the rows of mlp_bwd_layer_kernel, as layer_backward_impl (mlp_bwd.hip) sizes them: the workspace route needs more than one"""
    cdiv = lambda a, b: -(-a // b)
    ntiles = cdiv(R, 32)
    cb = 1 if C <= 32 else 2 if C <= 64 else 4
    cpb = 1 if Cp <= 32 else 2 if (Cp <= 64 or Cp > 96 or cb == 4) else 3
    wgs = max(1, min(1024, cdiv(ntiles, 8)))
    if cb == 4:
        wgs = max(1, min(256 // (1 if pooled else cdiv(Cp, 32 * cpb)), cdiv(ntiles, 4)))
    return cdiv(ntiles, cdiv(cdiv(ntiles, wgs), 4) * 4)


# split-bf16 only (fp32 is refused by both entry points); bf16x6 on the fused kernel is the same loads and stores with one more piece.
# At 129 rows and fewer ONE workgroup walks the rows: a workspace that is handed over is not used and must stay untouched ('-ws_unused').
for _s in ((129, 36, 68, 72, 72), (1, 128, 128, 128, 128), (129, 20, 32, 32, 36)):
    for _fin, _act, _dz, _ws in ((False, False, False, False), (True, True, True, False), (False, True, True, True), (True, False, True, True)):
        CASES.append(('A-layer_backward{}{}{}{}-{}x{}x{}-bf16x3'.format('-finish' if _fin else '', '-act' if _act else '', '-dz' if _dz else '', '-ws_unused' if _ws else '', *_s[:3]),
                      'bf16x3', layer_backward, dict(R=_s[0], C=_s[1], Cp=_s[2], ldx=_s[3], lddw=_s[4], finish=_fin, act=_act, want_dz=_dz, ws=_ws, prec='bf16x3')))
# The row count from which the rows are split over workgroups, plus a ragged tail: 257 rows = 9 tiles of 32 -> 2 workgroups (3 at 128 channels);
# with the workspace: partial tiles + dw_reduce_kernel, without: fp32 atomics
for _s in ((257, 36, 68, 72, 72), (257, 128, 128, 128, 132)):
    assert fused_backward_grid(_s[0], _s[1], _s[2], False) > 1 and fused_backward_grid(256, 36, 68, False) == 1
    for _ws in (True, False):
        CASES.append(('A-layer_backward-finish-act-dz{}-rowsplit-{}x{}x{}-bf16x3'.format('-ws' if _ws else '', *_s[:3]), 'bf16x3', layer_backward,
                      dict(R=_s[0], C=_s[1], Cp=_s[2], ldx=_s[3], lddw=_s[4], finish=True, act=True, want_dz=True, ws=_ws, prec='bf16x3')))
for _dz in (True, False):   # the pooled form: three groups of 32 rows
    CASES.append(('A-layer_backward-pooled{}-96x36x36-bf16x3'.format('-dz' if _dz else ''), 'bf16x3', layer_backward,
                  dict(R=96, C=36, Cp=36, ldx=40, lddw=40, finish=True, act=True, want_dz=_dz, ws=False, prec='bf16x3', pooled=True)))
for _p in ('bf16x3', 'bf16'):
    for _s in ((1, 128, 128, 128, 128), (67, 36, 100, 104, 104), (65, 128, 68, 72, 72)):
        for _mode, _drop, _act, _tk, _ws in ((0, 0.0, False, False, False), (1, 0.0, True, True, False), (2, 0.0, True, False, True), (2, 0.4, True, True, False)):
            CASES.append(('A-layer_backward_wide-mode{}{}{}{}{}-{}x{}x{}-{}'.format(_mode, '-drop' if _drop else '', '-act' if _act else '', '-ticket' if _tk else '',
                                                                                 ('-ws' if _s[0] > 64 else '-ws_unused') if _ws else '', *_s[:3], _p), _p, layer_backward,
                          dict(R=_s[0], C=_s[1], Cp=_s[2], ldx=_s[3], lddw=_s[4], finish=bool(_mode), act=_act, want_dz=True, ws=_ws, prec=_p, entry='wide',
                               mode=_mode, drop_p=_drop, ticket=_tk)))
    # The instances of mlp_bwd_wide_kernel specialised by mode (0, 1, 2, pooled) run only when both widths fill the instance (C = Cp = 128, or 64)
    # behind an activation; everything above with other widths, or mode 0 without activation, runs the generic one.  Modes 1 and 2 at 128 x 128 are
    # above; here mode 0 and the pooled form at 128 x 128, and the 64-channel instance (the only one with three pieces, bf16x6).
    CASES.append(('A-layer_backward_wide-mode0-act-65x128x128-' + _p, _p, layer_backward,
                  dict(R=65, C=128, Cp=128, ldx=132, lddw=132, finish=False, act=True, want_dz=True, ws=False, prec=_p, entry='wide', mode=0)))
    CASES.append(('A-layer_backward_wide_pooled-k5-65x128x128-' + _p, _p, layer_backward,
                  dict(R=65, C=128, Cp=128, ldx=132, lddw=132, finish=True, act=True, want_dz=True, ws=False, prec=_p, entry='wide', mode=2, pool_k=5)))
    # the SUM over pool_k = 5 rows behind the layer: R a multiple of 5 (65 rows: one tile plus a row; 335: several workgroups)
    for _R, _tk in ((65, True), (335, False)):
        CASES.append(('A-layer_backward_wide_pooled-k5{}-{}x128x68-{}'.format('-ticket' if _tk else '', _R, _p), _p, layer_backward,
                      dict(R=_R, C=128, Cp=68, ldx=72, lddw=72, finish=True, act=True, want_dz=True, ws=False, prec=_p, entry='wide', mode=2, ticket=_tk, pool_k=5)))


for _p in ('bf16x3', 'bf16x6'):
    CASES.append(('A-layer_backward_wide-mode1-act-ticket-65x64x64-' + _p, _p, layer_backward,
                  dict(R=65, C=64, Cp=64, ldx=68, lddw=68, finish=True, act=True, want_dz=True, ws=False, prec=_p, entry='wide', mode=1, ticket=True)))


def weight_grad_finish(a, R, Cout, Cin, ldx, lddw, kind, ws, prec):
    """mvp_mlp_weight_grad_finish_p_f32 ('plain'), _rel_p_f32 ('rel': [X | REL (R,4)] in one launch) and _act_p_f32 ('act')"""
    lib = L()
    g = gen(R, Cout, Cin, 11)
    dz, y, x = rn(g, R, Cout), rn(g, R, Cout) * 1.3 + 0.1, rn(g, R, Cin)
    a.inp('dZ', dz).inp('Y', y).inp('X', x, ld=ldx)
    bn, bnv = bn_inputs(a, g, Cout, 'bn')
    xh = (y.to(HI) - bnv[0]) * bnv[1]
    stat = torch.cat([dz.to(HI).sum(0), (dz.to(HI) * xh).sum(0)])
    a.inp('stat', stat)
    dw0 = rn(g, Cout, Cin)
    a.acc('dW', dw0, ld=lddw)
    actn, actv = bn_inputs(a, g, Cin, 'act') if kind == 'act' else ([None] * 4, None)
    nws = int(lib.lib().mvp_mlp_weight_grad_workspace_floats())
    if ws:
        a.scratch('workspace', nws, dtype=torch.float32)
    p = (lib.MLP_PRECISIONS[PREC[prec][0]], lib.MLP_PRECISIONS[PREC[prec][1] or 'bf16x3'])
    head = lambda t: (ptr(t['dZ']), ptr(t['Y']), ptr(t[bn[0]]), ptr(t[bn[1]]), ptr(t[bn[2]]), ptr(t['stat']), 1, ptr(t['X']), R, Cout, Cin, ldx)
    wsa = lambda t: (ptr(t['workspace']), nws) if ws else (None, 0)
    dyr = (bnv[2] * bnv[1]) * ((dz.to(HI) - stat[:Cout] / R) - xh * (stat[Cout:] / R))
    xin = x.to(HI)
    if kind == 'act':
        xin = torch.relu(((xin - actv[0]) * actv[1]) * actv[2] + actv[3])
    ref = dw0.to(HI) + dyr.t() @ xin
    loose = LOOSE[prec]
    tol = (1e-4 * loose, 3e-5 * max(1.0, float(ref.abs().max())) * loose)  # test_weight_gradient_with_the_finish_on_load, against float64
    out = dict(exact=[], close={})
    if kind == 'plain':
        out['call'] = lambda t: lib.call('mvp_mlp_weight_grad_finish_p_f32', t['dZ'], *head(t), ptr(t['dW']), lddw, *wsa(t), *p)
    elif kind == 'act':
        out['call'] = lambda t: lib.call('mvp_mlp_weight_grad_finish_act_p_f32', t['dZ'], *head(t), *[ptr(t[n]) for n in actn], ptr(t['dW']), lddw, *wsa(t), *p)
    else:
        rel, dwr0 = rn(g, R, 4) * 0.3, rn(g, Cout, 4)
        a.inp('REL', rel).acc('dWrel', dwr0, ld=lddw)
        refr = dwr0.to(HI) + dyr.t() @ rel.to(HI)
        out['call'] = lambda t: lib.call('mvp_mlp_weight_grad_finish_rel_p_f32', t['dZ'], *head(t), ptr(t['REL']), ptr(t['dW']), ptr(t['dWrel']), lddw, *p)
    names = ['dW'] + (['dWrel'] if kind == 'rel' else [])
    ws_used = ws and R > 256   # (weight_grad_impl: row splits of at least 256 rows; the workspace is used only when there are several)
    if R <= 256 or ws_used:    # one row split: every element is added once; several through the workspace: in split order
        out['exact'] += names
    else:
        out['close'].update({n: tol for n in names})

    def post(a):
        if ws:   # that the rows really were split shows in the workspace: written only then
            assert bool(torch.isnan(a.result('workspace')).all()) == (not ws_used), 'workspace route'
        close(a.result('dW'), ref, *tol, 'dW vs float64')
        if kind == 'rel':
            close(a.result('dWrel'), refr, *tol, 'dWrel vs float64')
    out['post'] = post
    return out


for _p in ('bf16x3', 'bf16'):
    for _s in ((129, 36, 36, 40, 40), (1, 256, 128, 128, 128)):
        for _kind, _ws in (('plain', False), ('act', True)):
            CASES.append(('A-weight_grad_finish-{}{}-{}x{}x{}-{}'.format(_kind, '-ws_unused' if _ws else '', *_s[:3], _p), _p, weight_grad_finish,
                          dict(R=_s[0], Cout=_s[1], Cin=_s[2], ldx=_s[3], lddw=_s[4], kind=_kind, ws=_ws, prec=_p)))
    for _kind, _ws in (('plain', True), ('act', True), ('act', False)):   # 257 rows: two row splits -- through the workspace, and through fp32 atomics
        CASES.append(('A-weight_grad_finish-{}{}-rowsplit-257x36x36-{}'.format(_kind, '-ws' if _ws else '', _p), _p, weight_grad_finish,
                      dict(R=257, Cout=36, Cin=36, ldx=40, lddw=40, kind=_kind, ws=_ws, prec=_p)))
    CASES.append(('A-weight_grad_finish-rel-129x36x36-' + _p, _p, weight_grad_finish, dict(R=129, Cout=36, Cin=36, ldx=40, lddw=44, kind='rel', ws=False, prec=_p)))
# The fp32 kernel (64 x 32 tiles, 16-byte rows): 32 input columns under the fp32 precision.  Under a split precision weight_grad_impl keeps
# 8 <= Cin <= 32 on the split-bf16 kernel, whose finish form exists for 64-wide tiles only (refused), so that precision runs the nearest
# accepted shape: the four relation columns of FeatureAggregation's first layer (Cin = 4 < 8 stays on the fp32 kernel).
CASES.append(('A-weight_grad_finish-plain-fp32kernel-129x64x32-fp32', 'fp32', weight_grad_finish, dict(R=129, Cout=64, Cin=32, ldx=32, lddw=36, kind='plain', ws=False, prec='fp32')))
CASES.append(('A-weight_grad_finish-plain-fp32kernel-129x64x4-bf16x3', 'bf16x3', weight_grad_finish, dict(R=129, Cout=64, Cin=4, ldx=4, lddw=8, kind='plain', ws=False, prec='bf16x3')))


def input_grad_wide(a, R, C, Cp, ldx, finish, prec):
    """mvp_mlp_input_grad_wide_p_f32: the workspace is exactly mvp_mlp_input_grad_wide_workspace_bytes(C, Cp) bytes"""
    lib = L()
    g = gen(R, C, Cp, 13)
    w, x, gsrc = rn(g, C, Cp) * 0.2, rn(g, R, Cp), rn(g, R, C)
    a.inp('G', gsrc).inp('X', x, ld=ldx).inp('W', w, ld=Cp + 4)
    actn, actv = bn_inputs(a, g, Cp, 'act')
    bi, biv = (None,) * 4, None
    if finish:
        yi = rn(g, R, C) * 1.5 + 0.2
        a.inp('Yi', yi)
        bi, biv = bn_inputs(a, g, C, 'bn_i')
        stat_i = rn(g, 2 * C).to(HI) * R * 0.01
        a.inp('stat_i', stat_i).out('dgamma', (C,)).out('dbeta', (C,))
    sp0 = rn(g, 2 * Cp).to(HI) * 3.0
    a.out('dZ', (R, Cp)).acc('stat_prev', sp0)
    nbytes = int(lib.lib().mvp_mlp_input_grad_wide_workspace_bytes(C, Cp))
    a.scratch('workspace', nbytes, dtype=torch.uint8)
    p = (lib.MLP_PRECISIONS[PREC[prec][0]], lib.MLP_PRECISIONS[PREC[prec][1]])
    opt = lambda t, n: ptr(t[n]) if finish else None
    call = lambda t: lib.call('mvp_mlp_input_grad_wide_p_f32', t['G'], ptr(t['G']), opt(t, 'Yi'), opt(t, bi[0]), opt(t, bi[1]), opt(t, bi[2]), opt(t, 'stat_i'),
                              opt(t, 'dgamma'), opt(t, 'dbeta'), 1, ptr(t['X']), ldx, *[ptr(t[n]) for n in actn], ptr(t['W']), Cp + 4, R, C, Cp, ptr(t['dZ']),
                              ptr(t['stat_prev']), ptr(t['workspace']), nbytes, *p)
    dyr = gsrc.to(HI)
    if finish:
        xh_i = (yi.to(HI) - biv[0]) * biv[1]
        dyr = (biv[2] * biv[1]) * ((dyr - stat_i[:C] / R) - xh_i * (stat_i[C:] / R))
    xh = (x.to(HI) - actv[0]) * actv[1]
    ref_dz = torch.where(act_f32(x, actv), dyr @ w.to(HI), torch.zeros(R, Cp, dtype=HI))
    loose = LOOSE[prec]
    sz = max(1.0, float(ref_dz.abs().max()))
    out = dict(call=call, exact=['dZ'] + (['dgamma', 'dbeta'] if finish else []), close={})
    if R <= 64:   # one 64-row tile: one workgroup per c_in block adds each sum once
        out['exact'].append('stat_prev')
    else:          # test_mlp_input_grad_wide (fp64 atomics, one per column and workgroup)
        out['close']['stat_prev'] = (1e-5 * loose, 2e-3 * loose * sz)

    def post(a):
        if finish:
            assert torch.equal(a.result('dgamma').cpu(), stat_i[C:].float()) and torch.equal(a.result('dbeta').cpu(), stat_i[:C].float())
        close(a.result('dZ'), ref_dz, 1e-5 * loose, 2e-5 * sz * loose, 'dZ vs float64')
        st = a.result('stat_prev').cpu() - sp0
        close(st[:Cp], ref_dz.sum(0), 1e-5 * loose, 2e-3 * loose * sz, 'stat_prev: sum dZ')
        close(st[Cp:], (ref_dz * xh).sum(0), 1e-5 * loose, 2e-3 * loose * sz, 'stat_prev: sum dZ * xhat')
    out['post'] = post
    return out


for _p in ('bf16x3', 'bf16'):   # (one- or two-piece backward split only; the one-piece kernel stages dZ through LDS: its own store path)
    for _s, _fin in (((67, 64, 128, 132), True), ((129, 512, 256, 256), False), ((1, 256, 128, 128), True), ((129, 256, 256, 260), True)):
        # (a pending finish is accepted up to 256 channels: the 512-wide shape runs with dy given, and 129 x 256 x 256 adds the finish at two c_in blocks)
        CASES.append(('A-input_grad_wide{}-{}x{}x{}-{}'.format('-finish' if _fin else '', *_s[:3], _p), _p, input_grad_wide,
                      dict(R=_s[0], C=_s[1], Cp=_s[2], ldx=_s[3], finish=_fin, prec=_p)))


def forward_bf16(a, R, Cin, ldx, Cout, ldy, affine):
    """mvp_mlp_forward_bf16: bfloat16 rows in and out, Y with real pad columns"""
    lib = L()
    g = gen(R, Cin, Cout, 19)
    bf = torch.bfloat16
    x, w = rn(g, R, Cin).to(bf), rn(g, Cout, Cin) * 0.2
    a.inp('X', x, ld=ldx).inp('W', w, ld=Cin + 4).out('Y', (R, Cout), dtype=bf, ld=ldy)
    names = [None] * 3
    prod = x.to(HI) @ w.to(bf).to(HI).t()
    ref = prod
    if affine:
        bias, scale, shift = rn(g, Cout), ru(g, Cout) + 0.5, rn(g, Cout) * 0.3
        a.inp('bias', bias).inp('scale', scale).inp('shift', shift)
        names = ['bias', 'scale', 'shift']
        ref = torch.relu((prod + bias.to(HI)) * scale.to(HI) + shift.to(HI))

    def post(a):  # test_mlp_layer_on_bfloat16_values: within one bf16 unit of the float64 value of the same expression
        err = (a.result('Y').cpu().to(HI) - ref).abs()
        assert bool((err <= ref.abs() * 2.0 ** -8 + 1e-3 * 2.0 ** -8 + 2e-5 * float(prod.abs().max())).all()), float(err.max())
    return dict(call=lambda t: lib.call('mvp_mlp_forward_bf16', t['X'], ptr(t['X']), R, Cin, ldx, ptr(t['W']), Cin + 4, Cout, *[ptr(t[n]) for n in names],
                                        1 if affine else 0, ptr(t['Y']), ldy), exact=['Y'], post=post)


for _s in ((129, 48, 56, 24, 32), (1, 128, 128, 256, 256)):
    for _aff in (False, True):
        CASES.append(('A-forward_bf16{}-{}x{}x{}'.format('-affine' if _aff else '', _s[0], _s[1], _s[3]), None, forward_bf16,
                      dict(R=_s[0], Cin=_s[1], ldx=_s[2], Cout=_s[3], ldy=_s[4], affine=_aff)))


def forward_pool(a, R, Cin, ldx, Cout, prec):
    """mvp_mlp_forward_pool_f32: the streaming kernel in pooled mode (K = 32 rows per group), statistics by fp64 atomics + finalize"""
    lib = L()
    assert R >= 32768 and R % 32 == 0 and max(Cin, Cout) <= 128 and prec != 'fp32'  # its support matrix: the threshold is met
    g = gen(R, Cin, Cout, 23)
    Gn = R // 32
    x, w = rn(g, R, Cin), rn(g, Cout, Cin) * 0.2
    a.inp('X', x, ld=ldx).inp('W', w, ld=Cin + 4)
    actn, actv = bn_inputs(a, g, Cin, 'act')
    a.out('ymax', (Gn, Cout)).out('ymin', (Gn, Cout)).out('amax', (Gn, Cout), dtype=torch.uint8).out('amin', (Gn, Cout), dtype=torch.uint8)
    a.acc('stat', torch.zeros(2 * Cout + 1, dtype=HI))
    a.scratch('partial', ((R + 127) // 128) * 2 * Cout)
    fin = bn_outputs(a, g, Cout)
    y = torch.relu(((x.to(HI) - actv[0]) * actv[1]) * actv[2] + actv[3]) @ w.to(HI).t()
    yg = y.reshape(Gn, 32, Cout)
    loose = LOOSE[prec]

    def post(a):
        tol = (1e-5 * loose, 2e-5 * max(1.0, float(y.abs().max())) * loose)  # test_mlp_kernels_vs_torch
        close(a.result('ymax'), yg.max(1)[0], *tol, 'ymax vs float64')
        close(a.result('ymin'), yg.min(1)[0], *tol, 'ymin vs float64')
        assert int(a.result('amax').max()) < 32 and int(a.result('amin').max()) < 32 and int(a.result('nbt')) == 6
        assert float(a.result('stat')[2 * Cout]) == 0.0  # the completion counter is zero again
    return dict(call=lambda t: lib.call('mvp_mlp_forward_pool_f32', t['X'], ptr(t['X']), R, Cin, ldx, ptr(t['W']), Cin + 4, Cout, *[ptr(t[n]) for n in actn],
                                        ptr(t['ymax']), ptr(t['ymin']), ptr(t['amax']), ptr(t['amin']), ptr(t['stat']), ptr(t['partial']), 1e-5, 0.1,
                                        *[ptr(t[n]) for n in fin]),
                exact=['ymax', 'ymin', 'amax', 'amin', 'nbt'], close=dict({n: BN_FIN for n in fin[:4]}, stat=STAT_FWD), post=post)


for _p in ('bf16x3', 'bf16x6'):
    for _s in ((36, 40, 36), (128, 128, 128)):
        CASES.append(('A-forward_pool-32800x{}x{}-{}'.format(_s[0], _s[2], _p), _p, forward_pool, dict(R=32768 + 32, Cin=_s[0], ldx=_s[1], Cout=_s[2], prec=_p)))


@pytest.mark.parametrize('prec,build,kw', [pytest.param(p, b, k, id=i) for i, p, b, k in CASES if i.startswith('A-')])
def test_shared_mlp_contractions(dev, prec, build, kw):
    run_case(dev, prec, build, kw)


# =====================================================================================================================================
# B. row kernels (rows.hip) and mvp_copy_slices_f32.  B = 2 chunks, N = 50 points, M = 7 centres, K = 5 and 32 neighbours.
# C = 20 is kept where the entry point takes any multiple of 4; the column-statistics family (check_rows: C / 4 must divide the 256 lanes
# of a workgroup) refuses 20 and 36, which are replaced by the nearest widths it accepts, 16 and 32.
# =====================================================================================================================================
NB, NN, NM = 2, 50, 7
SCATTER = (1e-4, 1e-5)   # test_group_rows_vs_channel_major / test_interp_rows_vs_channel_major: the fp32 scatter-add backward


def ball_index(g, K, holes):
    idx = torch.randint(0, NN, (NB, NM, K), generator=g)
    if holes:   # values outside [0, N): group_rows zero-fills such rows
        idx[0, 1, K - 1], idx[1, 3, 0], idx[1, NM - 1, K // 2] = -1, NN, -1
    return idx


def group_rows(a, C, K, ld, with_xyz):
    lib = L()
    g = gen(C, K, ld, 29)
    idx = ball_index(g, K, True)
    a.inp('index', idx, fill=0)
    if C:
        a.inp('feature', rn(g, NB, NN, C))
    if with_xyz:
        a.inp('xyz', ru(g, NB, NN, 3)).inp('centre', ru(g, NB, NM, 3))
    a.out('out', (NB * NM * K, ld))   # all ld columns are written: [feature | xyz - centre | zeros]
    fn, xn, cn = 'feature' if C else None, 'xyz' if with_xyz else None, 'centre' if with_xyz else None

    def post(a):
        o = a.result('out')
        assert float(o[:, C + (3 if with_xyz else 0):].abs().max() if ld > C + (3 if with_xyz else 0) else 0.0) == 0.0
    return dict(call=lambda t: lib.call('mvp_group_rows_f32', t['out'], ptr(t[fn]), ptr(t[xn]), ptr(t[cn]), ptr(t['index']), NB, NN, C, NM, K, ld, ptr(t['out'])),
                exact=['out'], post=post)


def group_rows_backward(a, C, K, ld):
    lib = L()
    g = gen(C, K, ld, 31)
    a.inp('index', ball_index(g, K, False), fill=0).inp('grad_out', rn(g, NB * NM * K, C), ld=ld).out('grad_feature', (NB * NN, C), finite=True)   # (zeroed, then fp32 atomics)
    return dict(call=lambda t: lib.call('mvp_group_rows_backward_f32', t['grad_out'], ptr(t['grad_out']), ptr(t['index']), NB, NN, C, NM, K, ld, ptr(t['grad_feature'])),
                close={'grad_feature': SCATTER})


def relation_rows(a, C, K, four):
    lib = L()
    g = gen(C, K, 37)
    a.inp('src', ru(g, NM * K, 3)).inp('tgt', ru(g, NM, 3))
    if four:
        a.out('out', (NM * K, 4))
        return dict(call=lambda t: lib.call('mvp_relation4_rows_f32', t['out'], ptr(t['src']), ptr(t['tgt']), NM, K, ptr(t['out'])), exact=['out'])
    a.inp('feature', rn(g, NM * K, C)).out('out', (NM * K, C + 4))
    return dict(call=lambda t: lib.call('mvp_relation_rows_f32', t['out'], ptr(t['feature']), ptr(t['src']), ptr(t['tgt']), NM, K, C, ptr(t['out'])), exact=['out'])


def lin_rows(a, C, K, kind, with_opt, with_stat, bn):
    """mvp_group_lin_rows[_bn]_f32 (kind 'group': zf / diff optional) and mvp_interp_add_rows[_bn]_f32 ('interp': add optional)"""
    lib = L()
    g = gen(C, K, 41, int(with_opt), int(bn))
    rows = NB * NM * K if kind == 'group' else NB * NN
    a.out('out', (rows, C))
    fin = [None] * 5
    sn = pn = None
    if with_stat:
        sn, pn = 'stat', 'partial'
        a.acc('stat', torch.zeros(2 * C + 1, dtype=HI) if bn else rn(g, 2 * C).to(HI) * 3.0)
        n = int(lib.lib().mvp_group_lin_partial_count(NB, C, NM, K) if kind == 'group' else lib.lib().mvp_group_lin_partial_count(NB, C, NN, 1))
        assert n > 0
        a.scratch('partial', n)
        if bn:
            fin = bn_outputs(a, g, C)
    tail = (lambda t: (1e-5, 0.1, *[ptr(t[n]) for n in fin])) if bn else (lambda t: ())
    sfx = '_bn_f32' if bn else '_f32'
    # (the partial rows of these shapes are fewer than 128: one workgroup adds each sum, stats_reduce.h -- bit for bit)
    exact = ['out'] + (['stat'] if with_stat else []) + (fin if bn else [])
    if kind == 'group':
        a.inp('index', ball_index(g, K, False), fill=0).inp('xyz', ru(g, NB, NN, 3)).inp('centre', ru(g, NB, NM, 3)).inp('wxyz', rn(g, C, 3))
        zn = dn = None
        if with_opt:
            zn, dn = 'zf', 'diff'
            a.inp('zf', rn(g, NB, NN, C)).out('diff', (rows, 4))
            exact.append('diff')
        return dict(call=lambda t: lib.call('mvp_group_lin_rows' + sfx, t['out'], ptr(t[zn]), ptr(t['xyz']), ptr(t['centre']), ptr(t['wxyz']), ptr(t['index']),
                                            NB, NN, C, NM, K, ptr(t['out']), ptr(t[dn]), ptr(t[sn]), ptr(t[pn]), *tail(t)), exact=exact)
    w = ru(g, NB, NN, 3)
    a.inp('feature', rn(g, NB, NM, C)).inp('index', torch.randint(0, NM, (NB, NN, 3), generator=g), fill=0).inp('weight', w / w.sum(2, keepdim=True))
    an = 'add' if with_opt else None
    if with_opt:
        a.inp('add', rn(g, NB, NN, C))
    return dict(call=lambda t: lib.call('mvp_interp_add_rows' + sfx, t['out'], ptr(t['feature']), ptr(t['index']), ptr(t['weight']), ptr(t[an]), NB, NM, C, NN,
                                        ptr(t['out']), ptr(t[sn]), ptr(t[pn]), *tail(t)), exact=exact)


def interp_rows(a, C, ld, backward):
    lib = L()
    g = gen(C, ld, 43)
    w = ru(g, NB, NN, 3)
    a.inp('index', torch.randint(0, NM, (NB, NN, 3), generator=g), fill=0).inp('weight', w / w.sum(2, keepdim=True))
    if backward:
        a.inp('grad_out', rn(g, NB * NN, C), ld=ld).out('grad_feature', (NB * NM, C), finite=True)   # (zeroed, then fp32 atomics)
        return dict(call=lambda t: lib.call('mvp_interp_rows_backward_f32', t['grad_out'], ptr(t['grad_out']), ptr(t['index']), ptr(t['weight']), NB, NM, C, NN, ld,
                                            ptr(t['grad_feature'])), close={'grad_feature': SCATTER})
    a.inp('feature', rn(g, NB, NM, C)).out('out', (NB * NN, C), ld=ld)
    return dict(call=lambda t: lib.call('mvp_interp_rows_f32', t['out'], ptr(t['feature']), ptr(t['index']), ptr(t['weight']), NB, NM, C, NN, ld, ptr(t['out'])),
                exact=['out'])


def gather_index(g, E):
    idx = torch.randint(0, NN, (NB, E), generator=g)
    idx[0, 0], idx[0, E - 1], idx[1, E // 2], idx[1, 1] = -1, NN, NN + 3, -7   # outside [0, N): ignored
    return idx


def csr_reference(idx, N=NN):
    """offsets (B, N + 1), slots (B, E) with every list ascending, unused tail = 0"""
    Bn, E = idx.shape
    off, slots = torch.zeros(Bn, N + 1, dtype=torch.int32), torch.zeros(Bn, E, dtype=torch.int32)
    for b in range(Bn):
        order = torch.sort(idx[b], stable=True)
        lists = [[] for _ in range(N)]
        for v, e in zip(order[0].tolist(), order[1].tolist()):
            if 0 <= v < N:
                lists[v].append(e)
        flat = [e for l in lists for e in l]
        off[b, 1:] = torch.tensor([len(l) for l in lists]).cumsum(0).to(torch.int32)
        slots[b, :len(flat)] = torch.tensor(flat, dtype=torch.int32)
    return off, slots


def csr_build(a, E, want_sorted):
    lib = L()
    # At N = 50 (the shape the cases are specified at) the library builds the index in ONE launch with the counters in LDS: `cursor` is then not
    # touched at all, so "cursor is a guarded scratch" only says that it stays untouched; the three-launch global path (count / scan / fill,
    # N beyond ~37 000), the only one that uses `cursor` and global arrival order, is not reached by these cases.
    g = gen(E, 47)
    idx = gather_index(g, E)
    off, slots = csr_reference(idx)
    a.inp('index', idx, fill=0).out('offsets', (NB, NN + 1), dtype=torch.int32).out('slots', (NB, E), dtype=torch.int32)
    a.scratch('cursor', NB * NN, dtype=torch.int32)

    def post(a):   # the lists are in arrival order (sorted ascending by the sorted build): compare list by list; the tail behind the last list is not written
        assert torch.equal(a.result('offsets').cpu(), off)
        got = a.result('slots').cpu()
        for b in range(NB):
            for j in range(NN):
                lo, hi = int(off[b, j]), int(off[b, j + 1])
                seg = got[b, lo:hi] if want_sorted else got[b, lo:hi].sort()[0]
                assert torch.equal(seg, slots[b, lo:hi]), (b, j)
    return dict(call=lambda t: lib.call('mvp_csr_build_sorted_i64' if want_sorted else 'mvp_csr_build_i64', t['offsets'], ptr(t['index']), NB, E, NN,
                                        ptr(t['offsets']), ptr(t['slots']), ptr(t['cursor'])), exact=['offsets'], post=post)


def gather_backward(a, C, E, S, ld, weighted, finish):
    lib = L()
    g = gen(C, E, S, 53)
    off, slots = csr_reference(gather_index(g, E))
    rows = NB * (E // S)
    a.inp('offsets', off, fill=0).inp('slots', slots, fill=0).out('grad_feature', (NB * NN, C))
    wn = 'weight' if weighted else None
    if weighted:
        a.inp('weight', ru(g, NB, E))
    if not finish:
        a.inp('grad_out', rn(g, rows, C), ld=ld)
        return dict(call=lambda t: lib.call('mvp_gather_rows_backward_csr_f32', t['grad_out'], ptr(t['grad_out']), ptr(t['offsets']), ptr(t['slots']), ptr(t[wn]),
                                            NB, NN, C, E, S, ld, ptr(t['grad_feature'])), exact=['grad_feature'])
    a.inp('dz', rn(g, rows, C), ld=ld).inp('y', rn(g, rows, C), ld=ld).inp('stat', rn(g, 2 * C).to(HI) * rows * 0.01)
    bn, _ = bn_inputs(a, g, C, 'bn')
    return dict(call=lambda t: lib.call('mvp_gather_rows_backward_csr_finish_f32', t['dz'], ptr(t['dz']), ptr(t['y']), ptr(t[bn[0]]), ptr(t[bn[1]]), ptr(t[bn[2]]),
                                        ptr(t['stat']), 1, ptr(t['offsets']), ptr(t['slots']), ptr(t[wn]), NB, NN, C, E, S, ld, ptr(t['grad_feature'])),
                exact=['grad_feature'])


def colstats(a, G, K, C, partial):
    lib = L()
    g = gen(G, K, C, 59)
    R = G * K
    a.inp('y', rn(g, R, C) * 2 + 0.5).acc('stat', rn(g, 2 * C).to(HI) * 3.0)
    pn = 'partial' if partial else None
    if partial:
        a.scratch('partial', int(lib.lib().mvp_colstats_partial_count(R, C)))
    return dict(call=lambda t: lib.call('mvp_colstats_f32', t['y'], ptr(t['y']), R, C, ptr(t['stat']), ptr(t[pn])), **sums(R, C, partial, ['stat']))


def sums(R, C, partial, names, derived=()):
    """what to compare of a column-statistics pass: with `partial` and at most 128 workgroups one workgroup adds each sum (bit for bit), else fp64 atomics:
    the sums within test_column_statistics_scratch_variant's tolerance, what is derived from them within that test's: 1e-6 / 1e-6 for mean, invstd
    and out, 1e-5 / 1e-5 for dy, 1e-6 / 1e-4 for the backward sums (dgamma / dbeta are those sums as float32)"""
    if partial and max(16, -(-R * C * 4 // (16 * 1024))) <= 128:
        return dict(exact=list(names) + list(derived))
    tol = lambda n: (1e-5, 1e-5) if n == 'dy' else (1e-6, 1e-4) if n in ('dgamma', 'dbeta') else (1e-6, 1e-6)
    return dict(close=dict({n: COLSTAT for n in names}, **{n: tol(n) for n in derived}))


def bn_rows_forward(a, G, K, C, training, partial, pooled, dropout=False):
    """mvp_bn_rows_forward_f32 (K = 1; K > 1 max with arg; K > 1 sum with arg == NULL) and _dropout_f32"""
    lib = L()
    g = gen(G, K, C, 61)
    R = G * K
    a.inp('y', rn(g, R, C) * 2 + 0.5).inp('gamma', ru(g, C) + 0.5).inp('beta', rn(g, C) * 0.3)
    a.out('out', (G, C))
    an = 'arg' if (K > 1 and pooled == 'max') else None
    if an:
        a.out('arg', (G, C), dtype=torch.uint8)
    pn = 'partial' if partial else None
    if partial:
        a.scratch('partial', int(lib.lib().mvp_colstats_partial_count(R, C)))
    if training:
        a.out('stat', (2 * C,), dtype=HI, finite=True).out('mean', (C,)).out('invstd', (C,)).acc('running_mean', rn(g, C)).acc('running_var', ru(g, C) + 0.5)
        rm, rv, sn = 'running_mean', 'running_var', 'stat'
        cmp = sums(R, C, partial, ['stat'], ['mean', 'invstd', 'running_mean', 'running_var', 'out'])
    else:
        a.inp('mean', rn(g, C) * 0.3).inp('invstd', ru(g, C) + 0.5)
        rm = rv = sn = None
        cmp = dict(exact=['out'])
    if an:
        cmp.setdefault('exact', []).append('arg')
    if dropout:
        call = lambda t: lib.call('mvp_bn_rows_forward_dropout_f32', t['y'], ptr(t['y']), ptr(t['gamma']), ptr(t['beta']), R, C, training, 1e-5, 0.1, 1, ptr(t[rm]),
                                  ptr(t[rv]), ptr(t[sn]), ptr(t['mean']), ptr(t['invstd']), ptr(t['out']), ptr(t[pn]), 0.25, SEED)
    else:
        call = lambda t: lib.call('mvp_bn_rows_forward_f32', t['y'], ptr(t['y']), ptr(t['gamma']), ptr(t['beta']), G, K, C, training, 1e-5, 0.1, 1, ptr(t[rm]), ptr(t[rv]),
                                  ptr(t[sn]), ptr(t['mean']), ptr(t['invstd']), ptr(t['out']), ptr(t[an]), ptr(t[pn]))
    return dict(call=call, **cmp)


def bn_rows_backward(a, G, K, C, training, partial, pooled, want_dy, dropout=False):
    """mvp_bn_rows_backward_f32 (K = 1; max over K through arg; sum over K with arg == NULL; dy == NULL: the two sums only) and _dropout_f32"""
    lib = L()
    g = gen(G, K, C, 67)
    R = G * K
    y = rn(g, R, C) * 2 + 0.5
    a.inp('y', y).inp('dsrc', rn(g, G if K > 1 else R, C))
    bn, _ = bn_inputs(a, g, C, 'bn')
    on = an = None
    if K > 1 and pooled == 'max':
        on, an = 'out', 'arg'
        a.inp('out', rn(g, G, C)).inp('arg', torch.randint(0, K, (G, C), generator=g).to(torch.uint8), fill=0)
    a.out('stat', (2 * C,), dtype=HI, finite=True)   # (zeroed by the call, then fp64 atomics: finite guards)
    pn = 'partial' if partial else None
    if partial:
        a.scratch('partial', int(lib.lib().mvp_colstats_partial_count(G if an else R, C)))
    dn = 'dy' if want_dy else None
    if want_dy:
        a.out('dy', (R, C)).out('dgamma', (C,)).out('dbeta', (C,))
    gn, bn_ = ('dgamma', 'dbeta') if want_dy else (None, None)
    cmp = sums(G if an else R, C, partial, ['stat'], ['dy', 'dgamma', 'dbeta'] if want_dy else [])
    if 'close' in cmp:
        cmp['close']['stat'] = (1e-6, 1e-4)   # (that test's tolerance for the BACKWARD sums)
    if dropout:
        call = lambda t: lib.call('mvp_bn_rows_backward_dropout_f32', t['y'], ptr(t['dsrc']), ptr(t['y']), *[ptr(t[n]) for n in bn], R, C, 1, training, ptr(t['stat']),
                                  ptr(t[dn]), ptr(t[gn]), ptr(t[bn_]), ptr(t[pn]), 0.25, SEED)
    else:
        call = lambda t: lib.call('mvp_bn_rows_backward_f32', t['y'], ptr(t['dsrc']), ptr(t[on]), ptr(t[an]), ptr(t['y']), *[ptr(t[n]) for n in bn], G, K, C, 1, training,
                                  ptr(t['stat']), ptr(t[dn]), ptr(t[gn]), ptr(t[bn_]), ptr(t[pn]))
    return dict(call=call, **cmp)


def bn_tail(a, R, C, which):
    """mvp_bn_rows_backward_finish_f32 ('finish') and mvp_bn_finalize_f32 ('finalize')"""
    lib = L()
    g = gen(R, C, 71)
    if which == 'finalize':
        y = rn(g, max(R, 2), C).to(HI)
        a.inp('stat', torch.cat([y.sum(0), (y * y).sum(0)]))
        fin = bn_outputs(a, g, C)
        return dict(call=lambda t: lib.call('mvp_bn_finalize_f32', t['mean'], ptr(t['stat']), max(R, 2), C, 1e-5, 0.1, *[ptr(t[n]) for n in fin]), exact=fin)
    a.inp('dz', rn(g, R, C)).inp('y', rn(g, R, C)).inp('stat', rn(g, 2 * C).to(HI) * R * 0.01)
    bn, _ = bn_inputs(a, g, C, 'bn')
    a.out('dy', (R, C)).out('dgamma', (C,)).out('dbeta', (C,))
    return dict(call=lambda t: lib.call('mvp_bn_rows_backward_finish_f32', t['dz'], ptr(t['dz']), ptr(t['y']), *[ptr(t[n]) for n in bn], R, C, 1, ptr(t['stat']),
                                        ptr(t['dy']), ptr(t['dgamma']), ptr(t['dbeta'])), exact=['dy', 'dgamma', 'dbeta'])


def pool_tail(a, G, C, which):
    """mvp_pool_finalize_f32 ('finalize') and mvp_pool_backward_stats_f32 ('stats')"""
    lib = L()
    g = gen(G, C, 73)
    bn, _ = bn_inputs(a, g, C, 'bn')
    if which == 'finalize':
        ymax = rn(g, G, C) + 1.0
        a.inp('ymax', ymax).inp('ymin', ymax - ru(g, G, C) * 2).inp('amax', torch.randint(0, 32, (G, C), generator=g).to(torch.uint8), fill=0)
        a.inp('amin', torch.randint(0, 32, (G, C), generator=g).to(torch.uint8), fill=0)
        a.out('out', (G, C)).out('arg', (G, C), dtype=torch.uint8).out('ysel', (G, C))
        return dict(call=lambda t: lib.call('mvp_pool_finalize_f32', t['ymax'], ptr(t['ymax']), ptr(t['ymin']), ptr(t['amax']), ptr(t['amin']), *[ptr(t[n]) for n in bn],
                                            G, C, 1, ptr(t['out']), ptr(t['arg']), ptr(t['ysel'])), exact=['out', 'arg', 'ysel'])
    a.inp('dout', rn(g, G, C)).inp('out', torch.relu(rn(g, G, C))).inp('ysel', rn(g, G, C)).out('stat', (2 * C,), dtype=HI, finite=True)
    a.scratch('partial', int(lib.lib().mvp_colstats_partial_count(G, C)))
    return dict(call=lambda t: lib.call('mvp_pool_backward_stats_f32', t['dout'], ptr(t['dout']), ptr(t['out']), ptr(t['ysel']), ptr(t[bn[0]]), ptr(t[bn[1]]), G, C, 1,
                                        ptr(t['stat']), ptr(t['partial'])), **sums(G, C, True, ['stat']))


def copy_slices(a):
    """three slices of different widths; sources are column slices of wider matrices, destinations zero-padded operands whose pad is never written"""
    lib = L()
    g = gen(79)
    spec = [(5, 7, 12, 8), (33, 3, 4, 4), (1, 128, 260, 132)]   # rows, cols, source stride, destination stride
    for i, (r, c, lds, ldd) in enumerate(spec):
        a.inp('src%d' % i, rn(g, r, c), ld=lds).out('dst%d' % i, (r, c), ld=ldd)

    def call(t):
        table = torch.tensor([[t['src%d' % i].data_ptr(), t['dst%d' % i].data_ptr(), lds, ldd, r, c] for i, (r, c, lds, ldd) in enumerate(spec)],
                             dtype=torch.int64, device=t['src0'].device)
        lib.call('mvp_copy_slices_f32', table, ptr(table), len(spec))
        torch.cuda.synchronize()   # (the table is this call's own)

    def post(a):
        for i in range(len(spec)):
            assert torch.equal(a.result('dst%d' % i), a.result('src%d' % i))
    return dict(call=call, exact=['dst%d' % i for i in range(len(spec))], post=post)


for _K in (5, 32):
    for _C in (0, 8, 20):
        for _pad in (4, 8):
            CASES.append(('B-group_rows-C{}-K{}-ld{}'.format(_C, _K, _C + _pad), None, group_rows, dict(C=_C, K=_K, ld=_C + _pad, with_xyz=True)))
            if _C:
                CASES.append(('B-group_rows_backward-C{}-K{}-ld{}'.format(_C, _K, _C + _pad), None, group_rows_backward, dict(C=_C, K=_K, ld=_C + _pad)))
    CASES.append(('B-group_rows-noxyz-C8-K{}-ld12'.format(_K), None, group_rows, dict(C=8, K=_K, ld=12, with_xyz=False)))
    for _C in (8, 20):
        CASES.append(('B-relation_rows-C{}-K{}'.format(_C, _K), None, relation_rows, dict(C=_C, K=_K, four=False)))
    CASES.append(('B-relation4_rows-K{}'.format(_K), None, relation_rows, dict(C=0, K=_K, four=True)))
    for _C in (8, 16):   # (20 is refused: see above)
        for _opt, _stat, _bn in ((False, False, False), (True, True, False), (False, True, True), (True, True, True)):
            CASES.append(('B-group_lin_rows{}{}{}-C{}-K{}'.format('-zf-diff' if _opt else '', '-stat' if _stat else '', '-bn' if _bn else '', _C, _K), None, lin_rows,
                          dict(C=_C, K=_K, kind='group', with_opt=_opt, with_stat=_stat, bn=_bn)))
for _C in (8, 20):
    for _pad in (4, 8):
        for _bwd in (False, True):
            CASES.append(('B-interp_rows{}-C{}-ld{}'.format('_backward' if _bwd else '', _C, _C + _pad), None, interp_rows, dict(C=_C, ld=_C + _pad, backward=_bwd)))
for _C in (8, 16):
    for _opt, _stat, _bn in ((False, False, False), (True, True, False), (False, True, True), (True, True, True)):
        CASES.append(('B-interp_add_rows{}{}{}-C{}'.format('-add' if _opt else '', '-stat' if _stat else '', '-bn' if _bn else '', _C), None, lin_rows,
                      dict(C=_C, K=1, kind='interp', with_opt=_opt, with_stat=_stat, bn=_bn)))
for _E, _S in ((3 * 37, 3), (7 * 5, 1)):
    for _sorted in (False, True):
        CASES.append(('B-csr_build{}-E{}'.format('_sorted' if _sorted else '', _E), None, csr_build, dict(E=_E, want_sorted=_sorted)))
    for _C, _ld in ((8, 12), (20, 28)):
        for _w, _fin in ((False, False), (True, False), (True, True)):
            CASES.append(('B-gather_rows_backward_csr{}{}-C{}-E{}-S{}'.format('_finish' if _fin else '', '-weight' if _w else '', _C, _E, _S), None, gather_backward,
                          dict(C=_C, E=_E, S=_S, ld=_ld, weighted=_w, finish=_fin)))
for _G, _K, _C in ((37, 32, 16), (1, 1, 128), (1031, 1, 32), (13, 3, 64)):   # (37, 32, 20) -> C = 16 and (1031, 1, 36) -> C = 32: see above
    _pool = 'max' if _K == 32 else 'sum'
    for _part in (True, False):
        _t = '-partial' if _part else ''
        CASES.append(('B-colstats{}-{}x{}x{}'.format(_t, _G, _K, _C), None, colstats, dict(G=_G, K=_K, C=_C, partial=_part)))
        CASES.append(('B-bn_rows_forward-train{}-{}x{}x{}'.format(_t, _G, _K, _C), None, bn_rows_forward, dict(G=_G, K=_K, C=_C, training=1, partial=_part, pooled=_pool)))
        CASES.append(('B-bn_rows_backward-train{}-{}x{}x{}'.format(_t, _G, _K, _C), None, bn_rows_backward,
                      dict(G=_G, K=_K, C=_C, training=1, partial=_part, pooled=_pool, want_dy=True)))
    CASES.append(('B-bn_rows_forward-eval-{}x{}x{}'.format(_G, _K, _C), None, bn_rows_forward, dict(G=_G, K=_K, C=_C, training=0, partial=False, pooled=_pool)))
    CASES.append(('B-bn_rows_backward-eval-{}x{}x{}'.format(_G, _K, _C), None, bn_rows_backward,
                  dict(G=_G, K=_K, C=_C, training=0, partial=True, pooled=_pool, want_dy=True)))
    if _pool == 'sum':   # dy == NULL (K = 1, or the sum over K): the two column sums only
        CASES.append(('B-bn_rows_backward-sums_only-{}x{}x{}'.format(_G, _K, _C), None, bn_rows_backward,
                      dict(G=_G, K=_K, C=_C, training=1, partial=True, pooled=_pool, want_dy=False)))
    if _K == 1:
        for _part in (True, False):
            _t = '-partial' if _part else ''
            CASES.append(('B-bn_rows_forward_dropout{}-{}x{}'.format(_t, _G, _C), None, bn_rows_forward,
                          dict(G=_G, K=1, C=_C, training=1, partial=_part, pooled='sum', dropout=True)))
            CASES.append(('B-bn_rows_backward_dropout{}-{}x{}'.format(_t, _G, _C), None, bn_rows_backward,
                          dict(G=_G, K=1, C=_C, training=1, partial=_part, pooled='sum', want_dy=True, dropout=True)))
    CASES.append(('B-bn_rows_backward_finish-{}x{}'.format(_G * _K, _C), None, bn_tail, dict(R=_G * _K, C=_C, which='finish')))
    CASES.append(('B-bn_finalize-{}x{}'.format(_G * _K, _C), None, bn_tail, dict(R=_G * _K, C=_C, which='finalize')))
for _w in ('finalize', 'stats'):   # (1025, 36) -> C = 32: see above
    CASES.append(('B-pool_{}-1025x32'.format(_w), None, pool_tail, dict(G=1025, C=32, which=_w)))
CASES.append(('B-copy_slices', None, copy_slices, dict()))


@pytest.mark.parametrize('prec,build,kw', [pytest.param(p, b, k, id=i) for i, p, b, k in CASES if i.startswith('B-')])
def test_row_kernels(dev, prec, build, kw):
    run_case(dev, prec, build, kw)


# =====================================================================================================================================
# C. fused set-abstraction levels (sa_fused.hip, sa_train.hip).  B = 2, N = 200, M = 37, K = 32; the index has -1 slots and one empty ball.
# Widths (32, 32, 64) and (36, 36, 68); the training entry points need zf, so zf == NULL runs on the inference kernel alone, and the
# per-point statistics pass (256 lanes / (C1 / 4) points per workgroup) refuses C1 = 36: it runs C1 = 32 and the next width it accepts, 64.
# The float64 statistics are carved as rows.py carves them -- stat1 | stat2 | stat3 | zsum | replicas back to back in ONE arena, no guard
# between them -- with the slices a pass does not own declared as inputs holding their own recognisable values: they must stay bit-identical.
# =====================================================================================================================================
SB, SN, SM, SK = 2, 200, 37, 32


def summed(got, want, name):
    """what the workgroups sum with atomics: the convention of test_sa_train_y2_gpu.py::summed_close"""
    close(got, want, 1e-4, 1e-5 * float(want.abs().max()), name)


def slot_sum(got, want, name):
    summed(got.sum(0), want.sum(0), name)   # tsum: 16 slots by workgroup, their sum is the operand (test_backward_passes_from_the_stored_y2)


MEAN = (1e-6, 0.0)   # test_sa_train_y2_gpu.py: mean / invstd of two runs of a pass (fp64 sums whose order is free)


def sa_level(a, widths, with_zf, stage, y2=False):
    lib = L()
    from mvpnet_amd import rows as RW
    C1, C2, C3 = widths
    g = gen(C1, C2, C3, 83)
    G, R = SB * SM, SB * SM * SK
    index = torch.randint(0, SN, (SB, SM, SK), generator=g)
    hole = torch.rand(index.shape, generator=g) < 0.2
    hole[..., 0] = False
    index[hole] = -1
    index[0, 3] = -1   # a ball without any neighbour
    a.inp('index', index, fill=0).inp('xyz', ru(g, SB, SN, 3)).inp('centre', ru(g, SB, SM, 3)).inp('wxyz', rn(g, C1, 3) * 0.5)
    zn = 'zf' if with_zf else None
    if with_zf:
        a.inp('zf', rn(g, SB, SN, C1))
    bn1, _ = bn_inputs(a, g, C1, 'bn1')
    a.inp('W2', rn(g, C2, C1) * 0.2)
    level = lambda t: (ptr(t[zn]), ptr(t['xyz']), ptr(t['centre']), ptr(t['index']), ptr(t['wxyz']), SB, SN, SM, SK, C1, *[ptr(t[n]) for n in bn1], ptr(t['W2']), C2)
    layer3 = stage in ('fused', 'fwd3', 'bwd3')
    bn2 = [None] * 4
    if stage != 'fwd2':
        bn2, _ = bn_inputs(a, g, C2, 'bn2')
    if layer3:
        a.inp('W3', rn(g, C3, C2) * 0.2)
    own3 = lambda t: (*[ptr(t[n]) for n in bn2], ptr(t['W3']) if layer3 else None, C3 if layer3 else 0)
    if stage == 'fused':
        bn3, _ = bn_inputs(a, g, C3, 'bn3')
        a.out('out', (G, C3)).out('arg', (G, C3), dtype=torch.uint8)
        return dict(call=lambda t: lib.call('mvp_sa_fused_forward_f32', t['xyz'], *level(t), *own3(t), *[ptr(t[n]) for n in bn3], ptr(t['out']), ptr(t['arg'])),
                    exact=['out', 'arg'])
    yn = None
    if y2:   # stage 2 writes y_2, every other pass reads it
        yn = 'Y2'
        if stage == 'fwd2':
            a.out('Y2', (R, C2))
        else:
            a.inp('Y2', rn(g, R, C2))
    if stage in ('fwd2', 'fwd3'):
        C = C2 if stage == 'fwd2' else C3
        own = 'stat2' if stage == 'fwd2' else 'stat3'
        stat_arena(a, g, widths, {own}, RW.STATS1_REPLICAS)
        fin = bn_outputs(a, g, C)
        ext = [None] * 4
        exact = ['nbt']
        if stage == 'fwd3':
            ext = ['ymax', 'ymin', 'amax', 'amin']
            a.out('ymax', (G, C3)).out('ymin', (G, C3)).out('amax', (G, C3), dtype=torch.uint8).out('amin', (G, C3), dtype=torch.uint8)
            exact += ext
        elif y2:
            exact.append('Y2')

        def post(a):
            assert int(a.result(own)[2 * C:].view(torch.int64)[0]) == 0 and int(a.result('nbt')) == 6   # the completion counter is zero again
        return dict(call=lambda t: lib.call('mvp_sa_train_forward_f32', t['xyz'], 3 if stage == 'fwd3' else 2, *level(t), *own3(t), ptr(t[own]), 1e-5, 0.1,
                                            *[ptr(t[n]) for n in fin], *[ptr(t[n]) for n in ext], y2=ptr(t[yn])),
                    exact=exact, close={own: summed, 'mean': MEAN, 'invstd': MEAN, 'running_mean': BN_FIN, 'running_var': BN_FIN}, post=post)
    C, Cp = (C3, C2) if stage == 'bwd3' else (C2, C1)
    if stage == 'bwd3':
        a.inp('mean_i', rn(g, C) * 0.3).inp('invstd_i', ru(g, C) + 0.5)
        mi, ii = 'mean_i', 'invstd_i'
        a.inp('pool_dout', rn(g, G, C3)).inp('pool_out', rn(g, G, C3)).inp('pool_arg', torch.randint(0, SK, (G, C3), generator=g).to(torch.uint8), fill=0)
        src = lambda t: (None, ptr(t['pool_dout']), ptr(t['pool_out']), ptr(t['pool_arg']))
    else:
        mi, ii = bn2[0], bn2[1]
        a.inp('G', rn(g, R, C2))
        a.acc('tsum', rn(g, 16, C1, 4))
        src = lambda t: (ptr(t['G']), None, None, None)
    a.inp('gamma_i', ru(g, C) + 0.5).inp('stat_i', rn(g, 2 * C).to(HI) * R * 0.01).out('dgamma', (C,)).out('dbeta', (C,))
    a.acc('dW', rn(g, C, Cp), ld=Cp + 4).out('dZ', (R, Cp)).acc('stat_prev', rn(g, 2 * Cp).to(HI) * 3.0)
    tn = 'tsum' if stage == 'bwd2' else None
    cmp = {'dW': summed, 'stat_prev': summed}
    if tn:
        cmp['tsum'] = slot_sum
    return dict(call=lambda t: lib.call('mvp_sa_train_backward_f32', t['xyz'], 3 if stage == 'bwd3' else 2, *level(t), *own3(t), ptr(t[mi]), ptr(t[ii]),
                                        ptr(t['gamma_i']), ptr(t['stat_i']), ptr(t['dgamma']), ptr(t['dbeta']), 1, *src(t), ptr(t['dW']), Cp + 4, ptr(t['dZ']),
                                        ptr(t['stat_prev']), ptr(t[tn]), y2=ptr(t[yn])),
                exact=['dZ', 'dgamma', 'dbeta'], close=cmp)


def stat_arena(a, g, widths, owned, nrep):
    """stat1 | stat2 | stat3 | zsum | replicas as rows.py lays them out; `owned`: zero on entry and accumulated into, the others inputs with their own values"""
    C1, C2, C3 = widths
    for i, (name, n) in enumerate((('stat1', 2 * C1 + 1), ('stat2', 2 * C2 + 1), ('stat3', 2 * C3 + 1), ('zsum', 3 * C1), ('replicas', max(1, nrep) * 5 * C1))):
        if name in owned:
            a.acc(name, torch.zeros(n, dtype=HI), pack=i > 0)
        else:
            a.inp(name, torch.full((n,), 1000.0 * (i + 1), dtype=HI) + torch.arange(n, dtype=HI), pack=i > 0, finite=True)   # (finite guards around the whole arena)


def sa_points(a, C1, stage):
    """the per-POINT passes: mvp_sa_geom_sums_f32 ('geom'), mvp_sa_train_stats1[_ws]_f32 ('stats1', 'stats1_ws'), mvp_sa_train_backward1_f32 ('bwd1')"""
    lib = L()
    from mvpnet_amd import rows as RW
    g = gen(C1, 89)
    R = SB * SM * SK
    index = torch.randint(0, SN, (SB, SM, SK), generator=g)
    index[torch.rand(index.shape, generator=g) < 0.2] = -1
    index[0, 3] = -1
    off, slots = csr_reference(index.reshape(SB, SM * SK), SN)
    if stage == 'geom':
        a.inp('offsets', off, fill=0).inp('slots', slots, fill=0).inp('xyz', ru(g, SB, SN, 3)).inp('centre', ru(g, SB, SM, 3))
        a.out('dsum', (SB * SN, 4)).acc('gsum', torch.zeros(16, dtype=HI))
        return dict(call=lambda t: lib.call('mvp_sa_geom_sums_f32', t['xyz'], ptr(t['offsets']), ptr(t['slots']), ptr(t['xyz']), ptr(t['centre']), SB, SN, SM, SK,
                                            ptr(t['dsum']), ptr(t['gsum'])), exact=['dsum'], close={'gsum': summed})
    counts = (off[:, 1:] - off[:, :-1]).float()
    dsum = torch.cat([rn(g, SB, SN, 3) * counts.unsqueeze(-1) * 0.1, counts.unsqueeze(-1)], 2)
    a.inp('zf', rn(g, SB, SN, C1)).inp('dsum', dsum).inp('wxyz', rn(g, C1, 3) * 0.5).inp('gsum', ru(g, 16).to(HI) * R)
    if stage.startswith('stats1'):
        ws = stage == 'stats1_ws'
        nrep = RW.STATS1_REPLICAS
        assert not ws or nrep >= 2
        stat_arena(a, g, (C1, C1, C1), {'stat1', 'zsum'} | ({'replicas'} if ws else set()), nrep)
        fin = bn_outputs(a, g, C1)
        tail = (lambda t: (ptr(t['replicas']), nrep * 5 * C1)) if ws else (lambda t: ())
        return dict(call=lambda t: lib.call('mvp_sa_train_stats1_ws_f32' if ws else 'mvp_sa_train_stats1_f32', t['zf'], ptr(t['zf']), ptr(t['dsum']), ptr(t['wxyz']),
                                            ptr(t['gsum']), SB, SN, SM, SK, C1, ptr(t['stat1']), ptr(t['zsum']), 1e-5, 0.1, *[ptr(t[n]) for n in fin], *tail(t)),
                    exact=['nbt'], close={'stat1': summed, 'zsum': summed, 'mean': MEAN, 'invstd': MEAN, 'running_mean': BN_FIN, 'running_var': BN_FIN})
    a.inp('offsets', off, fill=0).inp('slots', slots, fill=0).inp('dz1', rn(g, R, C1)).inp('tsum', rn(g, 16, C1, 4)).inp('zsum', rn(g, 3 * C1).to(HI))
    a.inp('mean', rn(g, C1) * 0.3).inp('invstd', ru(g, C1) + 0.5).inp('gamma', ru(g, C1) + 0.5).inp('stat', rn(g, 2 * C1).to(HI) * R * 0.01)
    a.out('dgamma', (C1,)).out('dbeta', (C1,)).out('gz', (SB * SN, C1)).acc('dWxyz', rn(g, C1, 3), ld=7)
    return dict(call=lambda t: lib.call('mvp_sa_train_backward1_f32', t['zf'], ptr(t['dz1']), ptr(t['offsets']), ptr(t['slots']), ptr(t['zf']), ptr(t['dsum']),
                                        ptr(t['wxyz']), ptr(t['tsum']), ptr(t['zsum']), ptr(t['gsum']), SB, SN, SM, SK, C1, ptr(t['mean']), ptr(t['invstd']),
                                        ptr(t['gamma']), ptr(t['stat']), 1, ptr(t['dgamma']), ptr(t['dbeta']), ptr(t['gz']), ptr(t['dWxyz']), 7),
                exact=['dgamma', 'dbeta', 'gz', 'dWxyz'])


for _w, _zf in (((32, 32, 64), False), ((36, 36, 68), True)):
    for _p in ('bf16x3', 'bf16x6'):
        CASES.append(('C-sa_fused_forward-{}x{}x{}{}-{}'.format(*_w, '' if _zf else '-nozf', _p), _p, sa_level, dict(widths=_w, with_zf=_zf, stage='fused')))
for _w in ((32, 32, 64), (36, 36, 68)):
    for _p in ('mixed', 'bf16x3'):   # (mixed: the forward's three pieces, the backward's two -- what training runs)
        for _st in ('fwd2', 'fwd3', 'bwd3', 'bwd2'):
            for _y2 in (False, True):
                CASES.append(('C-sa_train_{}{}-{}x{}x{}-{}'.format(_st, '_y2' if _y2 else '', *_w, _p), _p, sa_level, dict(widths=_w, with_zf=True, stage=_st, y2=_y2)))
CASES.append(('C-sa_geom_sums', None, sa_points, dict(C1=32, stage='geom')))
for _C1 in (32, 64):
    for _st in ('stats1', 'stats1_ws'):
        CASES.append(('C-sa_train_{}-C{}'.format(_st, _C1), None, sa_points, dict(C1=_C1, stage=_st)))
for _C1 in (32, 36):
    CASES.append(('C-sa_train_backward1-C{}'.format(_C1), None, sa_points, dict(C1=_C1, stage='bwd1')))


@pytest.mark.parametrize('prec,build,kw', [pytest.param(p, b, k, id=i) for i, p, b, k in CASES if i.startswith('C-')])
def test_fused_set_abstraction_levels(dev, prec, build, kw):
    run_case(dev, prec, build, kw)

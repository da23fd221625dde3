"""rows.MLPChainRows: WHICH library entry points a shared-MLP chain launches, in which order and with which arguments.  Host logic only:
the library's entry points are recording stubs, the tensors live on the CPU and nothing reads them.

The GPU tests compare numbers against float64, so a layer that silently takes a slower or a differently rounded route still passes
them; this test pins the routes.  tests/golden/chain_launches.json holds, per case, the ordered list of
[entry point, argument, ...] with a ['SIDE'] marker in front of a launch that went through rows.side_stream.run.  Pointers are
labelled p0, p1, ... per distinct address in order of first appearance within the case (a swapped tensor changes the trace, the
allocation order does not), None is NULL, floats are rounded to 6 places, integers of 2^32 and more (the folded dropout's seed) are
labelled s0, s1, ... the same way.

The fixture records what the code did at the commit named in its `generated_from` field and is not regenerated when the host code is
re-arranged: a trace that differs is a changed launch.  Only a change that MEANS to alter a launch regenerates it,
    python tests/test_chain_launches_cpu.py <tree that holds mvpnet_amd> <commit id>
and says so.
"""
import json
import os
import sys

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'chain_launches.json')

# name -> (R, K, C_in, widths, options of run_case)
CASES = {
    'pooled level': (65536, 32, 32, (32, 64), {}),
    '128-wide': (32768, 1, 128, (128, 128, 128), {}),
    '256-wide': (16384, 1, 384, (256, 256), {}),
    '256-wide, dx-wide': (16384, 1, 384, (256, 256), {'dxw': True}),
    '256-wide x3, dx-wide': (16384, 1, 384, (256, 256, 256), {'dxw': True}),
    'aggregation': (98304, 3, 64, (64, 64), {'gradx': False, 'reduce': 'sum', 'rel': True}),
    'aggregation, 96 feature columns': (98304, 3, 96, (64, 64), {'gradx': False, 'reduce': 'sum', 'rel': True}),
    'aggregation, input with gradient': (98304, 3, 64, (64, 64), {'reduce': 'sum', 'rel': True}),
    'aggregation, 64-wide over many rows': (393216, 3, 64, (64, 64, 64), {'gradx': False, 'reduce': 'sum', 'rel': True}),
    'head': (32768, 1, 128, (128,), {'drop': 0.5, 'act_out': True}),
    'first_done': (65536, 32, 64, (64, 64, 128), {'first_done': True}),
    'first_done, deferred finish': (65536, 1, 128, (128, 128), {'first_done': True, 'defer': True}),
    'eval': (4096, 32, 32, (32, 64), {'train': False}),
    'reproducible, 128-wide': (32768, 1, 128, (128, 128, 128), {'det': True}),
    'reproducible, narrow': (65536, 1, 32, (32, 64, 64), {'det': True}),
    'few rows': (4096, 1, 128, (128, 128), {}),
}

# every entry point the fixture must show, and no other: the lock cannot shrink unnoticed
ENTRY_POINTS = {
    'mvp_mlp_forward_p_f32', 'mvp_mlp_forward_bn_p_f32', 'mvp_mlp_forward_pool_p_f32', 'mvp_mlp_forward_rel_bn_p_f32', 'mvp_pool_finalize_f32',
    'mvp_bn_rows_forward_f32', 'mvp_bn_rows_forward_dropout_f32', 'mvp_colstats_f32', 'mvp_bn_finalize_f32', 'mvp_pool_backward_stats_f32',
    'mvp_bn_rows_backward_f32', 'mvp_bn_rows_backward_dropout_f32', 'mvp_bn_rows_backward_finish_f32', 'mvp_mlp_layer_backward_p_f32',
    'mvp_mlp_layer_backward_wide_pooled_p_f32', 'mvp_mlp_weight_grad_p_f32', 'mvp_mlp_weight_grad_ws_p_f32', 'mvp_mlp_weight_grad_finish_p_f32',
    'mvp_mlp_weight_grad_finish_rel_p_f32', 'mvp_mlp_input_grad_p_f32', 'mvp_mlp_input_grad_wide_p_f32', 'mvp_mlp_weight_grad_finish_act_p_f32',
    'mvp_mlp_layer_backward_ws_p_f32',
}


class Ptr:
    """What the stubbed _lib.ptr / ptr_at return: the address, and the tensor itself so that no address is reused within a case."""
    __slots__ = ('tensor', 'addr')

    def __init__(self, tensor, offset=0):
        self.tensor, self.addr = tensor, tensor.data_ptr() + offset


class FakeLib:
    """The four size queries the chain's host code makes of the library (any fixed formulas)."""

    def mvp_colstats_partial_count(self, R, C):
        return 2 * C * min(2048, (R + 127) // 128)

    def mvp_mlp_layer_backward_partial_count(self, R, cin):
        return 2 * cin * ((R + 127) // 128)

    def mvp_mlp_input_grad_wide_workspace_bytes(self, cout, cin):
        return 6 * cout * cin

    def mvp_mlp_weight_grad_workspace_floats(self):
        return 1024


class Recorder:
    def __init__(self, patch, L, rows):
        self.L, self.rows = L, rows
        self.log, self.pointers, self.seeds = [], {}, {}
        self.workspace = torch.empty(1024)
        fake = FakeLib()
        patch.setattr(L, '_fn', self.entry_point)
        patch.setattr(L, 'ptr', lambda t: None if t is None else Ptr(t))
        patch.setattr(L, 'ptr_at', lambda t, offset: Ptr(t, int(offset) * t.element_size()))
        patch.setattr(L, 'lib', lambda: fake)
        patch.setattr(L, 'current_precision', lambda: (6, 3))
        patch.setattr(L, '_raw_stream', lambda index: 0)
        patch.setattr(L, '_raw_device', lambda: None)
        patch.setattr(L, 'dw_workspace', lambda index, handle: self.workspace)
        patch.setattr(L, 'current_dw_workspace', lambda dev: (Ptr(self.workspace), self.workspace.numel()) if L.DW_WORKSPACE else (None, 0))
        patch.setattr(rows.weight_slices, 'get', lambda w, c0, c1, ld: torch.empty(w.size(0), ld))
        patch.setattr(rows.side_stream, 'run', self.side)
        patch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)

    def label(self, a):
        if a is None:
            return 'NULL'
        if isinstance(a, int) and not isinstance(a, bool) and a == self.workspace.data_ptr():  # (_lib.call appends the workspace's raw address)
            a = Ptr(self.workspace)
        if isinstance(a, Ptr):
            return 'p%d' % self.pointers.setdefault(a.addr, (len(self.pointers), a.tensor))[0]
        if isinstance(a, float):
            return round(a, 6)
        if isinstance(a, int) and not isinstance(a, bool) and a >= 2 ** 32:
            return 's%d' % self.seeds.setdefault(a, len(self.seeds))
        assert isinstance(a, int), a
        return int(a)

    def entry_point(self, name):
        def launch(*args):
            self.log.append([name] + [self.label(a) for a in args[:-1]])  # (the last argument is the stream)
            return 0
        return launch

    def side(self, dev, name, args, tensors, prec=None):
        self.log.append(['SIDE'])
        self.L.call(name, tensors[0], *args, prec=prec)


class Layer(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = torch.nn.Conv1d(cin, cout, 1, bias=False)
        self.bn = torch.nn.BatchNorm1d(cout)
        self.relu = torch.nn.ReLU()


def run_case(patch, L, rows, R, K, cin, widths, gradx=True, train=True, reduce='max', rel=False, first_done=False, defer=False, drop=0.0,
             det=False, dxw=False, act_out=False):
    """-> the launches of shared_mlp_rows (+ backward in training mode) over an (R, cin) input.  first_done: x is the first layer's
    pre-BN output (widths[0] columns; cin counts the feature columns of the skipped weight, which also has three coordinate columns)."""
    rec = Recorder(patch, L, rows)
    patch.setattr(L, 'DW_WORKSPACE', det)
    if dxw:
        patch.setattr(rows, 'DX_WIDE', True)
        patch.setattr(rows, 'DX_WIDE_MIN_ROWS', 64)
    torch.manual_seed(1)
    layers, c = [], cin + (4 if rel else 0) + (3 if first_done else 0)
    for w in widths:
        layers.append(Layer(c, w))
        c = w
    mlp = torch.nn.ModuleList(layers)
    mlp.train(train)
    x = torch.empty(R, widths[0] if first_done else cin, requires_grad=gradx)
    kw = {}
    if rel:
        kw['rel'] = torch.empty(R, 4)
    if defer:
        kw['defer'] = rows.DeferredFinish()
        kw['defer'].accepts = True
    if act_out:
        kw['act_out'] = rows.ActivationHandOver()
    with torch.set_grad_enabled(train):
        out = rows.shared_mlp_rows(x, mlp, K=K, dropout_p=drop, training=train, reduce=reduce, first_done=first_done, **kw)
    assert tuple(out.shape) == (R // K, widths[-1])
    if train:
        out.backward(torch.zeros_like(out))
    return rec.log


def record(name, patch, L, rows):
    R, K, cin, widths, options = CASES[name]
    return run_case(patch, L, rows, R, K, cin, widths, **options)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('name', list(CASES))
def test_chain_launches_match_the_fixture(name, monkeypatch):
    from mvpnet_amd import _lib as L, rows
    want = load_fixture()['cases'][name]
    got = record(name, monkeypatch, L, rows)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, 'launch {} of {!r}'.format(k, name)
    assert got == want


def test_fixture_covers_every_case_and_entry_point():
    cases = load_fixture()['cases']
    assert set(cases) == set(CASES)
    names = {launch[0] for trace in cases.values() for launch in trace} - {'SIDE'}
    assert names == ENTRY_POINTS


if __name__ == '__main__':
    # python tests/test_chain_launches_cpu.py <tree that holds mvpnet_amd> <commit id>: write the fixture from THAT tree's host code
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from mvpnet_amd import _lib, rows as rows_module
    assert os.path.abspath(rows_module.__file__).startswith(os.path.abspath(sys.argv[1]))
    traces = {}
    for case in CASES:
        with pytest.MonkeyPatch.context() as mp:
            traces[case] = record(case, mp, _lib, rows_module)
    with open(FIXTURE, 'w') as f:
        f.write('{\n "generated_from": %s,\n "cases": {\n' % json.dumps(sys.argv[2]))
        f.write(',\n'.join('  %s: [\n%s\n  ]' % (json.dumps(c), ',\n'.join('   ' + json.dumps(l) for l in t)) for c, t in traces.items()))
        f.write('\n }\n}\n')
    print('wrote', FIXTURE, sum(len(t) for t in traces.values()), 'launches')

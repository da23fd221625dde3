"""The capturable solver on the device (csrc/adam.hip: mvp_adam_advance_f32, mvp_adam_step_dev_f32, mvp_lr_multistep_f64;
mvpnet_amd.optim.FusedAdam(capturable=True), DeviceMultiStepLR; mvpnet3d.GraphedTrainStep(solver='captured')): the pinned hyper block bit
for bit, a captured step + schedule that advances on every replay, parity with torch.optim.Adam + MultiStepLR and with the plain FusedAdam
at the project's FusedAdam bars, the deferred clip as the same arithmetic as the in-place one, checkpoints both ways, and the captured
training step of the small model against the same calls issued eagerly."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 6
P_TOL = dict(rtol=2e-6, atol=1e-7)   # the FusedAdam bars of tests/test_optim_gpu.py: parameters ...
M_TOL = dict(rtol=2e-6, atol=2e-6)   # ... and moments


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


FEW = [(1,), (3,), (2048,), (2049,), (5000,), (37, 41)]   # 16-byte vectors, the 1..3 element tail, the workgroup boundary (2048 per workgroup)
MANY = [(1 + (i * 7) % 300,) for i in range(100)]          # more tensors than one launch holds (96): two launches


def _params(dev, kind):
    g = torch.Generator(device='cpu').manual_seed(21)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in (FEW if kind == 'few' else MANY)]
    if kind == 'few':
        base = torch.randn(1001, generator=g).to(dev)
        ps.append(torch.nn.Parameter(base[1:]))  # a view one element into its storage: 4 bytes off a 16-byte boundary, the scalar path
        assert ps[-1].data_ptr() % 16 != 0
    return ps


_GRADS = {}


def _grads(dev, kind):
    """The gradients of the STEPS iterations, drawn once per parameter set (as tests/test_solver_gpu.py::_run_sgd draws them) and only read."""
    if kind not in _GRADS:
        gen = torch.Generator(device='cpu').manual_seed(9)
        shapes = [p.shape for p in _params(dev, kind)]
        _GRADS[kind] = [[(torch.randn(s, generator=gen) * (10.0 ** (it % 3 - 1))).to(dev) for s in shapes] for it in range(STEPS)]
    return _GRADS[kind]


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g.clone()


def _assert_close(pa, oa, pb, ob, what):
    for i, (a, b) in enumerate(zip(pa, pb)):
        for name, x, y, tol in (('param', a.detach(), b.detach(), P_TOL), ('exp_avg', oa.state[a]['exp_avg'], ob.state[b]['exp_avg'], M_TOL),
                                ('exp_avg_sq', oa.state[a]['exp_avg_sq'], ob.state[b]['exp_avg_sq'], M_TOL)):
            x, y = x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
            ratio = np.abs(x - y) / (tol['atol'] + tol['rtol'] * np.abs(y))
            assert ratio.max() <= 1.0, '{}: tensor {} {}: worst |a - b| / (atol + rtol |b|) = {:.3f}'.format(what, i, name, ratio.max())


def _torch_lrs(base_lr, milestones, gamma, epochs):
    """The doubles of torch's MultiStepLR after 1 .. epochs steps."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=milestones, gamma=gamma)
    out = []
    for _ in range(epochs):
        opt.step()
        sched.step()
        out.append(opt.param_groups[0]['lr'])
    return out


def _pinned_hyper(lr, beta1, beta2, t):
    """The header's rule restated in NumPy float64: every operation rounded once."""
    def pow_int(b, t):
        r, x = np.float64(1.0), np.float64(b)
        while t:
            if t & 1:
                r = r * x
            x = x * x
            t >>= 1
        return r
    lr = np.float64(lr)
    bc1 = np.float64(1.0) - pow_int(beta1, t)
    bc2 = np.float64(1.0) - pow_int(beta2, t)
    return np.array([np.float32(lr / bc1), np.float32(np.sqrt(bc2)), np.float32(lr), np.float32(0.0)], dtype=np.float32)


@pytest.mark.parametrize('start', [0, 39998])
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize('lr', [0.002, 0.004])
def test_hyper_block_bit_for_bit(dev, lr, betas, start):
    from mvpnet_amd import _lib as L
    lib = L.lib()
    counts = torch.full((5,), float(start), dtype=torch.float32, device=dev)
    lr_dev = torch.tensor([lr], dtype=torch.float64).to(dev)
    hyper = torch.full((L.LIMITS['MVP_SOLVER_HYPER_F32'],), -1.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with np.errstate(under='ignore'):
        for k in range(1, 9):
            assert lib.mvp_adam_advance_f32(counts.data_ptr(), counts.numel(), lr_dev.data_ptr(), betas[0], betas[1], hyper.data_ptr(), stream) == 0
            got = hyper.cpu().numpy()
            want = _pinned_hyper(lr, betas[0], betas[1], start + k)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (start + k, got, want)
            assert counts.tolist() == [float(start + k)] * 5
    assert float(lr_dev) == lr


def _graph_edges(graph):
    """-> (node handles, (from, to) edges) of a captured torch.cuda.CUDAGraph(keep_graph=True), asked of the HIP runtime the process
    already holds (hipGraphGetNodes / hipGraphGetEdges)."""
    with open('/proc/self/maps') as f:
        paths = {line.split()[-1] for line in f if 'libamdhip64' in line}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    handle, count = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(count)) == 0
    nodes = (ctypes.c_void_p * count.value)()
    assert hip.hipGraphGetNodes(handle, nodes, ctypes.byref(count)) == 0
    assert hip.hipGraphGetEdges(handle, None, None, ctypes.byref(count)) == 0
    src, dst = (ctypes.c_void_p * count.value)(), (ctypes.c_void_p * count.value)()
    assert hip.hipGraphGetEdges(handle, src, dst, ctypes.byref(count)) == 0
    return list(nodes), list(zip(src, dst))


def test_replay_advances(dev):
    """opt.step(); sched.step() captured ONCE: six replays are six updates at the scheduled learning rates."""
    from mvpnet_amd.optim import DeviceMultiStepLR, FusedAdam
    lr, milestones, gamma = 0.002, [2, 4], 0.1
    grads = _grads(dev, 'few')
    pa, pb = _params(dev, 'few'), _params(dev, 'few')
    start = [p.detach().clone() for p in pa]
    oa, ob = (FusedAdam(ps, lr=lr, weight_decay=1e-4, capturable=True) for ps in (pa, pb))
    sa, sb = (DeviceMultiStepLR(o, milestones=milestones, gamma=gamma) for o in (oa, ob))
    static = [torch.zeros_like(p) for p in pa]
    for p, g in zip(pa, static):
        p.grad = g
    oa.materialize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):           # one eager warm-up off the default stream, then everything it moved is put back in place
        oa.step()
        sa.step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    with torch.no_grad():
        for p, p0 in zip(pa, start):
            p.copy_(p0)
            for t in oa.state[p].values():
                t.zero_()
        oa.device_lr(0).fill_(lr)
    sa.load_state_dict(dict(sa.state_dict(), last_epoch=0))
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        oa.step()
        sa.step()
    assert all(float(oa.state[p]['step']) == 0.0 for p in pa)   # a capture runs nothing
    # the graph: advance -> step -> schedule, a chain (every node at most one predecessor and one successor: no parallel branch)
    nodes, edges = _graph_edges(graph)
    assert len(nodes) == 3 and len(edges) == len(nodes) - 1, (nodes, edges)
    assert all(sum(1 for e in edges if e[0] == n) <= 1 and sum(1 for e in edges if e[1] == n) <= 1 for n in nodes), edges
    graph.instantiate()
    want_lr = _torch_lrs(lr, milestones, gamma, STEPS)
    for it in range(STEPS):
        for s, g in zip(static, grads[it]):
            s.copy_(g)
        graph.replay()
        assert float(oa.device_lr(0)) == float(sa.get_last_lr()[0]) == want_lr[it], (it, float(oa.device_lr(0)), want_lr[it])
    for it in range(STEPS):                  # the eager twin on the same gradients
        _set_grads(pb, grads[it])
        ob.step()
        sb.step()
    for a, b, a0 in zip(pa, pb, start):
        assert torch.equal(a, b) and not torch.equal(a, a0)
        assert torch.equal(oa.state[a]['exp_avg'], ob.state[b]['exp_avg']) and torch.equal(oa.state[a]['exp_avg_sq'], ob.state[b]['exp_avg_sq'])
        assert float(oa.state[a]['step']) == float(ob.state[b]['step']) == float(STEPS)
    assert sa.last_epoch == sb.last_epoch == STEPS and float(ob.device_lr(0)) == want_lr[-1]


@pytest.mark.parametrize('kind', ['few', 'many'])
@pytest.mark.parametrize('weight_decay', [0.0, 1e-4])
def test_against_torch_adam_and_the_plain_fused_adam(dev, weight_decay, kind):
    from mvpnet_amd.optim import DeviceMultiStepLR, FusedAdam
    lr, milestones, gamma = 0.002, [3], 0.1
    grads = _grads(dev, kind)
    pa, pb, pc = _params(dev, kind), _params(dev, kind), _params(dev, kind)
    oa = FusedAdam(pa, lr=lr, weight_decay=weight_decay, capturable=True)
    ob = torch.optim.Adam(pb, lr=lr, weight_decay=weight_decay, foreach=False)
    oc = FusedAdam(pc, lr=lr, weight_decay=weight_decay)
    sa = DeviceMultiStepLR(oa, milestones=milestones, gamma=gamma)
    sb = torch.optim.lr_scheduler.MultiStepLR(ob, milestones=milestones, gamma=gamma)
    sc = torch.optim.lr_scheduler.MultiStepLR(oc, milestones=milestones, gamma=gamma)
    for it in range(STEPS):
        for ps, o, s in ((pa, oa, sa), (pb, ob, sb), (pc, oc, sc)):
            _set_grads(ps, grads[it])
            o.step()
            s.step()
    assert float(oa.device_lr(0)) == ob.param_groups[0]['lr'] == oc.param_groups[0]['lr']
    assert all(float(oa.state[p]['step']) == float(STEPS) and oa.state[p]['step'].is_cuda and oa.state[p]['step'].dtype == torch.float32 for p in pa)
    _assert_close(pa, oa, pb, ob, 'capturable against torch.optim.Adam')
    _assert_close(pa, oa, pc, oc, 'capturable against the plain FusedAdam')


@pytest.mark.parametrize('max_norm', [0.5, 1e6])
def test_deferred_clip_is_the_same_arithmetic(dev, max_norm):
    """total_grad_norm + step(grad_scale=coef) against clip_grad_norm_ + step(): one rounded product per gradient element either way."""
    from mvpnet_amd import optim
    grads = _grads(dev, 'few')
    pa, pb = _params(dev, 'few'), _params(dev, 'few')
    oa, ob = (optim.FusedAdam(ps, lr=0.002, weight_decay=1e-4, capturable=True) for ps in (pa, pb))
    for it in range(3):
        _set_grads(pa, grads[it])
        _set_grads(pb, grads[it])
        total_a, coef = optim.total_grad_norm(pa, max_norm)
        oa.step(grad_scale=coef)
        total_b = optim.clip_grad_norm_(pb, max_norm)
        ob.step()
        assert torch.equal(total_a, total_b)
        assert float(coef) == 1.0 if max_norm == 1e6 else float(coef) < 1.0
        for p, g in zip(pa, grads[it]):     # the deferred form leaves the gradients as they were
            assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32))
        if max_norm == 0.5:
            assert not torch.equal(pb[4].grad, grads[it][4])
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert torch.equal(oa.state[a]['exp_avg'], ob.state[b]['exp_avg']) and torch.equal(oa.state[a]['exp_avg_sq'], ob.state[b]['exp_avg_sq'])


def _run(opts, plists, grads, its):
    for it in its:
        for o, ps in zip(opts, plists):
            _set_grads(ps, grads[it])
            o.step()


def test_checkpoint_capturable_to_plain(dev):
    from mvpnet_amd.optim import FusedAdam
    grads = _grads(dev, 'few')
    pa = _params(dev, 'few')
    oa = FusedAdam(pa, lr=0.002, weight_decay=1e-4, capturable=True)
    _run([oa], [pa], grads, range(3))
    sd = copy.deepcopy(oa.state_dict())
    assert sd['param_groups'][0]['lr'] == 0.002 and sd['param_groups'][0]['capturable'] is False
    assert all(not v['step'].is_cuda and float(v['step']) == 3.0 for v in sd['state'].values())
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = torch.optim.Adam(pb, lr=1.0, foreach=False)   # (its own lr and weight decay are replaced by the checkpoint's)
    ob.load_state_dict(sd)
    _run([oa, ob], [pa, pb], grads, range(3, 5))
    assert all(float(ob.state[p]['step']) == 5.0 for p in pb) and all(float(oa.state[p]['step']) == 5.0 for p in pa)
    _assert_close(pa, oa, pb, ob, 'torch.optim.Adam resumed from the capturable checkpoint')


def test_checkpoint_plain_to_capturable_with_a_decayed_lr(dev):
    from mvpnet_amd.optim import DeviceMultiStepLR, FusedAdam
    lr, milestones, gamma = 0.002, [2, 4], 0.1
    grads = _grads(dev, 'few')
    pb = _params(dev, 'few')
    ob = torch.optim.Adam(pb, lr=lr, weight_decay=1e-4, foreach=False)
    sb = torch.optim.lr_scheduler.MultiStepLR(ob, milestones=milestones, gamma=gamma)
    for it in range(3):
        _run([ob], [pb], grads, [it])
        sb.step()
    sd, ssd = copy.deepcopy(ob.state_dict()), copy.deepcopy(sb.state_dict())
    assert sd['param_groups'][0]['lr'] == lr * gamma != lr      # decayed at epoch 2
    pa = [torch.nn.Parameter(p.detach().clone()) for p in pb]
    oa = FusedAdam(pa, lr=lr, weight_decay=1e-4, capturable=True)
    oa.load_state_dict(sd)
    assert float(oa.device_lr(0)) == lr * gamma
    assert all(oa.state[p]['step'].is_cuda and float(oa.state[p]['step']) == 3.0 for p in pa)
    sa = DeviceMultiStepLR(oa, milestones=milestones, gamma=gamma)
    sa.load_state_dict(ssd)
    assert sa.last_epoch == sb.last_epoch == 3 and float(sa.get_last_lr()[0]) == sb.get_last_lr()[0]
    assert sa.state_dict()['milestones'] == ssd['milestones'] and sa.state_dict()['base_lrs'] == ssd['base_lrs'] == [lr]
    for it in range(3, 5):                   # epoch 4 decays again, in both
        _run([oa, ob], [pa, pb], grads, [it])
        sa.step()
        sb.step()
        assert float(oa.device_lr(0)) == ob.param_groups[0]['lr']
    assert sa.last_epoch == 5 and ob.param_groups[0]['lr'] == _torch_lrs(lr, milestones, gamma, 5)[-1]
    _assert_close(pa, oa, pb, ob, 'the capturable optimizer resumed from the torch checkpoint')
    assert oa.state_dict()['param_groups'][0]['lr'] == ob.param_groups[0]['lr']   # read back from the device
    with pytest.raises(ValueError):
        DeviceMultiStepLR(oa, milestones=[2, 5], gamma=gamma, last_epoch=5).load_state_dict(ssd)   # another schedule


def test_unequal_loaded_counts_and_missing_state_are_refused(dev):
    from mvpnet_amd.optim import FusedAdam
    grads = _grads(dev, 'few')
    pa = _params(dev, 'few')
    oa = FusedAdam(pa, lr=0.002, capturable=True)
    _run([oa], [pa], grads, range(2))
    sd = copy.deepcopy(oa.state_dict())
    sd['state'][2]['step'] = torch.tensor(5.0)
    oa.load_state_dict(sd)
    _set_grads(pa, grads[2])
    with pytest.raises(RuntimeError, match='non-capturable'):
        oa.step()
    # a capturable step that would have to create state inside a capture
    pb = _params(dev, 'few')
    ob = FusedAdam(pb, lr=0.002, capturable=True)
    _set_grads(pb, grads[0])
    before = [p.detach().clone() for p in pb]
    dummy = torch.zeros(4, device=dev)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match='materialize'):
        with torch.cuda.graph(graph):
            dummy.add_(1.0)                  # (the capture is not empty)
            ob.step()
    torch.cuda.synchronize(dev)
    assert all(len(ob.state[p]) == 0 for p in pb) and all(torch.equal(p, q) for p, q in zip(pb, before))
    ob.materialize()                         # ... after which the eager step is the ordinary one
    ob.step()
    assert all(float(ob.state[p]['step']) == 1.0 for p in pb)


# ---- model level: the builder, batches and stub of tests/test_model_gpu.py::test_graphed_train_step_matches_eager ----
CFG = dict(num_centroids=(256, 64, 16, 4), radius=(0.1, 0.2, 0.4, 0.8), max_neighbors=(32, 32, 32, 32))


class StubNet2D(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.feature = None

    def forward(self, data):
        return {'feature': self.feature}


class _NoStep:
    """An optimizer stand-in for GraphedTrainStep(solver='eager'): clears the gradients, steps nothing."""

    def __init__(self, optimizer):
        self.optimizer = optimizer

    def zero_grad(self, set_to_none=True):
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def step(self):
        pass


def _build(dev):
    from mvpnet_amd.mvpnet3d import MVPNet3D
    from mvpnet_amd.pn2 import PN2SSG
    torch.manual_seed(5)
    return MVPNet3D(StubNet2D(), '', PN2SSG(16, 20, dropout_prob=0.0, **CFG), in_channels=16, mlp_channels=(16, 16, 16)).to(dev).train()


def _batch_of(dev, ids):
    from mvpnet_amd.synthetic import make_chunk
    cs = [make_chunk(800 + i, nb_pts=1024, nv=2, h=30, w=40, channels=16) for i in ids]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = lambda k: np.stack([c[k] for c in cs])
    b = {'images': torch.zeros(len(ids), 2, 3, 30, 40, device=dev), 'points': t(st('points').transpose(0, 2, 1)),
         'seg_label': t(np.maximum(st('seg_label'), 0)), 'depth': t(st('depth_mm').astype(np.int16)),
         'cam_matrix': t(np.stack([np.repeat(c['cam_matrix'][None, :3, :3], 2, 0) for c in cs])), 'kinv': t(st('kinv')),
         'pose': t(st('pose')), 'pixel_box': t(st('pixel_box')), 'k': 3}
    return b, t(st('feature_2d')).view(len(ids) * 2, 30, 40, 16).permute(0, 3, 1, 2)


@pytest.fixture(scope='module')
def batches(dev):
    (ba, fa), (bb, fb) = _batch_of(dev, [0, 1]), _batch_of(dev, [2, 3])
    return [ba, bb, ba, bb], [fa, fb, fa]


def _model_run(dev, batches, solver, max_norm):
    from mvpnet_amd import optim
    from mvpnet_amd.mvpnet3d import GraphedTrainStep, SegLoss
    seq, feats = batches
    model = _build(dev)
    params = list(model.parameters())
    opt = optim.FusedAdam(params, lr=0.002, capturable=True)
    sched = optim.DeviceMultiStepLR(opt, milestones=[2], gamma=0.1)
    static_feat = feats[0].clone()
    model.net_2d.feature = static_feat
    if solver == 'captured':
        g = GraphedTrainStep(model, SegLoss(), opt, dict(seq[0]), dict(seq[1]), scheduler=sched, max_grad_norm=max_norm, warmup=1,
                             geometry='captured', solver='captured')
    else:
        g = GraphedTrainStep(model, SegLoss(), _NoStep(opt), dict(seq[0]), dict(seq[1]), max_grad_norm=0, warmup=1, geometry='captured',
                             solver='eager')
    model.load_state_dict(copy.deepcopy(_build(dev).state_dict()))   # the constructor's warm-up moved the BatchNorm running statistics
    losses = []
    for i in range(3):
        static_feat.copy_(feats[i])
        loss = g.step(seq[i], seq[i + 1])[0]
        if solver == 'eager':                # the same three calls, issued eagerly behind the replay
            coef = None
            if max_norm > 0:
                coef = optim.total_grad_norm(params, max_norm)[1]
            opt.step(grad_scale=coef)
            sched.step()
        losses.append(float(loss))
    counts = [float(opt.state[p]['step']) for p in params if p.grad is not None]
    return losses, [p.detach().clone() for p in params], counts, float(opt.device_lr(0)), sched.last_epoch


@pytest.mark.parametrize('max_norm', [0, 1.0])
def test_captured_solver_equals_the_eager_tail(dev, batches, max_norm):
    """In the reproducible mode both runs execute the same kernels on the same bits: losses and parameters are EQUAL.  A difference is a
    missing dependency or a stale pointer in the capture."""
    from mvpnet_amd import _lib as L
    old = L.set_deterministic(True)
    try:
        captured = _model_run(dev, batches, 'captured', max_norm)
        eager = _model_run(dev, batches, 'eager', max_norm)
    finally:
        L.set_deterministic(old)
    print('losses captured', captured[0], 'eager', eager[0])
    assert captured[0] == eager[0] and len(set(captured[0])) == 3
    assert len(captured[1]) == len(eager[1]) and all(torch.equal(a, b) for a, b in zip(captured[1], eager[1]))
    assert captured[2] == eager[2] and captured[2] and set(captured[2]) == {3.0}
    assert captured[3] == eager[3] == _torch_lrs(0.002, [2], 0.1, 3)[-1] and captured[4] == eager[4] == 3
    start = list(_build(dev).parameters())
    assert any(not torch.equal(a, b) for a, b in zip(captured[1], start))     # ... and the captured solver did train


def test_captured_solver_conditions(dev):
    from mvpnet_amd import optim
    from mvpnet_amd.mvpnet3d import GraphedTrainStep
    ps = [torch.nn.Parameter(torch.zeros(4, device=dev))]
    plain, cap = optim.FusedAdam(ps, lr=0.002), optim.FusedAdam(ps, lr=0.002, capturable=True)
    for kw in (dict(optimizer=plain), dict(optimizer=cap, scheduler=torch.optim.lr_scheduler.MultiStepLR(plain, milestones=[2])),
               dict(optimizer=cap, grad_sync=lambda weight_sum=None: None)):
        with pytest.raises(ValueError):      # refused before anything is run
            GraphedTrainStep(None, None, kw.pop('optimizer'), {}, {}, solver='captured', **kw)

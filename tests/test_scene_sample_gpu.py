"""The 3D baselines' batch drawn on the MI355X: mvp_sample_scenes_f32 and mvp_gather_cloud_f32 bit for bit against the NumPy restatement
(tests/scene_sample_oracle.py) and, for the rotation and the colours, against the reference's own results (tests/golden/scene_sample.npz);
ops.sample_scenes against the whole-scene fallback of ops.sample_chunks; scene.sample_train_batch_3d against the batch assembled by hand."""
import numpy as np
import pytest
import torch

from tests import scene_sample_oracle as SS
from tests import train_sample_oracle as TO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TILE = 8192  # (key, index) pairs one workgroup sorts in LDS (csrc/scene_sample.hip, kTile): past it the sorted tiles are merged


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def both(sizes, rows, nb_pts, seed, Ntot=None):
    """ops.sample_scenes and the oracle on the same arguments, asserted equal -> choice (B,nb_pts) as numpy"""
    import mvpnet_amd.ops as ops
    off, rows = offsets(sizes), np.asarray(rows, np.int64)
    out = ops.sample_scenes(t(off), t(rows), nb_pts, seed=seed, Ntot=Ntot)
    choice, num = SS.sample_scenes(off, rows, nb_pts, seed=seed)
    got = out['choice'].cpu().numpy()
    assert out['choice'].dtype == torch.int64 and got.shape == (len(rows), nb_pts) and out['num_points'].dtype == torch.int32
    assert np.array_equal(out['num_points'].cpu().numpy(), num)
    for b in range(len(rows)):
        assert np.array_equal(got[b], choice[b]), 'row %d (n = %d)' % (b, num[b])
    return got


def cloud_store(sizes, seed, extent=3.0):
    rs = np.random.RandomState(seed)
    n = int(sum(sizes))
    points = (rs.rand(n, 3) * extent).astype(np.float32)
    label = rs.randint(0, 20, n).astype(np.int64)
    label[rs.rand(n) < 0.3] = -100
    colors = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    return points, label, colors


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb_pts', [1, 255, 8192, 8193, 32768, 65536])
def test_scene_sizes_around_nb_pts(nb_pts):
    """n = nb_pts - 1 (a pad; for nb_pts = 1 a scene without points), nb_pts (a crop that keeps every point), nb_pts + 1 and 100 003, one
    row each in one call; 8193 is the first size past one LDS sort, 65536 merges eight tiles three times."""
    sizes = [nb_pts - 1, nb_pts, nb_pts + 1, 100003]
    got = both(sizes, [0, 1, 2, 3], nb_pts, seed=1000 + nb_pts, Ntot=sum(sizes))
    assert np.array_equal(np.sort(got[1]), np.arange(nb_pts))
    if nb_pts > 8:
        assert not np.array_equal(got[1], np.arange(nb_pts)), 'key order, not index order'
    if nb_pts == 1:
        assert got[0, 0] == 0


def test_one_point_padded_past_a_tile():
    got = both([1, 5], [0], TILE + 1, seed=4)
    assert (got == 0).all()


@pytest.mark.parametrize('rows', [[0, 1, 2, 3], [1, 0, 1, 3]])
def test_mixed_batch(rows):
    """Pad and crop rows in one call, nb_pts between two and three tiles; the same scene twice: two draws."""
    sizes = [5000, 40000, 20001, 19999]
    got = both(sizes, rows, 20000, seed=77, Ntot=sum(sizes))
    if rows.count(1) == 2:
        a, b = (i for i, r in enumerate(rows) if r == 1)
        assert not np.array_equal(got[a], got[b]) and len(np.intersect1d(got[a], got[b])) < 20000


def test_without_the_store_size_and_with_a_64_bit_seed():
    """Ntot left out (the limit stands in: 256 workgroups per row, most of them idle) and given: the same choice; both words of the seed count"""
    sizes = [3000, 70000]
    a = both(sizes, [1, 0, 1], 9000, seed=(5 << 32) | 9)
    b = both(sizes, [1, 0, 1], 9000, seed=(5 << 32) | 9, Ntot=sum(sizes))
    c = both(sizes, [1, 0, 1], 9000, seed=(6 << 32) | 9, Ntot=sum(sizes))
    assert np.array_equal(a, b) and not np.array_equal(a[0], c[0])


@pytest.mark.parametrize('nb_pts', [1, 255, 8192])
def test_equals_the_chunk_samplers_whole_scene_fallback(nb_pts):
    """chunk_thresh = 2.0: no try can pass, ops.sample_chunks falls back to the whole scene; the same seed: the same choice, bit for bit"""
    import mvpnet_amd.ops as ops
    sizes = [nb_pts + 1, max(nb_pts - 1, 1), 30000, nb_pts]
    points, label, _ = cloud_store(sizes, 5)
    off, rows = offsets(sizes), np.array([0, 1, 2, 3, 2], np.int64)
    args = (t(off), t(rows))
    for seed in (12, torch.tensor([(3 << 32) + 12], dtype=torch.int64, device=DEV)):
        ch = ops.sample_chunks(t(points), t(label), *args, t(np.zeros((5, 2), np.int64)), nb_pts, chunk_thresh=2.0, seed=seed)
        sc = ops.sample_scenes(*args, nb_pts, seed=seed, Ntot=len(points))
        assert (ch['try_index'] == -1).all() and torch.equal(ch['num_members'], sc['num_points'])
        assert torch.equal(ch['choice'], sc['choice'])
    assert np.array_equal(sc['choice'].cpu().numpy(), SS.sample_scenes(off, rows, nb_pts, seed=(3 << 32) + 12)[0])


# ---- the gather -------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_floats(a, b):
    """bit-equal, except that a NaN an operation produced (inf * 0 under a rotation) is any NaN: its sign and payload are the platform's"""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def check_gather(points, off, rows, choice, label, colors, rot):
    import mvpnet_amd.ops as ops
    out = ops.gather_cloud(t(points), t(off), t(rows), t(choice), seg_label=None if label is None else t(label),
                           colors=None if colors is None else t(colors), rot=None if rot is None else t(rot))
    exp = SS.gather_cloud(points, off, rows, choice, seg_label=label, colors=colors, rot=rot)
    assert sorted(out) == sorted(exp)
    B, nb = choice.shape
    assert tuple(out['points'].shape) == (B, 3, nb) and out['points'].dtype == torch.float32 and out['points'].is_contiguous()
    got = out['points'].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(exp['points'])) if rot is None else _same_floats(got, exp['points'])
    if label is not None:
        assert out['seg_label'].dtype == torch.int64 and np.array_equal(out['seg_label'].cpu().numpy(), exp['seg_label'])
    if colors is not None:
        assert tuple(out['feature'].shape) == (B, 3, nb) and np.array_equal(_bits(out['feature'].cpu().numpy()), _bits(exp['feature']))
    return out, exp


@pytest.fixture(scope='module')
def gather_case():
    sizes = [700, 0, 1300, 1]
    points, label, colors = cloud_store(sizes, 11)
    points[5] = [-0.0, np.nan, 1.5]
    points[6] = [np.inf, -0.0, -0.0]
    points[700] = [-0.0, -0.0, -0.0]
    colors.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    off, rows = offsets(sizes), np.array([0, 2, 1, 3, 2, 7, -1], np.int64)  # (a scene without points; scene numbers out of range are clamped)
    rs = np.random.RandomState(3)
    nb = 4 * 256 + 37  # more than one workgroup of four slots a lane, and a ragged tail
    choice = np.stack([rs.randint(0, max(int(np.diff(off)[np.clip(r, 0, 3)]), 1), nb) for r in rows]).astype(np.int64)
    choice[0, :9] = [5, 6, 0, 699, 5, -3, 700, 2 ** 40, -2 ** 40]  # the special rows, and indices out of range (clamped)
    rot = SS.z_rotation(rs.uniform(-np.pi, np.pi, len(rows)))
    return points, off, rows, choice, label, colors, rot


@pytest.mark.parametrize('with_label', [False, True])
@pytest.mark.parametrize('with_colors', [False, True])
@pytest.mark.parametrize('with_rot', [False, True])
def test_gather_with_and_without_each_optional_input(gather_case, with_label, with_colors, with_rot):
    points, off, rows, choice, label, colors, rot = gather_case
    out, exp = check_gather(points, off, rows, choice, label if with_label else None, colors if with_colors else None, rot if with_rot else None)
    assert ('seg_label' in out) == with_label and ('feature' in out) == with_colors
    if with_label:
        assert (out['seg_label'][2] == -100).all()
    assert (out['points'][2] == 0).all()  # the row of the scene without points


def test_gather_without_rotation_copies_the_bits(gather_case):
    points, off, rows, choice, label, colors, rot = gather_case
    out, _ = check_gather(points, off, rows, choice, None, None, None)
    got = out['points'].cpu().numpy()
    j = np.clip(choice[0], 0, 699)
    assert np.array_equal(_bits(got[0].T), _bits(points[j]))
    assert np.signbit(got[0, 0, 0]) and got[0, 0, 0] == 0 and np.isnan(got[0, 1, 0]) and np.isinf(got[0, 0, 1]) and np.signbit(got[0, 1, 1])


def test_gather_against_the_reference(golden):
    """The reference's matrices on the fixture cloud, one row per angle: rotated points within twice the float32 dot-product bound of the
    reference's (tests/test_scene_sample_cpu.py), features and labels its bits."""
    fx = golden('scene_sample')
    points, colors, label = SS.fixture_cloud()
    n, A = len(points), len(fx['angle'])
    rows, choice = np.zeros(A, np.int64), np.tile(np.arange(n, dtype=np.int64), (A, 1))
    out, _ = check_gather(points, offsets([n]), rows, choice, label, colors, fx['rot'])
    got = out['points'].cpu().numpy().transpose(0, 2, 1).astype(np.float64)
    bound = 6.0 * 2.0 ** -24 * np.abs(points.astype(np.float64)).sum(1)
    err = np.abs(got - fx['rotated'].astype(np.float64)).max(2)
    print('rotated points: largest error / bound = %.3f' % float((err / bound).max()))
    assert (err <= bound).all()
    assert np.array_equal(_bits(out['feature'][0].cpu().numpy().T), _bits(fx['feature']))
    assert (out['seg_label'].cpu().numpy() == label).all()
    # the matrices drawn by the product's formula at the fixture's angles: the same bound holds against the reference
    out2, _ = check_gather(points, offsets([n]), rows, choice, None, None, SS.z_rotation(fx['angle']))
    scale = np.abs(points.astype(np.float64)).sum(1)
    err2 = np.abs(out2['points'].cpu().numpy().transpose(0, 2, 1).astype(np.float64) - fx['rotated'].astype(np.float64)).max(2)
    assert (err2 <= bound + 2.0 ** -23 * scale).all()  # + the matrices' own rounding (2^-23 per entry, test_scene_sample_cpu.py)


def test_gather_a_choice_from_each_sampler():
    import mvpnet_amd.ops as ops
    sizes = [9000, 3000]
    points, label, colors = cloud_store(sizes, 21)
    off, rows = offsets(sizes), np.array([0, 1, 0], np.int64)
    rot = SS.z_rotation(np.array([0.3, -2.0, 3.1]))
    dev = [t(points), t(label), t(off), t(rows)]
    sc = ops.sample_scenes(dev[2], dev[3], 8193, seed=5, Ntot=len(points))['choice']
    centers = np.array([[10, 20, 30], [5, 6, 7], [100, 200, 300]], np.int64)
    ch = ops.sample_chunks(*dev, t(centers), 1024, chunk_size=(1.0, 1.0), seed=5, bounds_f64=True)
    for choice in (sc, ch['choice']):
        out, _ = check_gather(points, off, rows, choice.cpu().numpy(), label, colors, rot)
    # without the rotation the gather is the chunk sampler's own
    plain = ops.gather_cloud(dev[0], dev[2], dev[3], ch['choice'], seg_label=dev[1])
    assert torch.equal(plain['points'], ch['points']) and torch.equal(plain['seg_label'], ch['seg_label'])


# ---- graph, seeds, no host synchronisation ----------------------------------------------------------------------------------------------
def test_graph_replays_draw_afresh_from_a_device_seed():
    import mvpnet_amd.ops as ops
    sizes = [12000, 900, 30000]
    points, label, colors = cloud_store(sizes, 31)
    off, rows, nb = offsets(sizes), np.array([0, 1, 2, 0], np.int64), 9001
    rot = SS.z_rotation(np.array([0.1, 0.2, 0.3, 0.4]))
    dp, dl, dc, do, dr, drot = t(points), t(label), t(colors), t(off), t(rows), t(rot)
    seed_t = torch.tensor([11], dtype=torch.int64, device=DEV)

    def run():
        s = ops.sample_scenes(do, dr, nb, seed=seed_t, Ntot=len(points))
        g = ops.gather_cloud(dp, do, dr, s['choice'], seg_label=dl, colors=dc, rot=drot)
        return dict(g, choice=s['choice'], num_points=s['num_points'])
    eager = run()  # (the scratch exists from here on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        again = run()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert all(torch.equal(eager[k], again[k]) for k in eager)
    assert torch.equal(eager['choice'], ops.sample_scenes(do, dr, nb, seed=11, Ntot=len(points))['choice'])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = run()
    for rep, seed in enumerate([12, 13]):
        seed_t.fill_(seed)
        for v in r.values():
            v.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        choice, num = SS.sample_scenes(off, rows, nb, seed=seed)
        exp = SS.gather_cloud(points, off, rows, choice, seg_label=label, colors=colors, rot=rot)
        assert np.array_equal(r['choice'].cpu().numpy(), choice) and np.array_equal(r['num_points'].cpu().numpy(), num), rep
        assert _same_floats(r['points'].cpu().numpy(), exp['points']), rep
        assert np.array_equal(r['seg_label'].cpu().numpy(), exp['seg_label']) and np.array_equal(r['feature'].cpu().numpy(), exp['feature']), rep
    assert not np.array_equal(choice, eager['choice'].cpu().numpy())


def _store(sizes, seed):
    points, label, colors = cloud_store(sizes, seed)
    host = dict(points=points, seg_label=label, colors=colors, scene_offsets=offsets(sizes))
    return host, {k: t(v) for k, v in host.items()}


@pytest.mark.parametrize('dataset,nb_pts', [('ScanNet3DChunks', 1024), ('ScanNet3DScene', 8193)])
@pytest.mark.parametrize('z_rot', [None, (-np.pi, np.pi)])
def test_sample_train_batch_3d_equals_the_hand_assembled_batch(dataset, nb_pts, z_rot):
    """Both datasets, training (rotated) and validation recipe, with colours: no host synchronisation, and the batch is the oracle's for
    the draws the docstring states -- the sampler's, then the angles."""
    from mvpnet_amd import augment as A
    from mvpnet_amd import chunks as CH
    from mvpnet_amd import scene as SC
    host, store = _store([9000, 6000, 12000], 41)
    rows = np.array([0, 1, 2, 1], np.int64)
    rows_t = t(rows)
    kw = dict(dataset=dataset, nb_pts=nb_pts, use_color=True, z_rot=z_rot, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2), chunk_thresh=0.3)
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    SC.sample_train_batch_3d(store, rows_t, generator=gen(), **kw)  # (the scratch exists from here on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        batch = SC.sample_train_batch_3d(store, rows_t, generator=gen(), **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert sorted(batch) == sorted(['points', 'seg_label', 'feature', 'choice'] + (['z_rot'] if z_rot else []))
    g = gen()
    if dataset == 'ScanNet3DChunks':
        draws = CH.sample_train_chunks(store['points'], store['seg_label'], store['scene_offsets'], rows_t, nb_pts, bounds_f64=True, generator=g)
        choice = TO.sample_chunks(host['points'], host['seg_label'], host['scene_offsets'], rows, draws['center_ind'].cpu().numpy(), nb_pts,
                                  seed=int(draws['seed'].item()), bounds_f64=True)['choice']
    else:
        draws = CH.sample_train_scenes(store['scene_offsets'], rows_t, nb_pts, generator=g)
        choice = SS.sample_scenes(host['scene_offsets'], rows, nb_pts, seed=int(draws['seed'].item()))[0]
    rot = None
    if z_rot:  # the angles are the generator's next draws; the device's float64 cos / sin may differ from numpy's in the last place, so
        # the matrices -- float64 values rounded once, entries at most 1 -- are held to 2^-23 and the batch to the oracle with ITS matrices
        u = torch.rand(4, dtype=torch.float64, generator=g, device=DEV).cpu().numpy()
        rot = batch['z_rot'].cpu().numpy()
        assert batch['z_rot'].dtype == torch.float32 and rot.shape == (4, 3, 3)
        assert np.abs(rot.astype(np.float64) - SS.z_rotation(z_rot[0] + (z_rot[1] - z_rot[0]) * u).astype(np.float64)).max() <= 2.0 ** -23
    hand = SS.gather_cloud(host['points'], host['scene_offsets'], rows, choice, seg_label=host['seg_label'], colors=host['colors'], rot=rot)
    hand['choice'] = choice
    for key, v in hand.items():
        got = batch[key].cpu().numpy()
        assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v), key


def test_scene_batch_with_colours_trains_pn2ssg():
    """A ScanNet3DScene batch with colours, B = 2, nb_pts one past a tile (a crop and a pad), through PN2SSG(in_channels=3) forward and
    backward: a finite loss, non-zero gradients."""
    from mvpnet_amd import scene as SC
    from mvpnet_amd.mvpnet3d import SegLoss
    from mvpnet_amd.pn2 import PN2SSG
    host, store = _store([9000, 8000], 51)
    batch = SC.sample_train_batch_3d(store, t(np.array([0, 1], np.int64)), dataset='ScanNet3DScene', nb_pts=TILE + 1, use_color=True,
                                     z_rot=(-np.pi, np.pi), generator=torch.Generator(device=DEV).manual_seed(2))
    assert tuple(batch['points'].shape) == (2, 3, TILE + 1) and tuple(batch['feature'].shape) == (2, 3, TILE + 1)
    torch.manual_seed(3)
    model = PN2SSG(3, 20, dropout_prob=0.0, num_centroids=(256, 64, 16, 4), radius=(0.1, 0.2, 0.4, 0.8), max_neighbors=(32, 32, 32, 32)).to(DEV).train()
    preds = model(batch)
    loss = SegLoss()(preds, batch)['seg_loss']
    loss.backward()
    assert tuple(preds['seg_logit'].shape) == (2, 20, TILE + 1) and torch.isfinite(loss)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_over_limit_arguments_raise_and_launch_nothing():
    import mvpnet_amd.ops as ops
    off, rows = t(offsets([100])), t(np.zeros(2, np.int64))
    with pytest.raises(RuntimeError):
        ops.sample_scenes(off, rows, 65537)
    with pytest.raises(RuntimeError):
        ops.sample_scenes(off, rows, 0)
    with pytest.raises(RuntimeError):
        ops.sample_scenes(off, rows, 64, Ntot=2 ** 31)
    with pytest.raises(RuntimeError):
        ops.sample_scenes(off, rows, 64, seed=torch.tensor([1]))  # a tensor seed lives on the device
    pts = t(np.zeros((100, 3), np.float32))
    with pytest.raises(RuntimeError):
        ops.gather_cloud(pts, off, rows, t(np.zeros((3, 8), np.int64)))  # B rows of choice
    with pytest.raises(RuntimeError):
        ops.gather_cloud(pts, off, rows, t(np.zeros((2, 8), np.int64)), colors=t(np.zeros((100, 3), np.float32)))
    with pytest.raises(RuntimeError):
        ops.gather_cloud(pts, off, rows, t(np.zeros((2, 8), np.int64)), rot=t(np.zeros((2, 3, 3), np.float64)))
    torch.cuda.synchronize()

"""Training chunks drawn on the MI355X: mvp_sample_chunks_f32 against the reference's own draws (tests/golden/train_sample.npz) and,
bit for bit, against the NumPy restatement (tests/train_sample_oracle.py); mvp_select_frames_ranges_u32 against one
chunks.select_frames call per chunk on the chunk's own frames; scene.sample_train_batch against the batch assembled by hand."""
import ctypes

import numpy as np
import pytest
import torch

from tests import scene_prep_oracle as SO
from tests import train_sample_oracle as TO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BLOCK = 256  # points per workgroup and tile of the counting / compaction passes (csrc/sample.hip, kSmpThreads)
KEYS = ('choice', 'points', 'seg_label', 'chunk_box', 'try_index', 'num_members')


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def concat(scenes):
    """[(points, label), ...] -> points (Ntot,3), label (Ntot,), scene_offsets (S+1,)"""
    off = np.concatenate([[0], np.cumsum([len(p) for p, _ in scenes])]).astype(np.int64)
    return np.concatenate([p for p, _ in scenes]).astype(np.float32), np.concatenate([l for _, l in scenes]).astype(np.int64), off


def both(scenes, scene_of_chunk, center_ind, nb_pts, base_point_ind=None, **kw):
    """the op and the oracle on the same arguments; asserts every output equal (NaN boxes: equal as NaN) -> (device dict, oracle dict)"""
    import mvpnet_amd.ops as ops
    points, label, off = concat(scenes)
    soc, ci = np.asarray(scene_of_chunk, np.int64), np.asarray(center_ind, np.int64)
    out = ops.sample_chunks(t(points), t(label), t(off), t(soc), t(ci), nb_pts, base_point_ind=None if base_point_ind is None else t(base_point_ind), **kw)
    exp = TO.sample_chunks(points, label, off, soc, ci, nb_pts, base_point_ind=base_point_ind, **kw)
    B = len(soc)
    assert out['choice'].dtype == torch.int64 and tuple(out['points'].shape) == (B, 3, nb_pts) and out['try_index'].dtype == torch.int32
    for key in KEYS:
        assert np.array_equal(out[key].cpu().numpy(), exp[key], equal_nan=key in ('chunk_box', 'points')), key
    if base_point_ind is not None:
        assert np.array_equal(out['base_bits'].cpu().numpy().view(np.uint32), exp['base_bits'])
    return out, exp


def random_scene(n, seed, extent=3.0, unlabelled=0.3):
    rs = np.random.RandomState(seed)
    pts = (rs.rand(n, 3) * extent).astype(np.float32)
    lab = rs.randint(0, 20, n).astype(np.int64)
    lab[rs.rand(n) < unlabelled] = -100
    return pts, lab


# ---- the reference's own draws ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixture(golden):
    return golden('train_sample')


@pytest.fixture(scope='module')
def cloud():
    points = TO.fixture_points()
    return [(points, TO.fixture_labels(points, kind)) for kind in TO.FIXTURE['label_kinds']]


@pytest.mark.parametrize('which', ['f32_2048', 'f32_8192', 'f64'])
def test_fixture_draws(fixture, cloud, which):
    """One scene per label array, one chunk per stored draw: try index, box, number of members and the member set are the reference's
    (the crop at 2048, pad and crop at 8192, the float64 bounds of the 3D loader); choice, points and labels are the oracle's."""
    P = TO.FIXTURE
    f64 = which == 'f64'
    nb_pts = 2048 if f64 else int(which[4:])
    rows = np.nonzero(fixture['f64'] if f64 else (fixture['nb_pts'] == nb_pts))[0]
    assert len(rows) == 18
    centers = np.maximum(fixture['centers'][rows], 0)  # tries behind the passing one were never drawn: any index will do
    out, exp = both(cloud, fixture['kind'][rows], centers, nb_pts, chunk_size=P['chunk_size'], chunk_margin=P['chunk_margin'],
                    chunk_thresh=P['chunk_thresh'], seed=2024, bounds_f64=f64)
    assert np.array_equal(out['try_index'].cpu().numpy(), fixture['try_index'][rows])
    assert np.array_equal(out['num_members'].cpu().numpy(), fixture['m'][rows])
    box, ref_box = out['chunk_box'].cpu().numpy(), fixture['box'][rows]
    defined = ~np.isnan(ref_box).all(1)
    assert defined.sum() >= 12 and np.array_equal(box[defined], ref_box[defined].astype(np.float32))
    choice = out['choice'].cpu().numpy()
    n = P['n_pts']
    crops = pads = 0
    for i, r in enumerate(rows):
        mask = np.unpackbits(fixture['mask_bits'][r], bitorder='little')[:n].astype(bool)
        m = int(mask.sum())
        assert mask[choice[i]].all()
        if m < nb_pts:
            pads += 1
            assert np.array_equal(choice[i, :m], np.nonzero(mask)[0])
        else:
            crops += 1
            assert len(np.unique(choice[i])) == nb_pts
    assert crops > 0 and (pads > 0 or nb_pts == 2048)


# ---- small shapes where it can go wrong ---------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7]


@pytest.fixture(scope='module')
def small_scenes():
    return [random_scene(n, 100 + n) for n in SIZES]


@pytest.mark.parametrize('nb_pts', [1, 64, 8192])
@pytest.mark.parametrize('T,thresh', [(3, 0.3), (1, 0.3), (3, 0.0), (3, 1.0)])
def test_small_scenes_in_one_batch(small_scenes, nb_pts, T, thresh):
    """Scenes of 1 ... 3 blocks + 7 points in one batch (seven workgroups per chunk: the segments' offsets are used), the largest scene
    by three chunks; nb_pts 1, 64 and the maximum (crops, `m == nb_pts` by chance aside, and pads); one try; thresholds 0 (the first
    non-empty try passes) and 1 (every member must be labelled, else the fallback)."""
    soc = list(range(len(SIZES))) + [len(SIZES) - 1] * 2
    rs = np.random.RandomState(nb_pts + T)
    ci = np.stack([rs.randint(0, SIZES[s], T) for s in soc])
    out, exp = both(small_scenes, soc, ci, nb_pts, chunk_size=(1.0, 1.0), chunk_margin=(0.2, 0.2), chunk_thresh=thresh, seed=nb_pts * 7 + T)
    tries = exp['try_index']
    if thresh == 0.0:
        assert (tries == 0).all()
    if thresh == 1.0:
        assert (tries == -1).any()
    if thresh == 0.3 and T == 3:
        assert (tries == 0).any()
    assert not np.array_equal(exp['choice'][-1], exp['choice'][-2]) or nb_pts == 1


def _cluster_scene(inside, outside, seed):
    """`inside` points within 0.1 m of (1, 1), the first of them exactly there, and `outside` points 50 m away"""
    rs = np.random.RandomState(seed)
    a = np.concatenate([[[1.0, 1.0]], 1.0 + rs.uniform(-0.1, 0.1, (inside - 1, 2))]) if inside > 1 else np.array([[1.0, 1.0]])
    b = 50.0 + rs.rand(outside, 2)
    xy = np.concatenate([a, b])
    perm = np.concatenate([[0], 1 + rs.permutation(len(xy) - 1)])  # the centre stays at index 0
    pts = np.concatenate([xy[perm], rs.rand(len(xy), 1)], 1).astype(np.float32)
    return pts, rs.randint(0, 20, len(pts)).astype(np.int64)


def test_member_counts_at_the_crop_pad_border():
    """m == nb_pts is a crop (a permutation of all members), m == nb_pts - 1 pads one slot, m == 1: every slot is that point"""
    nb = 64
    scenes = [_cluster_scene(nb, 300, 1), _cluster_scene(nb - 1, 300, 2), _cluster_scene(1, 300, 3)]
    out, exp = both(scenes, [0, 1, 2], [[0], [0], [0]], nb, chunk_thresh=0.0, seed=5)
    assert out['num_members'].tolist() == [nb, nb - 1, 1] and out['try_index'].tolist() == [0, 0, 0]
    choice = out['choice'].cpu().numpy()
    members0 = np.nonzero(exp['mask'][0])[0]
    assert np.array_equal(np.sort(choice[0]), members0) and not np.array_equal(choice[0], members0)
    assert np.array_equal(choice[1, :nb - 1], np.nonzero(exp['mask'][1])[0]) and exp['mask'][1][choice[1, -1]]
    assert (choice[2] == 0).all()


def test_all_labels_negative_falls_back():
    pts, lab = random_scene(700, 9)
    out, exp = both([(pts, np.full_like(lab, -100)), (pts, lab)], [0, 1, 0], [[5, 6, 7]] * 3, 128, chunk_size=(1.0, 1.0), seed=1)
    assert out['try_index'].tolist() == [-1, 0, -1] and out['num_members'].tolist()[0] == 700
    box = out['chunk_box'][0].cpu().numpy()
    m = np.float32(0.2)
    assert np.array_equal(box, np.hstack([pts[:, :2].min(0) - m, pts[:, :2].max(0) + m]))
    assert len(np.unique(out['choice'][0].cpu().numpy())) == 128  # a crop of the whole scene


def test_points_on_the_bounds_are_members():
    c = np.array([2.0, 2.0], np.float32)
    lo, hi = TO.try_box(c, (1.5, 1.5), (0.2, 0.2))
    below, above = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    xy = np.array([c, lo, hi, [lo[0], hi[1]], [hi[0], lo[1]], [below[0], 2.0], [2.0, below[1]], [above[0], 2.0], [2.0, above[1]],
                   [lo[0], 2.0], [2.0, hi[1]]], np.float32)
    pts = np.concatenate([xy, np.zeros((len(xy), 1), np.float32)], 1)
    out, exp = both([(pts, np.zeros(len(pts), np.int64))], [0], [[0]], 16, seed=3)
    assert np.array_equal(np.nonzero(exp['mask'][0])[0], [0, 1, 2, 3, 4, 9, 10])
    assert out['num_members'].tolist() == [7] and out['choice'][0, :7].tolist() == [0, 1, 2, 3, 4, 9, 10]
    assert np.array_equal(out['chunk_box'][0].cpu().numpy(), np.hstack([lo, hi]))


def test_nan_point_and_nan_centre():
    """A NaN coordinate is never a member of a try; a NaN centre makes its try empty and the next one is taken; in the fallback the NaN
    point is a member like every point and the box's bound is NaN (numpy.min)."""
    pts, lab = random_scene(500, 21)
    pts[17, 0] = np.nan
    pts[300, 1] = np.nan
    near = int(np.nanargmin(np.abs(pts[:, 0] - 1.5) + np.abs(pts[:, 1] - 1.5)))
    out, exp = both([(pts, lab), (pts, np.full_like(lab, -100))], [0, 0, 1], [[17, near, near], [300, 17, near], [near, near, near]], 600,
                    chunk_size=(1.0, 1.0), chunk_thresh=0.1, seed=8)
    assert out['try_index'].tolist() == [1, 2, -1]
    choice = out['choice'].cpu().numpy()
    assert 17 not in choice[0] and 300 not in choice[0]
    assert out['num_members'].tolist()[2] == 500 and np.array_equal(choice[2, :500], np.arange(500))
    assert np.isnan(out['chunk_box'][2].cpu().numpy()).all() and not np.isnan(out['chunk_box'][:2].cpu().numpy()).any()


def test_float64_bounds_disagree_with_float32_bounds():
    """Points one float32 step apart around both bounds: the float32 box (0.2f is not 0.2) and the float64 box admit different ones"""
    c = np.array([2.3, 1.7], np.float32)
    lo32, hi32 = TO.try_box(c, (1.5, 1.5), (0.2, 0.2), False)
    xs = [c[0]]
    for edge in (lo32[0], hi32[0]):
        x = np.float32(edge)
        for _ in range(4):
            x = np.nextafter(x, np.float32(-np.inf))
        for _ in range(9):
            xs.append(x)
            x = np.nextafter(x, np.float32(np.inf))
    pts = np.array([[x, c[1], 0.0] for x in xs], np.float32)
    lab = np.zeros(len(pts), np.int64)
    o32, e32 = both([(pts, lab)], [0], [[0]], 32, seed=1, bounds_f64=False)
    o64, e64 = both([(pts, lab)], [0], [[0]], 32, seed=1, bounds_f64=True)
    assert not np.array_equal(e32['mask'][0], e64['mask'][0]), 'the two arithmetics must disagree on this scene'
    assert o32['num_members'].tolist() != o64['num_members'].tolist()


# ---- base bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nbp', [37, 2000])
def test_base_bits(small_scenes, nbp):
    scenes = [random_scene(5000, 31), random_scene(1, 32), random_scene(2100, 33, unlabelled=1.0)]
    rs = np.random.RandomState(nbp)
    base = np.stack([rs.randint(0, len(p), nbp) for p, _ in scenes]).astype(np.int64)
    soc = [0, 1, 2, 0, 0]
    ci = np.stack([rs.randint(0, len(scenes[s][0]), 4) for s in soc])
    out, exp = both(scenes, soc, ci, 256, base_point_ind=base, chunk_size=(1.0, 1.0), seed=nbp)
    W = (nbp + 31) // 32
    assert tuple(out['base_bits'].shape) == (5, W) and out['base_bits'].dtype == torch.int32
    bits = out['base_bits'].cpu().numpy().view(np.uint32)
    for b, s in enumerate(soc):
        assert np.array_equal(SO.unpack_bits(bits[b:b + 1], nbp)[0], exp['mask'][b][base[s]])
    assert out['try_index'].tolist()[2] == -1 and SO.unpack_bits(bits[2:3], nbp).all()  # the fallback: every base point
    if nbp % 32:
        assert (bits[:, -1] >> np.uint32(nbp % 32) == 0).all(), 'padding bits stay zero'


# ---- ranged selection -----------------------------------------------------------------------------------------------------------------
def test_ranged_selection_equals_selection_on_the_slice():
    import mvpnet_amd.ops as ops
    from mvpnet_amd.chunks import select_frames
    rs = np.random.RandomState(12)
    nb, Ftot, n = 777, 300, 4
    ov = rs.rand(nb, Ftot) < 0.08
    ov[:, 7] = ov[:, 5]  # a tie inside a range: the lowest row wins
    begin = np.array([0, 1, 2, 12, 22, 2, 40, 299], np.int64)  # one-frame ranges, adjacent ranges, one range twice, the last row alone
    count = np.array([1, 1, 10, 10, 18, 10, 259, 1], np.int64)
    masks = rs.rand(len(begin), nb) < 0.3
    masks[5] = False  # an all-zero score: `begin`, pick after pick
    ov_t, mk_t = t(ov), t(masks)
    ov_bits = ops.pack_bits(ov_t.t())
    picked, gain = ops.select_frames_batched(ov_bits, mk_t, n, return_gain=True, frame_begin=t(begin), frame_count=t(count))
    epicked, egain = TO.select_frames_ranges(ov, masks, begin, count, n)
    assert picked.dtype == torch.int64 and np.array_equal(picked.cpu().numpy(), epicked) and np.array_equal(gain.cpu().numpy(), egain)
    for c in range(len(begin)):
        b, k = int(begin[c]), int(count[c])
        assert picked[c].tolist() == [b + f for f in select_frames(ov_t[mk_t[c]][:, b:b + k], n)], c
    assert (picked[5] == 2).all() and (gain[5] == 0).all() and (picked[0] == 0).all() and (picked[7] == 299).all()
    # the un-ranged entry on the same input: its old results
    old, old_gain = ops.select_frames_batched(ov_bits, mk_t, n, return_gain=True)
    eold, eold_gain = SO.select_frames_batched(ov, masks, n)
    assert np.array_equal(old.cpu().numpy(), eold) and np.array_equal(old_gain.cpu().numpy(), eold_gain)
    whole = ops.select_frames_batched(ov_bits, mk_t, n, frame_begin=t(np.zeros(8, np.int64)), frame_count=t(np.full(8, Ftot, np.int64)))
    assert torch.equal(whole, old)


# ---- reproducibility ------------------------------------------------------------------------------------------------------------------
def _repro_args():
    scenes = [random_scene(6000, 41), random_scene(900, 42)]
    points, label, off = concat(scenes)
    rs = np.random.RandomState(4)
    soc = np.array([0, 1, 0, 1], np.int64)
    ci = np.stack([rs.randint(0, len(scenes[s][0]), 5) for s in soc]).astype(np.int64)
    base = np.stack([rs.randint(0, len(p), 100) for p, _ in scenes]).astype(np.int64)
    return (points, label, off, soc, ci, base), [t(a) for a in (points, label, off, soc, ci)], t(base)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS + ('base_bits',))


def test_seeds_graph_and_no_host_synchronisation():
    import mvpnet_amd.ops as ops
    host, dev, base = _repro_args()
    kw = dict(chunk_size=(1.5, 1.5), base_point_ind=base)
    a = ops.sample_chunks(*dev, 512, seed=11, **kw)
    b = ops.sample_chunks(*dev, 512, seed=11, **kw)
    c = ops.sample_chunks(*dev, 512, seed=12, **kw)
    assert _same(a, b)
    assert torch.equal(a['try_index'], c['try_index']) and torch.equal(a['chunk_box'], c['chunk_box'])
    crop = (a['num_members'] >= 512).cpu().numpy()
    assert crop.any() and (~crop).any()
    for i in range(4):  # another seed: another crop, other pad repeats
        assert not torch.equal(a['choice'][i], c['choice'][i])
    exp = TO.sample_chunks(*host[:5], 512, chunk_size=(1.5, 1.5), seed=12, base_point_ind=host[5])
    assert np.array_equal(c['choice'].cpu().numpy(), exp['choice'])
    # a seed on the device gives the same draws as the same number from the host
    seed_t = torch.tensor([11], dtype=torch.int64, device=DEV)
    assert _same(ops.sample_chunks(*dev, 512, seed=seed_t, **kw), a)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        d = ops.sample_chunks(*dev, 512, seed=seed_t, **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert _same(d, a)
    # captured once, replayed: the same bits; a new seed in the seed tensor: the eager result for that seed
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = ops.sample_chunks(*dev, 512, seed=seed_t, **kw)
    for rep, (seed, want) in enumerate([(11, a), (11, a), (12, c)]):
        seed_t.fill_(seed)
        for v in r.values():
            v.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert _same(r, want), rep


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
CFG = dict(num_centroids=(256, 64, 16, 4), radius=(0.1, 0.2, 0.4, 0.8), max_neighbors=(32, 32, 32, 32))


class _Feature2D(torch.nn.Module):
    """Stands in for the 2D network: 16 feature channels that are fixed multiples of the image's three."""

    def forward(self, data):
        x = data['image']
        return {'feature': torch.cat([x * (0.25 * (i + 1)) for i in range(6)], 1)[:, :16].contiguous()}


def _store(nbp=300):
    import mvpnet_amd.ops as ops
    from mvpnet_amd.synthetic import make_rgbd_scene
    scs = [make_rgbd_scene(5 + i, F, n_pts=n, h=30, w=40) for i, (F, n) in enumerate([(12, 9000), (7, 6000), (16, 8000)])]
    rs = np.random.RandomState(77)
    labels = [TO.fixture_labels(sc['points'], kind, seed=i) for i, (sc, kind) in enumerate(zip(scs, ['dense', 'patchy', 'sparse']))]
    points, label, off = concat([(sc['points'], l) for sc, l in zip(scs, labels)])
    base = np.stack([rs.choice(len(sc['points']), nbp, replace=False) for sc in scs]).astype(np.int64)
    overlaps = [SO.rgbd_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], sc['points'][b], 0.1) for sc, b in zip(scs, base)]  # (nbp,F) each
    foff = np.concatenate([[0], np.cumsum([len(sc['pose']) for sc in scs])]).astype(np.int64)
    Ftot = int(foff[-1])
    host = dict(points=points, seg_label=label, scene_offsets=off, base_point_ind=base, overlaps=np.concatenate(overlaps, 1), frame_offsets=foff,
                depth=np.concatenate([sc['depth_mm'] for sc in scs]).astype(np.int16), pose=np.concatenate([sc['pose'] for sc in scs]),
                images=np.random.RandomState(8).standard_normal((Ftot, 3, 30, 40)).astype(np.float32),
                cam=np.stack([sc['cam_matrix'][:3, :3] for sc in scs]), kinv=np.stack([sc['kinv'] for sc in scs]))
    store = {k: t(v) for k, v in host.items() if k != 'overlaps'}
    store['overlap_bits'] = ops.pack_bits(t(host['overlaps']).t())
    return host, store


def test_sample_train_batch_equals_the_hand_assembled_batch():
    from mvpnet_amd import chunks as CH
    from mvpnet_amd import scene as SC
    from mvpnet_amd.pn2 import PN2SSG
    from mvpnet_amd.mvpnet3d import MVPNet3D, SegLoss
    host, store = _store()
    soc = np.array([0, 1, 2, 1, 0], np.int64)
    kw = dict(nb_pts=1024, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2), chunk_thresh=0.3)
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    soc_t = t(soc)
    draws = CH.sample_train_chunks(store['points'], store['seg_label'], store['scene_offsets'], soc_t, generator=gen(), **kw)
    SC.sample_train_batch(store, soc_t, num_rgbd_frames=3, k=3, generator=gen(), **kw)  # (the scratch exists from here on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        batch = SC.sample_train_batch(store, soc_t, num_rgbd_frames=3, k=3, generator=gen(), **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert sorted(batch) == sorted(['images', 'points', 'seg_label', 'depth', 'cam_matrix', 'kinv', 'pose', 'k', 'pixel_box'])
    ci = draws['center_ind'].cpu().numpy()
    n_of = np.diff(host['scene_offsets'])[soc]
    assert ci.shape == (5, 10) and (ci >= 0).all() and (ci < n_of[:, None]).all()
    exp = TO.sample_chunks(host['points'], host['seg_label'], host['scene_offsets'], soc, ci, 1024, seed=int(draws['seed'].item()),
                           base_point_ind=host['base_point_ind'], **{k: v for k, v in kw.items() if k != 'nb_pts'})
    assert (exp['try_index'] == -1).any() and (exp['try_index'] >= 0).any()
    picks = []
    for b, s in enumerate(soc):  # one chunks.select_frames call per chunk on the frames of its own scene
        f0, f1 = int(host['frame_offsets'][s]), int(host['frame_offsets'][s + 1])
        ov = t(host['overlaps'][:, f0:f1][exp['mask'][b][host['base_point_ind'][s]]])
        picks.append([f0 + f for f in CH.select_frames(ov, 3)])
    sel = torch.tensor(picks, device=DEV)
    m = np.float32(0.1)
    box = exp['chunk_box']
    hand = {'images': store['images'][sel].contiguous(), 'points': t(exp['points']), 'seg_label': t(exp['seg_label']),
            'depth': store['depth'][sel].contiguous(), 'cam_matrix': t(host['cam'][soc][:, None].repeat(3, 1)),
            'kinv': t(host['kinv'][soc][:, None].repeat(3, 1)), 'pose': store['pose'][sel].contiguous(),
            'pixel_box': t(np.concatenate([box[:, :2] - m, box[:, 2:] + m], 1)), 'k': 3}
    for key, v in hand.items():
        if key == 'k':
            assert batch[key] == v
        else:
            assert batch[key].dtype == v.dtype and batch[key].shape == v.shape and torch.equal(batch[key], v), key
    torch.manual_seed(3)
    model = MVPNet3D(_Feature2D(), '', PN2SSG(16, 20, dropout_prob=0.0, **CFG), in_channels=16, mlp_channels=(16, 16, 16)).to(DEV).train()
    loss_fn = SegLoss()
    res = []
    for data in (batch, hand):
        preds = model(dict(data))
        res.append((preds['seg_logit'].detach().clone(), loss_fn(preds, data)['seg_loss'].detach().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1])


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_over_limit_arguments_return_the_error_code_and_launch_nothing():
    import mvpnet_amd.ops as ops
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)

    def entry(T, nb_pts, Ntot=1000, B=2):
        return lib.mvp_sample_chunks_f32(d, d, d, d, d, None, Ntot, 1, B, T, 0, nb_pts, 1.5, 1.5, 0.2, 0.2, 0.3, 0, 0, None, d, d, d, d, d, d,
                                         None, d, 1 << 40, None)
    assert entry(10, 8193) == -2 and entry(33, 2048) == -2 and entry(10, 2048, Ntot=2 ** 31) == -2   # MVP_EUNSUPPORTED
    assert entry(0, 2048) == -1 and entry(10, 0) == -1                                                # MVP_EINVAL
    assert lib.mvp_sample_chunks_workspace(1000, 2, 33, 2048) == 0 and lib.mvp_sample_chunks_workspace(1000, 2, 10, 8192) > 0
    assert lib.mvp_select_frames_ranges_u32(d, d, d, d, 0, 4, 8, 3, d, None, None) == -1              # no frame at all
    assert lib.mvp_select_frames_ranges_u32(d, d, None, d, 5, 4, 8, 3, d, None, None) == -3
    assert lib.mvp_select_frames_ranges_u32(d, d, d, d, 5, 4, 1025, 3, d, None, None) == -2
    pts, lab = random_scene(100, 1)
    args = [t(pts), t(lab), t(np.array([0, 100], np.int64)), t(np.zeros(2, np.int64))]
    with pytest.raises(RuntimeError):
        ops.sample_chunks(*args, t(np.zeros((2, 10), np.int64)), 8193)
    with pytest.raises(RuntimeError):
        ops.sample_chunks(*args, t(np.zeros((2, 33), np.int64)), 2048)
    ov, mk = t(np.ones((40, 6), bool)), t(np.ones((2, 40), bool))
    with pytest.raises(RuntimeError):  # host-known ranges are checked before the launch
        ops.select_frames_batched(ov, mk, 3, frame_begin=torch.tensor([0, 3]), frame_count=torch.tensor([3, 0]))
    # ranges on the device cannot be read without a synchronisation: a chunk without frames is answered with -1 and reads no row
    picked, gain = ops.select_frames_batched(ov, mk, 3, return_gain=True, frame_begin=t(np.array([0, 3], np.int64)), frame_count=t(np.array([3, 0], np.int64)))
    assert picked.tolist() == [[0, 0, 0], [-1, -1, -1]] and gain[1].tolist() == [0, 0, 0]

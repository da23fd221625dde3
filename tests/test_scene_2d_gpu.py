"""scene.infer_scene_2d on the MI355X: the whole-scene test of the 2D baseline with every distinct frame through the 2D network once and
lift + vote in one launch, against the loop it replaces (MVPNet2D per chunk with B = 1 on the scene batcher's dicts, then dist.vote_scene)
on the ragged end-to-end scene of tests/test_scene_prep_gpu.py, and against the committed reference fixture (tests/golden/scene_2d.npz)."""
import numpy as np
import pytest
import torch

from tests import lift_vote_oracle as LO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
E2E = dict(n_frames=24, n_pts=24000, h=30, w=40, num_base_pts=700,
           chunk=dict(chunk_size=(1.5, 1.5), chunk_stride=1.0, chunk_thresh=300, chunk_margin=(0.2, 0.2)))
NV = 3


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class StandIn2D(torch.nn.Module):
    """Stands in for the 2D network: 20 class logits from the three image channels, (x0*w0 + x1*w1) + x2*w2 with separate elementwise
    operations -- each its own kernel, each rounding once, so neither the batch size nor the memory layout can change a bit.  Counts the
    images it is given."""
    num_classes = LO.STANDIN_CLASSES

    def __init__(self):
        super().__init__()
        self.w = t(LO.standin_weights())
        self.seen = 0

    def forward(self, data):
        x = data['image']
        self.seen += x.size(0)
        planes = []
        for c in range(self.w.size(1)):
            a = x[:, 0] * self.w[0, c]
            b = x[:, 1] * self.w[1, c]
            planes.append((a + b) + x[:, 2] * self.w[2, c])
        return {'seg_logit': torch.stack(planes, 1)}


def _model():
    from mvpnet_amd.mvpnet2d import MVPNet2D
    return MVPNet2D(StandIn2D()).to(DEV)


@pytest.fixture(scope='module')
def scene():
    from mvpnet_amd.synthetic import make_rgbd_scene
    sc = make_rgbd_scene(3, E2E['n_frames'], n_pts=E2E['n_pts'], h=E2E['h'], w=E2E['w'])
    F, h, w = sc['depth_mm'].shape
    images = np.random.RandomState(8).standard_normal((F, 3, h, w)).astype(np.float32)
    return dict(sc=sc, images=t(images), images_np=images, pts=t(sc['points']), depth=t(sc['depth_mm'].astype(np.int16)), pose=t(sc['pose']))


def _kw(k):
    return dict(num_rgbd_frames=NV, k=k, num_base_pts=E2E['num_base_pts'], **E2E['chunk'])


def _chunk_loop(model, s, k, images=None, **extra):
    """The loop infer_scene_2d replaces: the existing MVPNet2D on one chunk at a time (B = 1, all its points, its own three frames), the
    per-chunk logits voted by dist.vote_scene.  -> (mean, label, count), csr (the chunks, with their picked frames)."""
    from mvpnet_amd import scene as S
    from mvpnet_amd import dist as D
    sc, pts = s['sc'], s['pts']
    images = s['images'] if images is None else images
    csr = S._scene_chunks(pts, s['depth'], sc['cam_matrix'], s['pose'], None, NV, E2E['chunk']['chunk_size'], E2E['chunk']['chunk_stride'],
                          E2E['chunk']['chunk_thresh'], E2E['chunk']['chunk_margin'], E2E['num_base_pts'], 0.1, torch.Generator(device=DEV).manual_seed(7))
    batch = S._scene_batcher(DEV, s['depth'], sc['cam_matrix'], s['pose'], images, None, 'test', k, **extra)
    chunk_inds = list(torch.split(csr['index'], csr['lengths']))
    width = max(csr['lengths'])
    logits = torch.zeros((len(chunk_inds), LO.STANDIN_CLASSES, width), device=DEV)
    model.eval()
    with torch.no_grad():
        for c, ind in enumerate(chunk_inds):
            out = model(batch(csr['picked'][c:c + 1], pts[ind].t().contiguous()[None], csr['pixel_box'][c:c + 1]))['seg_logit']
            logits[c, :, :ind.numel()] = out[0]
    return D.vote_scene(logits, chunk_inds, pts.size(0)), csr


def _f64(s, csr, k):
    """The float64 evaluation of the scene (tests/lift_vote_oracle.py) from the device's own chunks, frames and k-NN indices."""
    import mvpnet_amd.ops as ops
    from mvpnet_amd import scene as S
    sc, pts = s['sc'], s['pts']
    batch = S._scene_batcher(DEV, s['depth'], sc['cam_matrix'], s['pose'], s['images'], None, 'test', k)
    chunk_inds = [i.cpu().numpy() for i in torch.split(csr['index'], csr['lengths'])]
    picked = csr['picked'].cpu().numpy()
    frames = np.unique(picked)
    rows = []
    for c, ind in enumerate(torch.split(csr['index'], csr['lengths'])):
        d = batch(csr['picked'][c:c + 1], pts[ind].t().contiguous()[None], csr['pixel_box'][c:c + 1])
        xyz, mask = ops.unproject(d['depth'], d['kinv'], d['pose'], d['pixel_box'])
        rows.append(ops.pixel_knn(xyz, mask, pts[ind][None].contiguous(), k, cam=d['cam_matrix'], pose=d['pose'])[0].cpu().numpy())
    lengths = np.array(csr['lengths'], np.int64)
    F, C, h, w = len(frames), LO.STANDIN_CLASSES, E2E['h'], E2E['w']
    store = LO.standin_logits(s['images_np'][frames]).reshape(F, C, h * w).transpose(0, 2, 1)
    return LO.lift_vote_f64(store, np.searchsorted(frames, picked), np.concatenate(rows), np.concatenate([[0], np.cumsum(lengths)[:-1]]), chunk_inds,
                            pts.size(0)), frames


@pytest.fixture(scope='module')
def loops(scene):
    """The per-chunk loop's results for k = 1 and k = 3, computed once."""
    out = {}
    for k in (1, 3):
        model = _model()
        (mean, label, count), csr = _chunk_loop(model, scene, k)
        out[k] = dict(mean=mean, label=label, count=count, csr=csr, seen=model.net_2d.seen)
    return out


def _run(scene, k, model=None, **kw):
    from mvpnet_amd.scene import infer_scene_2d
    model = _model() if model is None else model
    s = scene
    args = dict(_kw(k), generator=torch.Generator(device=DEV).manual_seed(7))
    args.update(kw)
    images = args.pop('images', s['images'])
    return infer_scene_2d(model, s['pts'], s['depth'], s['sc']['cam_matrix'], s['pose'], images, **args), model


def test_k1_equals_the_chunk_loop_bit_for_bit(scene, loops):
    ref = loops[1]
    csr = ref['csr']
    picked = csr['picked'].cpu().numpy()
    assert len(csr['lengths']) == 42 and len(set(csr['lengths'])) > 30, 'ragged chunks'
    assert any((p == 0).all() for p in picked), 'a chunk no frame sees'
    model = _model().train()
    (mean, label, count), _ = _run(scene, 1, model=model)
    assert model.training, 'the mode is restored'
    assert torch.equal(count, ref['count']) and torch.equal(label, ref['label'])
    assert torch.equal(mean.view(torch.int32), ref['mean'].view(torch.int32))
    distinct = len(np.unique(picked))
    assert model.net_2d.seen == distinct < 42 * NV == ref['seen'], 'every distinct picked frame goes through the 2D network once'
    assert int(count.max()) > 1 and int((count > 0).sum()) > count.numel() // 2 and bool((label[count == 0] == LO.STANDIN_CLASSES).all())
    assert bool((mean[count == 0] == 0).all()) and bool(torch.isfinite(mean).all())   # (points in no chunk: the fixture's scene has them)


def test_k3_lies_within_the_rounding_bound_of_float64_like_the_chunk_loop(scene, loops):
    ref = loops[3]
    (mean, label, count), model = _run(scene, 3, frame_batch=5)   # several forwards, the last one partial
    assert torch.equal(count, ref['count'])
    (total64, scale, count64), frames = _f64(scene, ref['csr'], 3)
    assert np.array_equal(count64, count.cpu().numpy()) and model.net_2d.seen == len(frames) < 42 * NV
    for name, r in (('infer_scene_2d', (mean, label)), ('chunk loop', (ref['mean'], ref['label']))):
        worst, excluded = LO.check_against_f64(r[0].cpu().numpy(), r[1].cpu().numpy(), count64, total64, scale, 3)
        print('%s: worst error / bound %.3f, %.5f of the voted points excluded from the label comparison' % (name, worst, excluded))
    sure = torch.from_numpy(count64 > 0).to(DEV)
    print('labels equal to the chunk loop on %.4f of the voted points' % float((label[sure] == ref['label'][sure]).float().mean()))


def test_raw_frames_and_a_given_overlap(scene, loops):
    """Raw uint8 frames + image_normalizer go through ops.prepare_frames (the loop's _picked_views does the same per chunk): k = 1 is
    bit-equal again; overlap= given as the computation's own result changes nothing."""
    import mvpnet_amd.chunks as CH
    s = scene
    raw = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (E2E['n_frames'], E2E['h'], E2E['w'], 3)).astype(np.uint8)).to(DEV)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    (emean, elabel, ecount), _ = _chunk_loop(_model(), s, 1, images=raw, image_normalizer=norm)
    (mean, label, count), model = _run(s, 1, images=raw, image_normalizer=norm, frame_batch=7)
    assert torch.equal(mean.view(torch.int32), emean.view(torch.int32)) and torch.equal(label, elabel) and torch.equal(count, ecount)
    assert not torch.equal(mean, loops[1]['mean'])
    with pytest.raises(RuntimeError):
        _run(s, 1, image_normalizer=norm)   # float images are final
    given = CH.compute_rgbd_overlap(s['pts'], s['depth'], s['sc']['cam_matrix'], s['pose'], num_base_pts=E2E['num_base_pts'], radius=0.1,
                                    generator=torch.Generator(device=DEV).manual_seed(7), packed=True)
    (mean, label, count), _ = _run(s, 1, overlap=given, generator=None)
    assert torch.equal(mean.view(torch.int32), loops[1]['mean'].view(torch.int32)) and torch.equal(label, loops[1]['label']) and torch.equal(count, loops[1]['count'])


def test_a_scene_without_a_kept_window_takes_the_empty_path(scene):
    model = _model()
    (mean, label, count), _ = _run(scene, 3, model=model, chunk_thresh=10 ** 6)
    n = scene['pts'].size(0)
    assert tuple(mean.shape) == (n, LO.STANDIN_CLASSES) and not mean.any() and not count.any() and count.dtype == torch.int32
    assert bool((label == LO.STANDIN_CLASSES).all()) and model.net_2d.seen == 0

    class Silent2D(StandIn2D):   # a 2D network that does not say how many classes it has: one frame is run to learn it
        num_classes = None

    other = torch.nn.Module()
    other.net_2d = Silent2D()
    (mean, label, _), _ = _run(scene, 3, model=other, chunk_thresh=10 ** 6)
    assert mean.size(1) == LO.STANDIN_CLASSES and other.net_2d.seen == 1 and bool((label == LO.STANDIN_CLASSES).all())


def test_against_the_reference_fixture(golden):
    """infer_scene_2d(overlap=the fixture's) on the fixture's scene: the reference's picked frames and counts, its mean logits within the
    rounding bound of the float64 evaluation, its labels wherever the float64 top-two gap exceeds twice the bound."""
    from mvpnet_amd.scene import infer_scene_2d
    from mvpnet_amd import scene as S
    g = golden('scene_2d')
    g = {k: g[k] for k in g.files}
    P = LO.FIXTURE
    sc, store, view_frame, knn, knn_base, chunk_inds, frames = LO.fixture_inputs(g)
    overlaps = np.unpackbits(g['overlaps'], axis=1)[:, :P['n_frames']].astype(bool)
    given = (t(g['base_point_ind'].astype(np.int64)), t(overlaps))
    chunk = dict(chunk_size=P['chunk_size'], chunk_stride=P['chunk_stride'], chunk_thresh=P['chunk_thresh'], chunk_margin=P['chunk_margin'])
    pts, depth, pose = t(sc['points']), t(sc['depth_mm'].astype(np.int16)), t(sc['pose'])
    csr = S._scene_chunks(pts, depth, sc['cam_matrix'], pose, given, P['num_rgbd_frames'], P['chunk_size'], P['chunk_stride'], P['chunk_thresh'],
                          P['chunk_margin'], P['num_base_pts'], P['radius'], None)
    assert csr['lengths'] == g['lengths'].tolist() and np.array_equal(csr['picked'].cpu().numpy(), g['picked'])
    assert np.array_equal(csr['index'].cpu().numpy(), g['chunk_index'])
    model = _model()
    mean, label, count = infer_scene_2d(model, pts, depth, sc['cam_matrix'], pose, t(sc['images']), overlap=given, num_rgbd_frames=P['num_rgbd_frames'],
                                        k=P['k'], **chunk)
    assert model.net_2d.seen == len(frames) < g['picked'].size
    assert np.array_equal(count.cpu().numpy(), g['count'].astype(np.int32))
    total64, scale, count64 = LO.lift_vote_f64(store, view_frame, knn, knn_base, chunk_inds, P['n_pts'])
    worst, excluded = LO.check_against_f64(mean.cpu().numpy(), label.cpu().numpy(), count64, total64, scale, P['k'])
    LO.check_against_f64(g['mean'], g['label'].astype(np.int64), count64, total64, scale, P['k'])
    print('worst error / bound %.3f, excluded %.5f; bit-equal to the reference on %.4f of the elements' % (
        worst, excluded, float((mean.cpu().numpy() == g['mean']).mean())))

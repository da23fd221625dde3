"""scene.infer_scene_shared on the MI355X: the whole-scene test of MVPNet with every distinct frame through the 2D network once per store,
against the path it restates -- infer_scene on prepare_scene_bucketed's batches -- on the ragged end-to-end scene of
tests/test_scene_prep_gpu.py (42 chunks x 3 views): bit for bit, with a stand-in 2D network that is elementwise (its bits do not depend on
the batch size) and counts the images it is given."""
import numpy as np
import pytest
import torch

from tests.test_scene_prep_gpu import E2E, _Feature2D, _model as _prep_model

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NV, CHUNKS = 3, 42
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Counting2D(_Feature2D):
    def __init__(self):
        super().__init__()
        self.seen = 0

    def forward(self, data):
        self.seen += data['image'].size(0)
        return super().forward(data)


def _model():
    model = _prep_model()  # (same seed, same weights every time)
    model.net_2d = _Counting2D()
    return model


@pytest.fixture(scope='module')
def scene():
    from mvpnet_amd.synthetic import make_rgbd_scene
    sc = make_rgbd_scene(3, E2E['n_frames'], n_pts=E2E['n_pts'], h=E2E['h'], w=E2E['w'])
    F, h, w = sc['depth_mm'].shape
    images = np.random.RandomState(8).standard_normal((F, 3, h, w)).astype(np.float32)
    raw = np.random.RandomState(9).randint(0, 256, (F, h, w, 3)).astype(np.uint8)
    return dict(sc=sc, images=t(images), raw=t(raw), pts=t(sc['points']), depth=t(sc['depth_mm'].astype(np.int16)), pose=t(sc['pose']))


def _kw(**extra):
    kw = dict(num_rgbd_frames=NV, k=3, min_nb_pts=E2E['min_nb_pts'], num_base_pts=E2E['num_base_pts'], batch_size=8, pad_seed=11,
              generator=torch.Generator(device=DEV).manual_seed(7), **E2E['chunk'])
    kw.update(extra)
    return kw


def _parent(s, images, **extra):
    """The path infer_scene_shared restates -> (mean, label, count), frames the 2D network saw, the batches."""
    from mvpnet_amd.scene import prepare_scene_bucketed, infer_scene
    model = _model()
    prepared = prepare_scene_bucketed(s['pts'], s['depth'], s['sc']['cam_matrix'], s['pose'], images, **_kw(**extra))
    return infer_scene(model, *prepared[:3]), model.net_2d.seen, prepared[0]


def _shared(s, images, model=None, **extra):
    from mvpnet_amd.scene import infer_scene_shared
    model = _model() if model is None else model
    return infer_scene_shared(model, s['pts'], s['depth'], s['sc']['cam_matrix'], s['pose'], images, **_kw(**extra)), model.net_2d.seen


@pytest.fixture(scope='module')
def parent(scene):
    """The parent path's result on the float images, computed once."""
    out, seen, batches = _parent(scene, scene['images'])
    assert seen == CHUNKS * NV and sum(b['points'].size(0) for b in batches) == CHUNKS
    return dict(out=out, batches=batches)


def _distinct(s):
    """Number of distinct frames the scene's chunks picked."""
    from mvpnet_amd import scene as S
    csr = S._scene_chunks(s['pts'], s['depth'], s['sc']['cam_matrix'], s['pose'], None, NV, E2E['chunk']['chunk_size'], E2E['chunk']['chunk_stride'],
                          E2E['chunk']['chunk_thresh'], E2E['chunk']['chunk_margin'], E2E['num_base_pts'], 0.1, torch.Generator(device=DEV).manual_seed(7))
    assert len(csr['lengths']) == CHUNKS
    return int(torch.unique(csr['picked']).numel())


def _assert_equal(got, want):
    for name, a, b in zip(('mean logits', 'labels', 'counts'), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name


def test_equal_to_infer_scene_on_the_bucketed_batches_with_every_frame_once(scene, parent):
    model = _model().train()
    got, seen = _shared(scene, scene['images'], model=model)
    _assert_equal(got, parent['out'])
    distinct = _distinct(scene)
    assert seen == distinct < CHUNKS * NV
    assert model.training, 'the mode is restored'
    mean, label, count = got
    assert int((count > 0).sum()) > scene['pts'].size(0) // 2 and bool(torch.isfinite(mean).all()) and count.dtype == torch.int32
    got, seen = _shared(scene, scene['images'], model=model.eval(), frame_batch=5)  # the 2D batch size changes nothing
    _assert_equal(got, parent['out'])
    assert seen == 2 * distinct and not model.training


def test_a_capped_store_runs_in_several_groups_with_the_same_result(scene, parent, monkeypatch):
    from mvpnet_amd import scene as S
    plans = []
    plan = S.plan_store_groups
    monkeypatch.setattr(S, 'plan_store_groups', lambda frames, cap: plans.append((plan(frames, cap), cap)) or plans[-1][0])
    h, w, C = E2E['h'], E2E['w'], 16
    got, seen = _shared(scene, scene['images'], max_store_bytes=5 * h * w * C * 4 + 100)
    _assert_equal(got, parent['out'])  # the batch plan does not depend on the cap
    (runs, cap), = plans
    assert cap == 5 and len(runs) > 1 and runs[-1][1] == len(parent['batches'])
    assert all(len(frames) <= 5 or hi - lo == 1 for lo, hi, frames in runs)
    assert seen == sum(len(frames) for _, _, frames in runs), 'every run puts its distinct frames through the 2D network once'
    assert _distinct(scene) < seen < CHUNKS * NV


def test_raw_frames_with_a_normalizer(scene):
    want, seen_parent, _ = _parent(scene, scene['raw'], image_normalizer=NORM)
    got, seen = _shared(scene, scene['raw'], image_normalizer=NORM, frame_batch=7)
    _assert_equal(got, want)
    assert seen < seen_parent == CHUNKS * NV
    with pytest.raises(RuntimeError):
        _shared(scene, scene['images'], image_normalizer=NORM)  # float images are final


def test_a_scene_without_a_kept_window(scene):
    model = _model()
    (mean, label, count), seen = _shared(scene, scene['images'], model=model, chunk_thresh=10 ** 6)
    n, C = scene['pts'].size(0), 20
    assert tuple(mean.shape) == (n, C) and mean.dtype == torch.float32 and not mean.any()
    assert tuple(label.shape) == (n,) and label.dtype == torch.int64 and bool((label == C).all())
    assert tuple(count.shape) == (n,) and count.dtype == torch.int32 and not count.any()
    assert seen == 0


def test_a_2d_network_with_another_output_is_refused(scene):
    class Half(_Counting2D):
        def forward(self, data):
            return {'feature': super().forward(data)['feature'].half()}

    class Small(_Counting2D):
        def forward(self, data):
            return {'feature': super().forward(data)['feature'][:, :, ::2, ::2].contiguous()}

    for net_2d in (Half(), Small()):
        model = _model()
        model.net_2d = net_2d
        with pytest.raises(RuntimeError):
            _shared(scene, scene['images'], model=model)
        assert not model.training


def test_a_store_batch_handed_to_the_model_directly(scene, parent):
    """feature_store / view_slot in place of images: no net_2d call, the same seg_logit."""
    model = _model()
    batch = next(b for b in parent['batches'] if b['points'].size(0) > 1)
    B, nv = batch['depth'].shape[:2]
    with torch.no_grad():
        want = model(dict(batch))['seg_logit']
        assert model.net_2d.seen == B * nv
        # every view's map in a store of its own slot, shuffled; then the same batch through the store
        feat = model.net_2d({'image': batch['images'].reshape(B * nv, *batch['images'].shape[2:])})['feature']
        perm = torch.randperm(B * nv, generator=torch.Generator().manual_seed(2)).to(DEV)
        store = feat.permute(0, 2, 3, 1).contiguous()[perm]
        view_slot = torch.argsort(perm).to(torch.int32).view(B, nv)
        seen = model.net_2d.seen
        shared = {key: v for key, v in batch.items() if key != 'images'}
        got = model(dict(shared, feature_store=store, view_slot=view_slot))['seg_logit']
    assert model.net_2d.seen == seen, 'a store batch does not run the 2D network'
    assert torch.equal(got, want)

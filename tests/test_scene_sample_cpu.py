"""The definitions of mvp_sample_scenes_f32 and mvp_gather_cloud_f32 are the reference's: tests/scene_sample_oracle.py against what
`ScanNet3DScene.__getitem__` with `CropPad` + `RandomRotateZ` returned for the fixture cloud (tests/golden/scene_sample.npz, written by
tests/golden/make_scene_sample_golden.py from the reference itself); the laws of the crop and the pad; the refused shapes; the config
helper on the four 3D-baseline YAMLs (tests/golden/configs_3d.json).  No GPU, no kernel."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import scene_sample_oracle as SS
from tests.conftest import GOLDEN


@pytest.fixture(scope='module')
def fixture(golden):
    return golden('scene_sample')


@pytest.fixture(scope='module')
def cloud():
    return SS.fixture_cloud()


def test_features_are_the_reference_bits(fixture, cloud):
    points, colors, label = cloud
    out = SS.gather_cloud(points, np.array([0, len(points)]), np.array([0]), np.arange(len(points))[None], colors=colors)
    assert out['feature'].dtype == np.float32 and np.array_equal(out['feature'][0].T, fixture['feature'])
    assert len(np.unique(colors)) == 256, 'every uint8 value is divided once'


def test_rotation_matrices_are_within_one_rounding_of_scipy(fixture):
    """Both are float64 values rounded once to float32, entries at most 1 in magnitude: within 2^-23.  The formula is
    augment.z_rotation_from_angle's, the oracle restates it; further angles against scipy itself."""
    from mvpnet_amd import augment as A
    angle, ref = fixture['angle'], fixture['rot']
    assert ref.dtype == np.float32 and ref.shape == (SS.FIXTURE['angles'], 3, 3) and np.array_equal(angle, SS.fixture_angles())
    ours = A.z_rotation_from_angle(torch.from_numpy(angle)).numpy()
    assert ours.dtype == np.float32 and np.array_equal(ours, SS.z_rotation(angle))
    worst = float(np.abs(ours.astype(np.float64) - ref.astype(np.float64)).max())
    print('fixture angles: largest |ours - reference| = %g (2^-23 = %g)' % (worst, 2.0 ** -23))
    assert worst <= 2.0 ** -23
    from scipy.spatial.transform import Rotation
    more = np.random.RandomState(3).uniform(-np.pi, np.pi, 2000)
    sp = np.stack([Rotation.from_rotvec(a * np.array([0., 0., 1.], np.float32)).as_matrix().astype(np.float32) for a in more])
    worst = float(np.abs(SS.z_rotation(more).astype(np.float64) - sp.astype(np.float64)).max())
    print('2000 angles: largest |ours - scipy| = %g' % worst)
    assert worst <= 2.0 ** -23


def test_rotated_points_are_within_the_dot_product_bound(fixture, cloud):
    """|ours - reference| <= 6 * 2^-24 * (|x| + |y| + |z|): twice the error bound of a three-term float32 dot product with coefficients
    of magnitude at most 1, whatever order or fusing the reference's BLAS used.  With the reference's own matrices."""
    points = cloud[0]
    bound = 6.0 * 2.0 ** -24 * np.abs(points.astype(np.float64)).sum(1)
    worst = 0.0
    for R, ref in zip(fixture['rot'], fixture['rotated']):
        ours = SS.rotate(points, R)
        assert ours.dtype == np.float32
        err = np.abs(ours.astype(np.float64) - ref.astype(np.float64)).max(1)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all()
    print('rotated points: largest error / bound = %.3f' % worst)
    # the gather applies it per row, channel-major
    out = SS.gather_cloud(points, np.array([0, len(points)]), np.array([0, 0]), np.stack([np.arange(len(points))] * 2), rot=fixture['rot'][:2])
    assert np.array_equal(out['points'][1].T, SS.rotate(points, fixture['rot'][1]))


def test_draw_z_rotation_law():
    from mvpnet_amd import augment as A
    g = torch.Generator().manual_seed(7)
    R = A.draw_z_rotation(4000, device='cpu', generator=g)
    assert R.dtype == torch.float32 and tuple(R.shape) == (4000, 3, 3) and R.is_contiguous()
    u = torch.rand(4000, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    angle = -math.pi + (math.pi - -math.pi) * u
    assert np.array_equal(R.numpy(), SS.z_rotation(angle.numpy()))
    assert abs(float(angle.mean())) < 0.15 and float(angle.min()) < -3.0 and float(angle.max()) > 3.0  # uniform on [-pi, pi)
    assert torch.equal(R[:, 2], torch.tensor([0., 0., 1.]).expand(4000, 3)) and torch.equal(R[:, 0, 0], R[:, 1, 1]) and torch.equal(R[:, 0, 1], -R[:, 1, 0])
    R2 = A.draw_z_rotation((2, 3), 0.25, 0.5, device='cpu', generator=g)
    a2 = torch.atan2(R2[..., 1, 0], R2[..., 0, 0])
    assert tuple(R2.shape) == (2, 3, 3, 3) and (a2 >= 0.25 - 1e-6).all() and (a2 <= 0.5 + 1e-6).all()


@pytest.mark.parametrize('n,nb_pts', [(1, 1), (64, 64), (65, 64), (5000, 2048), (8193, 8193), (100003, 32768), (70000, 65536)])
def test_a_crop_is_distinct_indices_in_key_order(n, nb_pts):
    off = np.array([0, 17, 17 + n], np.int64)
    choice, num = SS.sample_scenes(off, [1, 1], nb_pts, seed=9)
    assert num.tolist() == [n, n] and choice.shape == (2, nb_pts) and choice.dtype == np.int64
    for b in range(2):
        c = choice[b]
        assert len(np.unique(c)) == nb_pts and c.min() >= 0 and c.max() < n
        keys = SS.lowbias32(c.astype(np.uint32) ^ np.uint32(SS.chunk_seed(9, b)))
        assert (np.diff(keys.astype(np.int64)) > 0).all(), 'ascending keys'
        rest = np.setdiff1d(np.arange(n), c)
        if len(rest):
            assert SS.lowbias32(rest.astype(np.uint32) ^ np.uint32(SS.chunk_seed(9, b))).min() > keys.max(), 'the nb_pts smallest keys'
    if nb_pts > 8:
        assert not np.array_equal(choice[0], choice[1]), 'the same scene twice: two draws'
        assert not np.array_equal(choice[0], SS.sample_scenes(off, [1, 1], nb_pts, seed=10)[0][0])
    assert np.array_equal(choice, SS.sample_scenes(off, [1, 1], nb_pts, seed=9)[0])


@pytest.mark.parametrize('n,nb_pts', [(1, 8193), (63, 64), (8192, 8193), (32767, 32768), (2000, 65536)])
def test_a_pad_is_the_scene_then_repeats_in_range(n, nb_pts):
    off = np.array([0, n, n, 2 * n], np.int64)
    choice, num = SS.sample_scenes(off, [0, 2, 1], nb_pts, seed=3)
    assert num.tolist() == [n, n, 0]
    for b in range(2):
        assert np.array_equal(choice[b, :n], np.arange(n)) and choice[b, n:].min() >= 0 and choice[b, n:].max() < n
    if n > 1 and nb_pts - n > 8:
        assert len(np.unique(choice[0, n:])) > 1 and not np.array_equal(choice[0, n:], choice[1, n:])
    assert (choice[2] == 0).all(), 'a scene without points'


def test_limits_are_refused_before_any_launch():
    """Over-limit nb_pts / Ntot / B: MVP_EUNSUPPORTED and a zero workspace; shape errors: MVP_EINVAL; missing pointers: MVP_ENULL -- all
    before any HIP call (safe without a GPU)."""
    import ctypes
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)

    def sample(nb_pts, Ntot=1000, B=2, S=1, ws=d, off=d):
        return lib.mvp_sample_scenes_f32(off, d, Ntot, S, B, nb_pts, 0, None, d, d, ws, 1 << 50, None)
    assert sample(65537) == -2 and sample(2048, Ntot=2 ** 31) == -2 and sample(2048, B=65536) == -2
    assert sample(0) == -1 and sample(2048, Ntot=0) == -1 and sample(2048, S=0) == -1 and sample(2048, B=-1) == -1
    assert sample(2048, ws=None) == -3 and sample(2048, off=None) == -3 and sample(2048, ws=ctypes.c_void_p(8)) == -1
    assert lib.mvp_sample_scenes_f32(d, d, 1000, 1, 2, 2048, 0, None, d, d, d, 64, None) == -1  # scratch too small
    assert sample(2048, B=0) == 0
    W = lib.mvp_sample_scenes_workspace
    assert W(1000, 2, 65537) == 0 and W(2 ** 31, 2, 2048) == 0 and W(1000, 65536, 2048) == 0 and W(1000, 0, 2048) == 0 and W(1000, 2, 0) == 0
    small, one_tile, big = W(1000, 2, 64), W(1000, 8, 8192), W(4800000, 8, 65536)
    assert 0 < small < one_tile < big < 16 << 20
    assert W(1000, 8, 8193) > 2 * 8 * 8193 * 8, 'two pair buffers past one LDS tile'

    def gather(nb_pts=64, Ntot=1000, B=2, points=d, label=None, out_label=None, colors=None, out_feature=None, out_points=d):
        return lib.mvp_gather_cloud_f32(points, label, colors, d, d, d, None, Ntot, 1, B, nb_pts, out_points, out_label, out_feature, None)
    assert gather(points=None) == -3 and gather(out_points=None) == -3 and gather(label=d) == -3 and gather(colors=d) == -3
    assert gather(nb_pts=0) == -1 and gather(Ntot=0) == -1 and gather(B=-1) == -1
    assert gather(nb_pts=2 ** 31) == -2 and gather(B=65536) == -2
    assert gather(B=0) == 0


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import mvpnet_amd.ops as ops
    off, rows = torch.tensor([0, 10]), torch.tensor([0])
    with pytest.raises(RuntimeError):
        ops.sample_scenes(off, rows, 8)
    with pytest.raises(RuntimeError):
        ops.gather_cloud(torch.zeros(10, 3), off, rows, torch.zeros(1, 8, dtype=torch.int64))


# ---- the config helper ----------------------------------------------------------------------------------------------------------------
def cfg_of(name, extra=''):
    from mvpnet_amd import config as C
    with open(os.path.join(GOLDEN, 'configs_3d.json')) as f:
        return C.load_cfg(text=yaml.safe_dump(json.load(f)[name]) + extra)


@pytest.mark.parametrize('name,dataset,nb_pts,color', [('pn2ssg_chunk', 'ScanNet3DChunks', 8192, False), ('pn2ssg_rgb_chunk', 'ScanNet3DChunks', 8192, True),
                                                      ('pn2ssg_scene', 'ScanNet3DScene', 32768, False), ('pn2ssg_rgb_scene', 'ScanNet3DScene', 32768, True)])
def test_config_helper_on_the_four_yamls(name, dataset, nb_pts, color):
    from mvpnet_amd import config as C
    cfg = cfg_of(name)
    train, val = C.build_batch_3d(cfg, training=True), C.build_batch_3d(cfg, training=False)
    assert train['dataset'] == val['dataset'] == dataset and train['nb_pts'] == val['nb_pts'] == nb_pts
    assert train['use_color'] is color and val['use_color'] is color
    assert train['z_rot'] == (-math.pi, math.pi) and val['z_rot'] is None
    if dataset == 'ScanNet3DChunks':
        assert (train['chunk_size'], train['chunk_margin'], train['chunk_thresh']) == ((1.5, 1.5), (0.2, 0.2), 0.3)
    else:
        assert 'chunk_size' not in train
    assert cfg.TRAIN.BATCH_SIZE == (32 if dataset == 'ScanNet3DChunks' else 8)
    model = C.build_model_sem_seg_3d(cfg)
    assert model.in_channels == (3 if color else 0)
    import inspect
    from mvpnet_amd import scene as SC
    assert set(train) <= set(inspect.signature(SC.sample_train_batch_3d).parameters)


@pytest.mark.parametrize('aug', ['(("Sample", 8192),)', '("RandomRotateZ",)', '(("CropPad", 8192), "RandomRotateZ", "RandomRotateZ")', '()',
                                 '(("CropPad", 8192), ("RandomRotateZ", 0.0, 1.0))', '(("CropPad", 0),)', '("RandomRotateZ", ("CropPad", 8192))'])
def test_config_helper_refuses_other_augmentations(aug):
    from mvpnet_amd import config as C
    cfg = cfg_of('pn2ssg_chunk')
    cfg.merge_from_list(['TRAIN.AUGMENTATION', aug])
    with pytest.raises(ValueError, match='AUGMENTATION'):
        C.build_batch_3d(cfg, training=True)
    assert C.build_batch_3d(cfg, training=False)['nb_pts'] == 8192  # (VAL's list is untouched)

"""Writes tests/golden/scene_sample.npz and tests/golden/configs_3d.json: what the REFERENCE's 3D-baseline loader does with the fixture
cloud of tests/scene_sample_oracle.py, angle by angle, and its four 3D-baseline YAMLs as data.

    python -m tests.golden.make_scene_sample_golden /path/to/the/reference/checkout

`ScanNet3DScene.__getitem__` (mvpnet/data/scannet_3d.py:206-221, use_color) runs unmodified on an object made with `object.__new__` (its
constructor reads ScanNet's files) with the transform `Compose([CropPad(nb_pts), RandomRotateZ()])` of mvpnet/data/transforms.py.
`np.random.uniform` returns the fixture's next angle instead of a draw, `np.random.randint` / `np.random.choice` are recorded, and
`Rotation.as_dcm`, which scipy 1.6 removed, is `Rotation.as_matrix` (_RotationWithDcm).  nb_pts = 2048 pads the 2000 points, so the first
2000 rows of the result are the cloud in its own order: the file keeps, per angle, the float32 matrix (`get_rotation` called again with
the same angle) and those rotated rows, and once the features of the 2000 points.  The script asserts that the rows behind them are the
recorded pad draws, and that a crop (nb_pts = 1024) returns the rows of its recorded `np.random.choice`.
configs_3d.json: the YAMLs under
configs/scannet/3d_baselines parsed by PyYAML, the way configs.json holds two experiment files."""
import json
import os
import sys

import numpy as np

from tests import scene_sample_oracle as SS
from tests.golden.make_train_sample_golden import Recorder, _stub_missing

HERE = os.path.dirname(os.path.abspath(__file__))


class _RotationWithDcm:
    """scipy's Rotation as transforms.py uses it (`Rotation.from_rotvec(v).as_dcm()`), for a scipy whose Rotation has `as_matrix` only
    (the class is immutable: the name in the transforms module is replaced instead)."""

    def __init__(self, rot):
        self.as_dcm = rot.as_matrix

    @staticmethod
    def from_rotvec(vec):
        from scipy.spatial.transform import Rotation
        return _RotationWithDcm(Rotation.from_rotvec(vec))


def main(reference_root):
    sys.path.insert(0, reference_root)
    _stub_missing()
    from mvpnet.data import transforms as T
    if not hasattr(T.Rotation, 'as_dcm'):
        T.Rotation = _RotationWithDcm
    from mvpnet.data.scannet_3d import ScanNet3DScene
    P = SS.FIXTURE
    points, colors, label = SS.fixture_cloud()
    n = len(points)
    angles = SS.fixture_angles()
    ds = object.__new__(ScanNet3DScene)
    # (the cache holds float64 points, uint8 colours and raw labels; label_mapping None keeps the labels as they are)
    ds.data = [dict(scan_id='fixture', points=points.astype(np.float64), colors=colors, seg_label=label)]
    ds.scan_ids, ds.label_mapping = ['fixture'], None
    ds.use_color = True
    uniform = np.random.uniform
    mats, rotated, feature = [], [], None
    try:
        for angle in angles:
            np.random.uniform = lambda low=0.0, high=1.0, size=None, a=float(angle): a
            ds.transform = T.Compose([T.CropPad(P['nb_pts']), T.RandomRotateZ()])
            np.random.seed(int(abs(angle) * 1000))
            with Recorder() as rec:
                out = ds[0]
            pad = [r for f, a, r in rec.log if f == 'randint' and a == n]
            assert len(pad) == 1 and len(pad[0]) == P['nb_pts'] - n
            R = T.RandomRotateZ().get_rotation()
            assert R.dtype == np.float32 and R.shape == (3, 3) and out['points'].dtype == np.float32 and out['feature'].dtype == np.float32
            assert np.array_equal(out['points'], np.concatenate([points, points[pad[0]]]) @ R.T)
            assert np.array_equal(out['seg_label'], np.concatenate([label, label[pad[0]]]))
            assert np.array_equal(out['feature'][n:], out['feature'][:n][pad[0]])
            mats.append(R)
            rotated.append(out['points'][:n].copy())
            if feature is None:
                feature = out['feature'][:n].copy()
            assert np.array_equal(feature, out['feature'][:n])
        # the crop: CropPad's np.random.choice picks the rows
        np.random.uniform = lambda low=0.0, high=1.0, size=None: 0.0
        ds.transform = T.Compose([T.CropPad(1024)])
        with Recorder() as rec:
            out = ds[0]
        pick = [r for f, a, r in rec.log if f == 'choice']
        assert len(pick) == 1 and len(np.unique(pick[0])) == 1024 and np.array_equal(out['points'], points[pick[0]])
        assert np.array_equal(out['feature'], feature[pick[0]])
    finally:
        np.random.uniform = uniform
    path = os.path.join(HERE, 'scene_sample.npz')
    np.savez_compressed(path, angle=angles.astype(np.float64), rot=np.stack(mats), rotated=np.stack(rotated), feature=feature)
    print('%d angles, %d points' % (len(angles), n))
    print('wrote', path, os.path.getsize(path), 'bytes')

    import yaml
    cfgs = {}
    for name in ('pn2ssg_chunk', 'pn2ssg_rgb_chunk', 'pn2ssg_scene', 'pn2ssg_rgb_scene'):
        with open(os.path.join(reference_root, 'configs', 'scannet', '3d_baselines', name + '.yaml')) as f:
            cfgs[name] = yaml.safe_load(f)
    path = os.path.join(HERE, 'configs_3d.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main(sys.argv[1])

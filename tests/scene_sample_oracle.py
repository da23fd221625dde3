"""NumPy restatement of what mvp_sample_scenes_f32 and mvp_gather_cloud_f32 compute (test infrastructure, never imported by the product):
`CropPad(nb_pts)` of whole scenes by the counter-hash resampling of tests/train_sample_oracle.py with every point a member
(mvpnet/data/transforms.py:112-133 behind mvpnet/data/scannet_3d.py:206-221), and the gather with `RandomRotateZ`'s float32 product and
`colors / 255` (transforms.py:64-85, scannet_3d.py:82).  tests/golden/scene_sample.npz holds what the REFERENCE's transforms return for the
angles of FIXTURE; tests/test_scene_sample_cpu.py holds this file to it."""
import numpy as np

from tests.train_sample_oracle import chunk_seed, lowbias32, resample  # noqa: F401 (re-exported for the tests)

FIXTURE = dict(n_pts=2000, nb_pts=2048, angles=32, seed=20250)


def fixture_cloud():
    """The fixture's cloud: points (n,3) float32 in a 8 x 6 x 3 m room moved off the origin, uint8 colours with every value present,
    labels in [0, 20) with -100 = unlabelled."""
    rs = np.random.RandomState(FIXTURE['seed'])
    n = FIXTURE['n_pts']
    points = (rs.rand(n, 3) * np.array([8.0, 6.0, 3.0]) + np.array([-1.5, 2.0, 0.0])).astype(np.float32)
    colors = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    colors.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    label = rs.randint(0, 20, n).astype(np.int64)
    label[rs.rand(n) < 0.2] = -100
    return points, colors, label


def fixture_angles():
    """Radians in [-pi, pi]: the ends, the quarter turns, zero, and seeded uniform draws."""
    rs = np.random.RandomState(FIXTURE['seed'] + 1)
    fixed = np.array([-np.pi, np.pi, 0.0, 0.5 * np.pi, -0.5 * np.pi, 0.25 * np.pi, 1e-9, -3.0])
    return np.concatenate([fixed, rs.uniform(-np.pi, np.pi, FIXTURE['angles'] - len(fixed))])


def z_rotation(angle):
    """augment.z_rotation_from_angle's formula: cos and sin in float64, rounded once -> (...,3,3) float32"""
    a = np.asarray(angle, np.float64)
    c, s = np.cos(a), np.sin(a)
    z, o = np.zeros_like(c), np.ones_like(c)
    return np.stack([c, -s, z, s, c, z, z, z, o], -1).reshape(a.shape + (3, 3)).astype(np.float32)


def sample_scenes(scene_offsets, scene_of_row, nb_pts, seed=0):
    """-> choice (B,nb_pts) int64, num_points (B,) int32"""
    B = len(scene_of_row)
    choice, num = np.zeros((B, nb_pts), np.int64), np.zeros(B, np.int32)
    for b in range(B):
        s = int(scene_of_row[b])
        n = int(scene_offsets[s + 1]) - int(scene_offsets[s])
        num[b] = n
        if n > 0:
            choice[b] = resample(np.ones(n, bool), nb_pts, seed, b)
    return choice, num


def rotate(xyz, R):
    """xyz (...,3) float32, R (3,3) float32 -> (R[a,0]*x + R[a,1]*y) + R[a,2]*z in float32, each operation rounded once"""
    xyz, R = np.asarray(xyz, np.float32), np.asarray(R, np.float32)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    with np.errstate(invalid='ignore'):
        return np.stack([(R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z for a in range(3)], -1).astype(np.float32)


def gather_cloud(points, scene_offsets, scene_of_row, choice, seg_label=None, colors=None, rot=None):
    """-> dict: points (B,3,nb) float32 [, seg_label (B,nb) int64] [, feature (B,3,nb) float32]"""
    B, nb = choice.shape
    Ntot = len(points)
    out = {'points': np.zeros((B, 3, nb), np.float32)}
    if seg_label is not None:
        out['seg_label'] = np.full((B, nb), -100, np.int64)
    if colors is not None:
        out['feature'] = np.zeros((B, 3, nb), np.float32)
    for b in range(B):
        s = int(np.clip(scene_of_row[b], 0, len(scene_offsets) - 2))
        off = int(np.clip(scene_offsets[s], 0, Ntot))
        end = int(np.clip(scene_offsets[s + 1], off, Ntot))
        if end == off:
            continue
        j = off + np.clip(choice[b], 0, end - off - 1)
        xyz = points[j]
        out['points'][b] = (xyz if rot is None else rotate(xyz, rot[b])).T
        if seg_label is not None:
            out['seg_label'][b] = seg_label[j]
        if colors is not None:
            out['feature'][b] = (colors[j].astype(np.float32) / np.float32(255.0)).T
    return out

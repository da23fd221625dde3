"""NumPy restatement of what mvp_sample_chunks_f32 and mvp_select_frames_ranges_u32 compute (test infrastructure, never imported by the
product): the try rule and the whole-scene fallback of ScanNet2D3DChunks.__getitem__ (mvpnet/data/scannet_2d3d.py:341-369) and of
ScanNet3DChunks (mvpnet/data/scannet_3d.py:149-178, float64 bounds), the counter-hash resampling that stands in for :374-381, the
base-point bits (:199-204) and frame selection per chunk inside its own scene's frame range.  tests/golden/train_sample.npz holds what
the REFERENCE's two `__getitem__` return for the draws of FIXTURE; tests/test_train_sample_cpu.py holds this file to it."""
import numpy as np

from tests import scene_prep_oracle as SO

FIXTURE = dict(scene_id=0, n_pts=60000, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2), chunk_thresh=0.3, num_tries=10,
               label_kinds=('dense', 'patchy', 'sparse'), seeds=6, nb_pts=(2048, 8192))


def fixture_points():
    """The cloud of the fixture scene (make_rgbd_scene is deterministic; one frame: the depth maps are not used here)."""
    from mvpnet_amd.synthetic import make_rgbd_scene
    return make_rgbd_scene(FIXTURE['scene_id'], 1, n_pts=FIXTURE['n_pts'], h=4, w=4)['points']


def fixture_labels(points, kind, seed=0):
    """Seeded labels in [0, 20) with -100 = unlabelled.  'dense': 10 % unlabelled (every try passes); 'patchy': the half x < 3.4 m of the
    room is 92 % unlabelled, the rest 10 % (tries fail or pass with the centre); 'sparse': 90 % unlabelled (the whole-scene fallback)."""
    rs = np.random.RandomState(4200 + seed)
    n = len(points)
    label = rs.randint(0, 20, n).astype(np.int64)
    u = rs.rand(n)
    if kind == 'dense':
        drop = u < 0.10
    elif kind == 'patchy':
        drop = np.where(points[:, 0] < 3.4, u < 0.92, u < 0.10)
    elif kind == 'sparse':
        drop = u < 0.90
    else:
        raise ValueError(kind)
    label[drop] = -100
    return label


def lowbias32(x):
    """csrc/dropout.h's hash on uint32 arrays (a bijection of 32-bit words)."""
    x = np.array(x, dtype=np.uint32, ndmin=1)
    with np.errstate(over='ignore'):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def try_box(center_xy, chunk_size, chunk_margin, bounds_f64=False):
    """(lo, hi) of one try, in the arithmetic of the class: float32 size / margin (scannet_2d3d.py:134-136) or float64 (scannet_3d.py:128-130)
    against the float32 centre -- `center -/+ 0.5 * size`, then `-/+ margin` (:345-352)."""
    dt = np.float64 if bounds_f64 else np.float32
    size, margin = np.array(chunk_size, dtype=dt), np.array(chunk_margin, dtype=dt)
    c = np.asarray(center_xy, np.float32)
    lo = (c - 0.5 * size) - margin
    hi = (c + 0.5 * size) + margin
    assert lo.dtype == dt
    return lo, hi


def members_of(points, lo, hi):
    xy = points[:, :2]
    with np.errstate(invalid='ignore'):
        return np.all(np.logical_and(xy >= lo, xy <= hi), axis=1)


def draw_chunk(points, label, centers, chunk_size, chunk_margin, chunk_thresh, bounds_f64=False):
    """-> try_index (-1: fallback), box (4,) float32 lo.x lo.y hi.x hi.y, member mask (n,) bool."""
    points = np.asarray(points, np.float32)
    for t, ci in enumerate(centers):
        lo, hi = try_box(points[int(ci), :2], chunk_size, chunk_margin, bounds_f64)
        mask = members_of(points, lo, hi)
        m = int(mask.sum())
        if m == 0:
            continue
        if float(np.mean(label[mask] >= 0)) >= float(chunk_thresh):  # (double) l / (double) m against the Python float
            return t, np.hstack([lo, hi]).astype(np.float32), mask
    margin = np.array(chunk_margin, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        lo = np.min(points[:, :2], axis=0) - margin
        hi = np.max(points[:, :2], axis=0) + margin
    return -1, np.hstack([lo, hi]).astype(np.float32), np.ones(len(points), bool)


def chunk_seed(seed, b):
    seed = int(seed) & (2 ** 64 - 1)
    seed32 = (seed ^ (seed >> 32)) & 0xFFFFFFFF
    return int(lowbias32((seed32 + 0x9E3779B9 * (b + 1)) & 0xFFFFFFFF)[0])


def resample(mask, nb_pts, seed, b):
    """choice (nb_pts,) int64 into the scene: the pad / crop rule of include/mvp_hip.h."""
    members = np.nonzero(mask)[0].astype(np.int64)
    m = len(members)
    sb = np.uint32(chunk_seed(seed, b))
    if m < nb_pts:
        s = np.arange(m, nb_pts, dtype=np.uint32)
        slot = (lowbias32(s ^ sb ^ np.uint32(0x85EBCA6B)).astype(np.uint64) * np.uint64(m)) >> np.uint64(32)
        return np.concatenate([members, members[slot.astype(np.int64)]])
    keys = lowbias32(members.astype(np.uint32) ^ sb)
    return members[np.argsort(keys, kind='stable')[:nb_pts]]


def sample_chunks(points, label, scene_offsets, scene_of_chunk, center_ind, nb_pts, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2),
                  chunk_thresh=0.3, seed=0, base_point_ind=None, bounds_f64=False):
    """The whole op on host arrays; + 'mask': list of the member masks."""
    B = len(scene_of_chunk)
    out = dict(choice=np.zeros((B, nb_pts), np.int64), points=np.zeros((B, 3, nb_pts), np.float32), seg_label=np.zeros((B, nb_pts), np.int64),
               chunk_box=np.zeros((B, 4), np.float32), try_index=np.zeros(B, np.int32), num_members=np.zeros(B, np.int32), mask=[])
    bits = []
    for b in range(B):
        s = int(scene_of_chunk[b])
        lo, hi = int(scene_offsets[s]), int(scene_offsets[s + 1])
        pts, lab = points[lo:hi], label[lo:hi]
        t, box, mask = draw_chunk(pts, lab, center_ind[b], chunk_size, chunk_margin, chunk_thresh, bounds_f64)
        choice = resample(mask, nb_pts, seed, b)
        out['choice'][b], out['points'][b], out['seg_label'][b] = choice, pts[choice].T, lab[choice]
        out['chunk_box'][b], out['try_index'][b], out['num_members'][b] = box, t, int(mask.sum())
        out['mask'].append(mask)
        if base_point_ind is not None:
            bits.append(mask[base_point_ind[s]])
    if base_point_ind is not None:
        out['base_bits'] = SO.pack_bits(np.stack(bits))
    return out


def select_frames_ranges(overlaps, chunk_masks, frame_begin, frame_count, num_rgbd_frames):
    """overlaps (nb,Ftot) bool: all scenes' frames side by side; chunk c chooses inside columns [begin, begin + count) -> global indices,
    gain."""
    C = len(chunk_masks)
    picked, gain = np.zeros((C, num_rgbd_frames), np.int64), np.zeros((C, num_rgbd_frames), np.int32)
    for c in range(C):
        b, k = int(frame_begin[c]), int(frame_count[c])
        p, g = SO.select_frames_batched(overlaps[:, b:b + k], chunk_masks[c:c + 1], num_rgbd_frames)
        picked[c], gain[c] = p[0] + b, g[0]
    return picked, gain

"""Writes tests/golden/scene_prep.npz: for the scene of tests/scene_prep_oracle.FIXTURE (mvpnet_amd.synthetic.make_rgbd_scene) the base
points, the oracle's packed RGB-D overlap, the chunks' base-point masks and the frames picked per chunk.

    python -m tests.golden.make_scene_prep_golden

The pinned float32 nearest-neighbour rule is checked here against an independent float64 KD-tree
(scipy.spatial.cKDTree(base).query(x, 1, distance_upper_bound=radius)): the two overlap matrices must be IDENTICAL for the fixture's
scene, so that the fixture is also what the reference's open3d search would give.  The script also insists that the scene has a chunk
no frame sees (all-zero scores: frame 0 picked again and again) and an exact score tie at a pick's maximum."""
import os

import numpy as np

from tests import scene_prep_oracle as SO


def kdtree_overlap(depth, kinv, pose, base, radius):
    from scipy.spatial import cKDTree
    xyz, mask = SO.world_points(depth, kinv, pose)
    tree = cKDTree(base.astype(np.float64))
    out = np.zeros((len(base), len(pose)), bool)
    for f in range(len(pose)):
        if not np.all(np.isfinite(pose[f])):
            continue
        x = xyz[f][mask[f]].astype(np.float64)
        if len(x) == 0:
            continue
        dist, j = tree.query(x, 1, distance_upper_bound=radius)
        out[j[np.isfinite(dist)], f] = True
    return out


def main():
    P = SO.FIXTURE
    sc = SO.fixture_scene()
    rs = np.random.RandomState(4242)
    base_point_ind = rs.choice(P['n_pts'], P['num_base_pts'], replace=False).astype(np.int64)
    base = sc['points'][base_point_ind]
    overlaps = SO.rgbd_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], base, P['radius'])
    tree = kdtree_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], base, P['radius'])
    differing = int((overlaps != tree).sum())
    print('oracle vs float64 KD-tree: %d differing entries of %d; %d set' % (differing, overlaps.size, int(overlaps.sum())))
    assert differing == 0
    assert not overlaps[:, P['n_frames'] // 2].any(), 'the frame with the inf pose sees nothing'
    assert np.array_equal(overlaps[:, -1], overlaps[:, P['n_frames'] // 3]), 'the duplicated frame'
    masks = SO.chunk_masks_of(sc['chunk_inds'], base_point_ind, P['n_pts'])
    picked, gain = SO.select_frames_batched(overlaps, masks, P['num_rgbd_frames'])
    unseen = [c for c in range(len(masks)) if masks[c].any() and not overlaps[masks[c]].any()]
    print('%d chunks, base points per chunk %d..%d, chunks no frame sees: %s' % (len(masks), masks.sum(1).min(), masks.sum(1).max(), unseen))
    assert unseen and all((picked[c] == 0).all() for c in unseen)
    ties = 0
    for c in range(len(masks)):
        left = overlaps[masks[c]]
        for f in picked[c]:
            score = left.sum(0)
            ties += int(score.max() > 0 and (score == score.max()).sum() > 1)
            left = left[~left[:, f]]
    print('picks whose maximum score is shared by several frames:', ties)
    assert ties > 0
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'scene_prep.npz')
    np.savez_compressed(path, base_point_ind=base_point_ind, overlap_bits=SO.pack_bits(overlaps.T), chunk_bits=SO.pack_bits(masks),
                        picked=picked, gain=gain, points_sum=np.float64(sc['points'].astype(np.float64).sum()),
                        depth_sum=np.int64(sc['depth_mm'].astype(np.int64).sum()))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

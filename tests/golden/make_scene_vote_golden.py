"""Writes tests/golden/scene_vote.npz: a jittered room surface cloud (floor and two walls of 6.5 x 5.5 x 2.5 m, sigma = 5 mm, n = 6000,
float32), V = 3 vote index sets of nb = 2048 and, per vote, the nearest sampled point of every scene point as
sklearn.neighbors.NearestNeighbors(n_neighbors=1, algorithm='ball_tree') returns it -- the call of mvpnet/test_3d_scene.py:159-160.

    python -m tests.golden.make_scene_vote_golden

The script insists that the pinned float32 lowest-index rule (tests/scene_vote_oracle.nearest) agrees with the ball tree on EVERY row of
every vote, and that every query is certified by its 27-cell block at this shape (10 cells per axis): the fixture then exercises the grid
path alone.  A seed that gives a disagreeing row is replaced by another one, never met with a tolerance.  No logits are stored: the tests
draw them from a seeded CPU generator."""
import os

import numpy as np

from tests import scene_vote_oracle as VO


def main():
    from sklearn.neighbors import NearestNeighbors
    P = VO.FIXTURE
    points, vote_inds = VO.fixture_cloud()
    assert points.dtype == np.float32 and points.shape == (P['n'], 3) and vote_inds.shape == (P['V'], P['nb'])
    nn = np.empty((P['V'], P['n']), np.int64)
    for v in range(P['V']):
        keys = points[vote_inds[v]]
        nbrs = NearestNeighbors(n_neighbors=1, algorithm='ball_tree').fit(keys)
        _, ind = nbrs.kneighbors(points)
        nn[v] = ind[:, 0]
        mine = VO.nearest(points, keys)
        differing = int((mine != nn[v]).sum())
        cert = VO.certified(points, keys)
        print('vote %d: %d rows differ from the ball tree, %d of %d queries certified, grid %s' % (
            v, differing, int(cert.sum()), len(cert), VO.build_grid(keys)[2].tolist()))
        assert differing == 0
        assert cert.all()
        assert (nn[v][vote_inds[v]] == np.arange(P['nb'])).all(), 'a sampled point is its own nearest key'
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'scene_vote.npz')
    np.savez_compressed(path, points=points, vote_inds=vote_inds.astype(np.int32), nn=nn.astype(np.int32))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

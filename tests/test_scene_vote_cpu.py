"""Whole-scene voting without a GPU: the NumPy oracle against the committed scikit-learn ball-tree fixture, the certification rule on the
fixture, the two entry points in the signature table and the library, and their argument checks (which return before any launch)."""
import ctypes

import numpy as np
import pytest

from tests import scene_vote_oracle as VO


@pytest.fixture(scope='module')
def fixture(golden):
    g = golden('scene_vote')
    return {k: g[k] for k in g.files}


def test_fixture_is_the_oracles_cloud(fixture):
    points, vote_inds = VO.fixture_cloud()
    P = VO.FIXTURE
    assert fixture['points'].dtype == np.float32 and fixture['points'].shape == (P['n'], 3)
    assert fixture['nn'].shape == (P['V'], P['n']) and fixture['vote_inds'].shape == (P['V'], P['nb'])
    assert np.array_equal(fixture['points'], points) and np.array_equal(fixture['vote_inds'], vote_inds)


def test_oracle_nearest_equals_the_ball_tree_on_every_row(fixture):
    pts = fixture['points']
    for v in range(VO.FIXTURE['V']):
        keys = pts[fixture['vote_inds'][v]]
        assert np.array_equal(VO.nearest(pts, keys), fixture['nn'][v].astype(np.int64))


def test_every_fixture_query_is_certified_by_its_block(fixture):
    pts = fixture['points']
    for v in range(VO.FIXTURE['V']):
        keys = pts[fixture['vote_inds'][v]]
        assert VO.build_grid(keys)[2].tolist() == [10, 10, 10]
        assert VO.certified(pts, keys).all()


def test_certification_restatement_refuses_what_it_must():
    """An empty block, a zero-extent cloud seen from afar and a NaN query are not certified; a query between two far clusters is not."""
    rs = np.random.RandomState(1)
    keys = np.concatenate([rs.rand(1024, 3), rs.rand(1024, 3) + np.array([6.0, 0, 0])]).astype(np.float32)
    q = np.array([[3.5, 0.5, 0.5], [0.5, 0.5, 0.5], [np.nan, 0.5, 0.5]], np.float32)
    assert VO.certified(q, keys).tolist() == [False, True, False]
    assert VO.nearest(np.zeros((1, 3), np.float32), np.zeros((5, 3), np.float32)).tolist() == [0]  # the lowest index among equals


def test_propagate_adds_in_vote_order():
    rs = np.random.RandomState(2)
    pts = rs.rand(50, 3).astype(np.float32)
    keys = np.stack([pts[rs.choice(50, 9, replace=False)] for _ in range(3)])
    logits = (rs.standard_normal((3, 4, 9)) * 1e3).astype(np.float32)
    total, nn = VO.propagate(pts, keys, logits)
    for p in range(50):
        s = logits[0, :, nn[0, p]]
        for v in (1, 2):
            s = (s + logits[v, :, nn[v, p]]).astype(np.float32)
        assert np.array_equal(total[p], s)
    mean, label = VO.finish(total, 3)
    assert np.array_equal(mean, total / np.float32(3)) and np.array_equal(label, mean.argmax(1))


def test_symbols_are_declared_and_exported():
    from mvpnet_amd import _lib
    lib = _lib.lib()
    assert 'mvp_vote_nearest_f32' in _lib._SIGNATURES and len(_lib._SIGNATURES['mvp_vote_nearest_f32']) == 16
    for name in ('mvp_vote_nearest_f32', 'mvp_vote_nearest_workspace'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    ws = lib.mvp_vote_nearest_workspace
    assert ws(3, 32768) == 3 * (16 * 32768 + 16512) and ws(1, 256) == 16 * 256 + 16512
    assert ws(1, 255) == 0 and ws(1, 65537) == 0 and ws(0, 2048) == 0 and ws(65536, 2048) == 0
    import mvpnet_amd.ops as ops
    from mvpnet_amd import scene
    assert callable(ops.vote_nearest) and callable(scene.infer_scene_votes)


def test_argument_errors_do_not_launch():
    """Precondition failures return MVP_E* before any HIP call (safe without a GPU)."""
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    big = 1 << 30

    def call(n=8, V=1, nb=2048, C=20, points=d, key=d, logit=d, total=d, ws=d, ws_bytes=big):
        return lib.mvp_vote_nearest_f32(points, n, key, V, nb, logit, C * nb, 1, nb, C, total, None, None, ws, ws_bytes, None)

    assert call(nb=0) == -1                                  # MVP_EINVAL: 1 <= nb
    assert call(nb=65537) == -1
    assert call(C=65) == -1 and call(C=0) == -1              # 1 <= C <= 64
    assert call(V=0) == -1 and call(V=65536) == -1           # 1 <= V < 65536
    assert call(n=1 << 31) == -1 and call(n=-1) == -1        # n < 2^31
    assert call(ws=ctypes.c_void_p(24)) == -1                # misaligned workspace
    assert call(ws_bytes=16 * 2048 + 16512 - 1) == -1        # too small
    assert call(ws=None) == -3                               # MVP_ENULL where a grid is built
    assert call(points=None) == -3 and call(key=None) == -3 and call(logit=None) == -3 and call(total=None) == -3
    assert call(n=0) == 0 and call(n=0, nb=100, ws=None, ws_bytes=0) == 0  # nothing to do: no launch either


def test_no_cpu_fallback():
    import torch
    import mvpnet_amd.ops as ops
    with pytest.raises(RuntimeError):
        ops.vote_nearest(torch.rand(5, 3), torch.rand(1, 4, 3), torch.rand(1, 2, 4))

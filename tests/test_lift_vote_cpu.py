"""Lift-and-vote without a GPU: the NumPy oracle of mvp_lift_vote_f32 against the committed reference fixture (the reference's MVPNet2D
run chunk by chunk and accumulated as mvpnet/test_2d_chunks.py does: tests/golden/make_scene_2d_golden.py), the entry point in the
signature table and the library, and its argument checks (which return before any launch)."""
import ctypes

import numpy as np
import pytest

from tests import lift_vote_oracle as LO


@pytest.fixture(scope='module')
def fixture(golden):
    g = golden('scene_2d')
    return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def inputs(fixture):
    return LO.fixture_inputs(fixture)


def test_fixture_describes_the_oracles_scene(fixture, inputs):
    from tests import scene_prep_oracle as SO
    P = LO.FIXTURE
    sc, store, view_frame, knn, knn_base, chunk_inds, frames = inputs
    assert fixture['mean'].dtype == np.float32 and fixture['mean'].shape == (P['n_pts'], LO.STANDIN_CLASSES)
    assert np.array_equal(fixture['base_point_ind'], sc['base_point_ind'])
    overlaps = np.unpackbits(fixture['overlaps'], axis=1)[:, :P['n_frames']].astype(bool)
    assert np.array_equal(overlaps, SO.rgbd_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], sc['points'][sc['base_point_ind']], P['radius']))
    masks = SO.chunk_masks_of(chunk_inds, sc['base_point_ind'], P['n_pts'])
    picked, gain = SO.select_frames_batched(overlaps, masks, P['num_rgbd_frames'])
    assert np.array_equal(picked, fixture['picked'])
    assert (gain.sum(1) == 0).any(), 'a chunk whose base points no frame sees'
    assert (fixture['count'] == 0).any() and fixture['count'].max() > 1, 'a point in no chunk and a point in several'
    assert len(frames) < picked.size and knn.min() >= 0 and knn.max() < P['num_rgbd_frames'] * P['h'] * P['w']
    assert knn.shape == (int(fixture['lengths'].sum()), P['k'])


def test_oracle_against_the_reference_fixture(fixture, inputs):
    """The float32 oracle and the reference's result both lie within the rounding bound of the float64 evaluation, with equal labels
    wherever the float64 top-two gap exceeds twice the bound (fewer than 0.5 % of the voted points are excluded); counts are equal."""
    P = LO.FIXTURE
    sc, store, view_frame, knn, knn_base, chunk_inds, frames = inputs
    total, count = LO.lift_vote_f32(store, view_frame, knn, knn_base, chunk_inds, P['n_pts'])
    mean, label = LO.finish(total, count)
    total64, scale, count64 = LO.lift_vote_f64(store, view_frame, knn, knn_base, chunk_inds, P['n_pts'])
    assert np.array_equal(count, fixture['count'].astype(np.int32)) and np.array_equal(count, count64)
    for name, (m, l) in (('oracle', (mean, label)), ('reference', (fixture['mean'], fixture['label'].astype(np.int64)))):
        worst, excluded = LO.check_against_f64(m, l, count, total64, scale, P['k'])
        print('%s: worst error / bound %.3f, excluded %.5f' % (name, worst, excluded))
    assert (mean[count == 0] == 0).all() and (label[count == 0] == LO.STANDIN_CLASSES).all()


def test_oracle_adds_in_the_pinned_order():
    """Two chunks naming one point, k = 3 with a missing neighbour, logits that make every other order round differently."""
    logit = np.zeros((2, 4, 1), np.float32)
    logit[0, :, 0] = [1e8, 1.0, -1e8, 3.0]
    logit[1, :, 0] = [5.0, 1e-3, 7.0, 2.0 ** -20]
    view_frame = np.array([[0, 1], [1, 0]], np.int32)
    knn = np.array([[0, 1, 2], [4 + 1, -1, 3], [9, 9, 9], [4 + 0, 1, 0]], np.int64)   # row 2 lies between the chunks and is never read
    total, count = LO.lift_vote_f32(logit, view_frame, knn, [0, 3], [np.array([1, 0]), np.array([1])], 3)
    f = np.float32
    m00 = f(f(f(1e8) + f(1.0)) + f(-1e8)) / f(3)             # chunk 0, row 0 -> point 1: frame 0 pixels 0, 1, 2
    m01 = f(f(f(1e-3) + f(0)) + f(3.0)) / f(3)               # chunk 0, row 1 -> point 0: frame 1 pixel 1, missing, frame 0 pixel 3
    m10 = f(f(f(1e8) + f(1e-3)) + f(5.0)) / f(3)             # chunk 1 (views: frame 1, frame 0), row 0 -> point 1
    assert total[1, 0] == f(f(f(0) + m00) + m10) and total[0, 0] == f(f(0) + m01) and total[2, 0] == 0
    assert count.tolist() == [1, 2, 0]
    mean, label = LO.finish(total, count)
    assert label.tolist() == [0, 0, 1] and mean[1, 0] == total[1, 0] / f(2)


def test_symbol_is_declared_and_exported():
    from mvpnet_amd import _lib
    lib = _lib.lib()
    assert 'mvp_lift_vote_f32' in _lib._SIGNATURES and len(_lib._SIGNATURES['mvp_lift_vote_f32']) == 20
    assert 'mvp_lift_vote_f32' in _lib.EXPORTS and hasattr(lib, 'mvp_lift_vote_f32')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import scene
    assert callable(ops.lift_vote) and callable(scene.infer_scene_2d)


def test_argument_errors_do_not_launch():
    """Precondition failures return MVP_E* before any HIP call (safe without a GPU)."""
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)

    def call(U=5, hw=48, C=20, nv=3, k=3, num_chunks=4, n_pts=300, ld=None, **ptrs):
        p = dict(logit=d, view_frame=d, knn=d, knn_base=d, chunk_offsets=d, point_offsets=d, point_slots=d, total=d, count=d)
        p.update(ptrs)
        ld_f, ld_p, ld_c = (hw * C, C, 1) if ld is None else ld
        return lib.mvp_lift_vote_f32(p['logit'], ld_f, ld_p, ld_c, U, hw, C, p['view_frame'], nv, p['knn'], k, p['knn_base'], p['chunk_offsets'],
                                     num_chunks, p['point_offsets'], p['point_slots'], n_pts, p['total'], p['count'], None)

    assert call(k=0) == -1 and call(k=9) == -1                        # MVP_EINVAL: 1 <= k <= 8
    assert call(C=0) == -1 and call(C=65) == -1                       # 1 <= C <= 64
    assert call(nv=0) == -1 and call(U=0) == -1 and call(hw=0) == -1 and call(num_chunks=0) == -1 and call(n_pts=-1) == -1
    assert call(ld=(-1, 20, 1)) == -1 and call(ld=(960, -20, 1)) == -1 and call(ld=(960, 1, -48)) == -1
    # MVP_EUNSUPPORTED: what the kernel holds in 32 bits
    assert call(nv=1 << 16, hw=1 << 15) == -2 and call(hw=1 << 31) == -2 and call(nv=1 << 31) == -2
    assert call(U=1 << 31) == -2 and call(num_chunks=1 << 30) == -2 and call(num_chunks=1 << 29, nv=4) == -2 and call(n_pts=1 << 31) == -2
    for name in ('logit', 'view_frame', 'knn', 'knn_base', 'chunk_offsets', 'point_offsets', 'point_slots', 'total', 'count'):
        assert call(**{name: None}) == -3, name                      # MVP_ENULL
    assert call(k=0, logit=None) == -3                                # a null pointer outranks an invalid size
    assert call(n_pts=0) == 0                                         # nothing to do: no launch either


def test_no_cpu_fallback():
    import torch
    import mvpnet_amd.ops as ops
    with pytest.raises(RuntimeError):
        ops.lift_vote(torch.rand(2, 4, 3, 3), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.int64), [0],
                      [torch.arange(5)], 7)

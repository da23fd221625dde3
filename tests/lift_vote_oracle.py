"""NumPy restatement of mvp_lift_vote_f32's pinned definition (include/mvp_hip.h) -- test infrastructure, never imported by the product.

  lift_vote_f32 : the float32 definition with sequential np.float32 operations, every one rounded once, in the pinned order:
                  m_e = (((l_0 + l_1) + ...) + l_{k-1}) / k per position, sum[p] = ((0 + m_e1) + m_e2) + ... in chunk order.
  lift_vote_f64 : the same quantity in float64 (exact to ~1e-16 relative) and, per point and class, S_p = sum_e (sum_j |l_j|) / k, the scale of the
                  float32 rounding bound (bound()).
  finish        : mvp_vote_finish_f32.
`logit` is always the LOGICAL (U, hw, C) array: how the store lies in memory is the kernel's business."""
import numpy as np

STANDIN_CLASSES = 20


def _neighbour_logits(logit, view_frame_i, ids, hw):
    """ids (n,) int64 chunk-local flat pixel ids -> (n,C) logits in logit's dtype, +0 rows where the id is missing (< 0)."""
    ok = ids >= 0
    safe = np.where(ok, ids, 0)
    view, q = safe // hw, safe % hw
    rows = logit[np.asarray(view_frame_i)[view], q]
    return np.where(ok[:, None], rows, np.zeros((), logit.dtype))


def lift_vote_f32(logit, view_frame, knn, knn_base, chunk_inds, n_pts):
    """logit (U,hw,C) float32; view_frame (num_chunks,nv); knn (R,k) int64; knn_base (num_chunks,); chunk_inds: list of int64 arrays of
    scene point ids (distinct inside a chunk) -> sum (n_pts,C) float32, count (n_pts,) int32."""
    logit = np.asarray(logit)
    assert logit.dtype == np.float32 and logit.ndim == 3
    hw, C = logit.shape[1], logit.shape[2]
    k = knn.shape[1]
    total = np.zeros((n_pts, C), np.float32)
    count = np.zeros(n_pts, np.int32)
    for i, ind in enumerate(chunk_inds):
        ind = np.asarray(ind, np.int64)
        assert len(np.unique(ind)) == len(ind)
        rows = knn[int(knn_base[i]):int(knn_base[i]) + len(ind)]  # rows beyond the chunk's valid length are never read
        m = _neighbour_logits(logit, view_frame[i], rows[:, 0], hw)
        for j in range(1, k):
            m = m + _neighbour_logits(logit, view_frame[i], rows[:, j], hw)
            assert m.dtype == np.float32
        m = m / np.float32(k)
        assert m.dtype == np.float32
        total[ind] = total[ind] + m
        count[ind] += 1
    return total, count


def lift_vote_f64(logit, view_frame, knn, knn_base, chunk_inds, n_pts):
    """-> (sum (n_pts,C) float64, S (n_pts,C) float64 with S_p[c] = sum_e (sum_j |l_j[c]|) / k, count (n_pts,) int32)."""
    logit = np.asarray(logit, np.float64)
    hw, C = logit.shape[1], logit.shape[2]
    k = knn.shape[1]
    total = np.zeros((n_pts, C), np.float64)
    scale = np.zeros((n_pts, C), np.float64)
    count = np.zeros(n_pts, np.int32)
    for i, ind in enumerate(chunk_inds):
        ind = np.asarray(ind, np.int64)
        rows = knn[int(knn_base[i]):int(knn_base[i]) + len(ind)]
        ls = [_neighbour_logits(logit, view_frame[i], rows[:, j], hw) for j in range(k)]
        total[ind] += sum(ls) / k
        scale[ind] += sum(np.abs(l) for l in ls) / k
        count[ind] += 1
    return total, scale, count


def finish(total, count):
    """mvp_vote_finish_f32: mean = sum / max(count, 1) in float32, label = first maximum, C where count == 0."""
    total = np.asarray(total, np.float32)
    mean = total / np.maximum(count, 1).astype(np.float32)[:, None]
    label = mean.argmax(1).astype(np.int64)
    label[np.asarray(count) == 0] = total.shape[1]
    return mean.astype(np.float32), label


def bound(scale, count, k):
    """|float32 mean - exact mean| <= (k + count + 1) * 2^-23 * S / max(count, 1), per class: the first-order rounding bound of k - 1
    additions, one division, `count` additions and the finishing division (each relative 2^-24 of a partial result no larger than its
    share of S), doubled for the higher-order terms.  scale (n_pts,C) or (n_pts,), count (n_pts,)."""
    c = np.asarray(count, np.float64)
    f = (k + c + 1.0) * 2.0 ** -23 / np.maximum(c, 1.0)
    return f[:, None] * scale if np.ndim(scale) == 2 else f * scale


def check_against_f64(mean, label, count, total64, scale, k, max_excluded=0.005):
    """The rule of the k > 1 comparisons: `mean` (n_pts,C) float32 lies within bound() of the float64 mean everywhere, and `label` equals
    the float64 label wherever the float64 top-two gap exceeds twice the bound; fewer than `max_excluded` of the voted points may be
    excluded that way.  -> (largest |error| / bound, excluded fraction), for the caller to print."""
    count = np.asarray(count)
    mean64 = total64 / np.maximum(count, 1)[:, None]
    b = bound(scale, count, k)
    err = np.abs(np.asarray(mean, np.float64) - mean64)
    assert (err <= b).all(), 'error beyond the rounding bound: worst ratio %g' % float((err / np.maximum(b, 1e-300)).max())
    voted = count > 0
    C = mean64.shape[1]
    label64 = mean64.argmax(1)
    if C > 1:
        top2 = np.sort(mean64, 1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
    else:
        gap = np.full(len(mean64), np.inf)
    sure = voted & (gap > 2 * b.max(1))
    label = np.asarray(label)
    assert (label[sure] == label64[sure]).all()
    assert (label[~voted] == C).all()
    excluded = float((voted & ~sure).sum()) / max(int(voted.sum()), 1)
    assert excluded < max_excluded, 'too many points excluded from the label comparison: %g' % excluded
    worst = float((err[voted] / np.maximum(b[voted], 1e-300)).max()) if voted.any() else 0.0
    return worst, excluded


# ---- the stand-in 2D network of the scene tests and of tests/golden/scene_2d.npz ---------------------------------------------------
def standin_weights():
    """(3, STANDIN_CLASSES) float32: the logit of class c is (x0*w[0,c] + x1*w[1,c]) + x2*w[2,c], every operation rounded once."""
    return np.random.RandomState(2020).standard_normal((3, STANDIN_CLASSES)).astype(np.float32)


def standin_logits(image):
    """image (F,3,h,w) float32 -> (F,C,h,w) float32 with the stand-in's operations in its order."""
    w = standin_weights()
    x = np.asarray(image, np.float32)
    out = np.empty((x.shape[0], w.shape[1]) + x.shape[2:], np.float32)
    for c in range(w.shape[1]):
        out[:, c] = (x[:, 0] * w[0, c] + x[:, 1] * w[1, c]) + x[:, 2] * w[2, c]
    return out


# ---- tests/golden/scene_2d.npz -----------------------------------------------------------------------------------------------------
FIXTURE = dict(scene_id=5, n_frames=12, n_pts=6000, h=12, w=16, num_base_pts=400, base_seed=31, image_seed=32, radius=0.1,
               num_rgbd_frames=3, k=3, chunk_size=(1.5, 1.5), chunk_stride=1.0, chunk_thresh=150, chunk_margin=(0.2, 0.2))


def fixture_scene():
    """The scene of tests/golden/scene_2d.npz, regenerated (make_rgbd_scene is deterministic), with the images the stand-in reads."""
    from mvpnet_amd.synthetic import make_rgbd_scene
    P = FIXTURE
    sc = make_rgbd_scene(P['scene_id'], P['n_frames'], n_pts=P['n_pts'], h=P['h'], w=P['w'])
    sc['images'] = np.random.RandomState(P['image_seed']).standard_normal((P['n_frames'], 3, P['h'], P['w'])).astype(np.float32)
    sc['base_point_ind'] = np.sort(np.random.RandomState(P['base_seed']).choice(P['n_pts'], P['num_base_pts'], replace=False)).astype(np.int64)
    return sc


def fixture_inputs(g):
    """The oracle's arguments from tests/golden/scene_2d.npz `g` and the regenerated scene: (scene, store (U,hw,C) of the stand-in's logits
    for the distinct picked frames, view_frame, knn (R,k) int64 with the chunks' rows back to back, knn_base, chunk_inds, frames)."""
    P = FIXTURE
    sc = fixture_scene()
    picked = g['picked'].astype(np.int64)
    frames = np.unique(picked)
    view_frame = np.searchsorted(frames, picked).astype(np.int32)
    store = np.ascontiguousarray(standin_logits(sc['images'][frames]).reshape(len(frames), STANDIN_CLASSES, P['h'] * P['w']).transpose(0, 2, 1))
    lengths = g['lengths'].astype(np.int64)
    knn_base = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    chunk_inds = np.split(g['chunk_index'].astype(np.int64), np.cumsum(lengths)[:-1])
    return sc, store, view_frame, g['knn'].astype(np.int64), knn_base, chunk_inds, frames

"""NumPy restatement of whole-scene voting (mvpnet/test_3d_scene.py:152-164 with the nearest neighbour pinned as include/mvp_hip.h pins
it for mvp_vote_nearest_f32): float32 brute force, the lowest key index among equal distances, the votes added in order.  Also restates
the kernel's grid (csrc/ball_grid.hip: ball_grid_build_kernel with cellmin = 0 and knn_grid_axis(nb) cells per axis) far enough to say
which queries the 27-cell block certifies, and draws the jittered room clouds the tests and the fixture use."""
import numpy as np

F32 = np.float32
FIXTURE = dict(n=6000, nb=2048, V=3, seed=22, vote_seed=77)


def room_cloud(n, seed, size=(6.5, 5.5, 2.5), sigma=0.005):
    """n float32 points on the floor and two walls of a room of `size` metres, jittered by N(0, sigma) per axis."""
    rs = np.random.RandomState(seed)
    sx, sy, sz = size
    area = np.array([sx * sy, sx * sz, sy * sz])
    which = rs.choice(3, n, p=area / area.sum())
    u, v = rs.rand(n), rs.rand(n)
    p = np.empty((n, 3), np.float64)
    p[which == 0] = np.stack([u * sx, v * sy, np.zeros(n)], 1)[which == 0]   # floor
    p[which == 1] = np.stack([u * sx, np.zeros(n), v * sz], 1)[which == 1]   # wall y = 0
    p[which == 2] = np.stack([np.zeros(n), u * sy, v * sz], 1)[which == 2]   # wall x = 0
    return (p + rs.standard_normal((n, 3)) * sigma).astype(F32)


def dist2(points, keys):
    """(q,nb) float32 (dx*dx + dy*dy) + dz*dz, every operation rounded once."""
    d = points[:, None, :].astype(F32) - keys[None, :, :].astype(F32)
    d = d * d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def nearest(points, keys, block=512):
    """int64 (n,): argmin over the keys of the pinned distance, the first (lowest) index among equals."""
    out = np.empty(len(points), np.int64)
    block = max(1, min(block, (1 << 23) // max(1, len(keys))))  # keeps the (block, nb, 3) temporaries near 100 MB
    with np.errstate(invalid='ignore', over='ignore'):
        for lo in range(0, len(points), block):
            out[lo:lo + block] = np.argmin(dist2(points[lo:lo + block], keys), axis=1)
    return out


def propagate(points, keys, logits):
    """points (n,3), keys (V,nb,3), logits (V,C,nb) -> sum (n,C) = (...(logit_0[nn_0] + logit_1[nn_1]) + ...) in float32, nn (V,n) int64."""
    V = len(keys)
    nn = np.stack([nearest(points, keys[v]) for v in range(V)])
    total = np.ascontiguousarray(logits[0].T[nn[0]], dtype=F32)
    with np.errstate(invalid='ignore', over='ignore'):
        for v in range(1, V):
            total = total + logits[v].T[nn[v]].astype(F32)
    return total, nn


def finish(total, V):
    """`pred_logit_whole_scene / num_votes` and `np.argmax(..., axis=1)` (test_3d_scene.py:163-164)."""
    mean = total / F32(V)
    return mean, np.argmax(mean, axis=1).astype(np.int64)


def grid_axis(nb):
    g = int(np.cbrt(float(nb)) / 1.3 + 0.5)
    return min(max(g, 2), 16)


def build_grid(keys):
    """min (3,), inv (3,) float32 and g (3,) int of one cloud's grid, as ball_grid_build_kernel forms them with cellmin = 0."""
    gmax = grid_axis(len(keys))
    mn, inv, g = np.zeros(3, F32), np.zeros(3, F32), np.ones(3, np.int64)
    fmax = np.finfo(F32).max
    with np.errstate(all='ignore'):
        for a in range(3):
            col = keys[:, a][np.abs(keys[:, a]) <= fmax]
            lo, hi = (F32(col.min()), F32(col.max())) if len(col) else (F32(0), F32(0))
            ext = F32(hi - lo)
            cell = max(F32(0), F32(ext / F32(gmax)))
            iv = F32(F32(1) / cell) if (cell > 0 and cell <= fmax) else F32(0)
            if not iv <= fmax:
                iv = F32(0)
            gf = F32(ext * iv)
            ga = int(min(gf, F32(gmax))) + 1 if (iv > 0 and gf >= 0) else 1
            mn[a], inv[a], g[a] = lo, iv, min(ga, gmax)
    return mn, inv, g


def cells_of(x, mn, inv, g):
    """(m,3) int cell of every row, as cell_of: u = (x - min) * inv, clamped to [0, g - 1], NaN -> 0."""
    with np.errstate(all='ignore'):
        u = (x.astype(F32) - mn[None]) * inv[None]
        c = np.where(u >= 0, np.minimum(u, (g - 1).astype(F32)[None]), F32(0))
    return c.astype(np.int64)


def certified(points, keys, block=512):
    """bool (n,): the 27 cells around the query certify their minimum -- it is below (0.999 margin)^2, margin = the distance to the nearest
    face of the block that has cells beyond it (float32, the kernel's expressions)."""
    mn, inv, g = build_grid(keys)
    kc = cells_of(keys, mn, inv, g)
    qc = cells_of(points, mn, inv, g)
    out = np.zeros(len(points), bool)
    with np.errstate(all='ignore'):
        margin = np.full(len(points), np.inf, F32)
        for a in range(3):
            if inv[a] > 0:
                cell = F32(F32(1) / inv[a])
                q = points[:, a].astype(F32)
                below = q - (mn[a] + (qc[:, a] - 1).astype(F32) * cell)
                above = (mn[a] + (qc[:, a] + 2).astype(F32) * cell) - q
                margin = np.where(qc[:, a] >= 2, np.fmin(margin, below), margin).astype(F32)
                margin = np.where(qc[:, a] + 2 < g[a], np.fmin(margin, above), margin).astype(F32)
        m = (margin * F32(0.999)).astype(F32)
        for lo in range(0, len(points), block):
            d = dist2(points[lo:lo + block], keys)
            inside = (np.abs(kc[None, :, :] - qc[lo:lo + block, None, :]) <= 1).all(2)
            d = np.where(inside & (d < np.inf), d, F32(np.inf))
            d1 = d.min(1)
            mm = m[lo:lo + block]
            out[lo:lo + block] = (mm > 0) & (d1 < mm * mm)
    return out


def fixture_cloud():
    """The committed fixture's inputs, redrawn: points (n,3) float32 and vote_inds (V,nb) int64."""
    P = FIXTURE
    points = room_cloud(P['n'], P['seed'])
    rs = np.random.RandomState(P['vote_seed'])
    vote_inds = np.stack([rs.choice(P['n'], P['nb'], replace=False) for _ in range(P['V'])]).astype(np.int64)
    return points, vote_inds

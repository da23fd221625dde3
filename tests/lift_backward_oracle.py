"""The lift backward as mvp_lift_backward_f32 defines it (include/mvp_hip.h), in NumPy: for every chunk the sequential loop over the
edges e = n*k + slot in ASCENDING e, `out[b, index[b,e], :] += grad[b,e,:]` in float32 (one rounding per addition) into a map of +0.0;
an index outside [0,P) is skipped.  Plain helper module: the input recipes of tests/test_lift_backward_{cpu,gpu}.py live here too, so
both files (and the references they share) see the same arrays."""
import functools

import numpy as np


def lift_backward(grad, index, P, descending=False):
    """grad (B,N,k,C) float32, index (B,N,k) int64 -> (B,P,C) float32.  descending: the same sum walked from the last edge to the
    first (what a wrong order looks like; the tests use it to show that their inputs can tell the orders apart)."""
    grad = np.ascontiguousarray(grad, dtype=np.float32)
    B, C = grad.shape[0], grad.shape[-1]
    g = grad.reshape(B, -1, C)
    ix = np.asarray(index).reshape(B, -1)
    out = np.zeros((B, P, C), np.float32)
    for b in range(B):
        order = range(ix.shape[1] - 1, -1, -1) if descending else range(ix.shape[1])
        for e in order:
            j = int(ix[b, e])
            if 0 <= j < P:
                out[b, j] += g[b, e]   # float32 + float32 -> float32, rounded once
    return out


def list_lengths(index, P):
    """(B,P) int64: how many edges name each pixel."""
    ix = np.asarray(index).reshape(index.shape[0], -1)
    return np.stack([np.bincount(r[(r >= 0) & (r < P)], minlength=P) for r in ix])


def gradients(rs, B, N, k, C):
    """normal x 10^U(-3,3) per row: magnitudes six decades apart, so the order of the additions shows in the low bits."""
    return (rs.standard_normal((B, N, k, C)) * 10.0 ** rs.uniform(-3, 3, (B, N, k, 1))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mixed_case(C, seed=0):
    """B = 2, P = 96 (nv = 2, 6 x 8), N = 50, k = 3; indices uniform in [-2, P + 2]: ignored entries on both sides occur."""
    B, P, N, k = 2, 96, 50, 3
    rs = np.random.RandomState(seed + 100 * C)
    index = rs.randint(-2, P + 3, (B, N, k)).astype(np.int64)
    assert (index < 0).any() and (index >= P).any()
    grad = gradients(rs, B, N, k, C)
    return grad, index, P, lift_backward(grad, index, P)


@functools.lru_cache(maxsize=None)
def hot_case(seed=0):
    """B = 2, P = 96, N = 1000, k = 3, C = 8.  Chunk 0: the first 2000 edges name pixel 7, the rest are random; chunk 1: all 3000
    edges name pixel 95."""
    B, P, N, k, C = 2, 96, 1000, 3, 8
    rs = np.random.RandomState(seed)
    index = rs.randint(0, P, (B, N * k)).astype(np.int64)
    index[0, :2000] = 7
    index[1, :] = 95
    index = index.reshape(B, N, k)
    grad = gradients(rs, B, N, k, C)
    return grad, index, P, lift_backward(grad, index, P)


@functools.lru_cache(maxsize=None)
def window_case(P, N, k, C, seed=0):
    """B = 1, P beyond the counters of one workgroup: half the indices uniform over P, half inside a 64-pixel window (lists of tens to
    hundreds of entries) that straddles a multiple of 8192."""
    rs = np.random.RandomState(seed + P)
    E = N * k
    index = rs.randint(0, P, E).astype(np.int64)
    window = rs.rand(E) < 0.5
    index[window] = 3 * 8192 - 20 + rs.randint(0, 64, int(window.sum()))
    index = index.reshape(1, N, k)
    grad = gradients(rs, 1, N, k, C)
    return grad, index, P, lift_backward(grad, index, P)

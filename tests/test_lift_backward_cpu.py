"""The lift backward as a gather, the host side (no GPU): the NumPy statement of the definition (tests/lift_backward_oracle.py) against
np.add.at and against the float64 sum; the derived ctypes signatures of the two new entries; every argument error of
mvp_lift_backward_f32 returns its code before any HIP call."""
import ctypes

import numpy as np
import pytest

from tests import lift_backward_oracle as O

OK, EINVAL, EUNSUPPORTED, ENULL = 0, -1, -2, -3


def test_the_oracle_loop_is_np_add_at_on_the_in_range_entries():
    for grad, index, P, want in (O.hot_case(), O.mixed_case(8), O.mixed_case(6)):
        B, C = grad.shape[0], grad.shape[-1]
        got = np.zeros((B, P, C), np.float32)
        for b in range(B):
            ix, g = index[b].reshape(-1), grad[b].reshape(-1, C)
            ok = (ix >= 0) & (ix < P)
            np.add.at(got[b], ix[ok], g[ok])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_the_hot_rows_tell_the_ascending_order_from_the_descending_one():
    grad, index, P, want = O.hot_case()
    back = O.lift_backward(grad, index, P, descending=True)
    differs = (want.view(np.int32) != back.view(np.int32)).any(axis=2)
    assert differs[0, 7] and differs[1, 95]
    lengths = O.list_lengths(index, P)
    assert lengths[0, 7] >= 2000 and lengths[1, 95] == 3000 and lengths[1].sum() == 3000


def test_the_oracle_stays_within_the_summation_bound_of_the_float64_sum():
    """Per element |float32 loop - float64 sum| <= (L - 1) * 2^-24 * sum |addend|, L = the list's length: L - 1 roundings (the first
    addition, into +0, is exact), each at most half an ulp of a partial sum that the sum of magnitudes bounds."""
    for grad, index, P, want in (O.hot_case(), O.mixed_case(64), O.window_case(57600, 2048, 3, 8)):
        B, C = grad.shape[0], grad.shape[-1]
        exact, mag = np.zeros((B, P, C), np.float64), np.zeros((B, P, C), np.float64)
        for b in range(B):
            ix, g = index[b].reshape(-1), grad[b].reshape(-1, C).astype(np.float64)
            ok = (ix >= 0) & (ix < P)
            np.add.at(exact[b], ix[ok], g[ok])
            np.add.at(mag[b], ix[ok], np.abs(g[ok]))
        L = O.list_lengths(index, P)[:, :, None]
        bound = np.maximum(L - 1, 0) * 2.0 ** -24 * mag
        assert (np.abs(want.astype(np.float64) - exact) <= bound).all()
        assert not want[L[:, :, 0] == 0].view(np.int32).any(), 'a pixel nobody names is +0.0'


def test_the_derived_signatures():
    from ctypes import c_int, c_int64, c_void_p
    from mvpnet_amd import _lib as L
    p, i64 = c_void_p, c_int64
    assert L._SIGNATURES['mvp_lift_backward_workspace_bytes'] == [i64] * 4 and L._RESTYPES['mvp_lift_backward_workspace_bytes'] is i64
    assert L._SIGNATURES['mvp_lift_backward_f32'] == [p, p] + [i64] * 5 + [p, p, p] and L._RESTYPES['mvp_lift_backward_f32'] is c_int
    assert L._SIGNATURES['mvp_lift_gather_backward_f32'] == [p, p] + [i64] * 5 + [p, p], 'the atomic entry stays as it was'
    for name in ('mvp_lift_backward_workspace_bytes', 'mvp_lift_backward_f32', 'mvp_lift_gather_backward_f32'):
        assert name in L.EXPORTS and hasattr(L.lib(), name)


def test_the_workspace_size():
    from mvpnet_amd import _lib as L
    size = L.lib().mvp_lift_backward_workspace_bytes
    assert size(2, 96, 50, 3) == 1984                              # 4 * 2 * (97 + 150) = 1976, rounded up to 16
    assert size(32, 57600, 8192, 3) == 4 * 32 * (57601 + 24576)    # offsets (B,P+1) + slots (B,N*k), int32
    assert size(1, 96, 0, 3) == 400 and size(0, 96, 50, 3) == 0
    for bad in ((-1, 96, 50, 3), (2, -1, 50, 3), (2, 96, -1, 3), (2, 96, 50, -1), (65536, 96, 50, 3), (2, 1 << 31, 50, 3),
                (2, 96, 1 << 28, 8), (2, 96, 1 << 31, 1)):
        assert size(*bad) == 0
    assert size(2, 96, (1 << 28) - 1, 8) > 0


def test_argument_errors_do_not_launch():
    """A precondition failure returns before any HIP call, so no dummy address here is ever dereferenced (and no GPU is needed)."""
    from mvpnet_amd import _lib as L
    fn = L.lib().mvp_lift_backward_f32
    d = ctypes.c_void_p(64)
    B, P, C, N, k = 2, 96, 8, 50, 3
    call = lambda g=d, ix=d, ws=d, out=d, B=B, P=P, C=C, N=N, k=k: fn(g, ix, B, P, C, N, k, ws, out, None)
    for name in ('g', 'ix', 'ws', 'out'):
        assert call(**{name: None}) == ENULL
        assert call(**{name: None}, B=-1) == ENULL   # a null pointer outranks an invalid argument, as everywhere in the library
    for name in ('B', 'P', 'C', 'N', 'k'):
        assert call(**{name: -1}) == EINVAL
    assert call(P=0) == EINVAL
    for misaligned in (64 + 8, 64 + 4, 64 + 1):
        assert call(ws=ctypes.c_void_p(misaligned)) == EINVAL
    assert call(g=ctypes.c_void_p(64 + 2)) == EINVAL and call(out=ctypes.c_void_p(64 + 1)) == EINVAL
    # beyond what the kernels hold in 32 bits
    assert call(N=1 << 28, k=8) == EUNSUPPORTED and call(N=1 << 31, k=1) == EUNSUPPORTED and call(N=1 << 40, k=3) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED and call(P=1 << 31) == EUNSUPPORTED
    assert call(B=65536, ws=ctypes.c_void_p(72)) == EINVAL and call(B=65536, N=-1) == EINVAL
    # nothing to do: no launch either
    assert call(B=0) == OK and call(C=0) == OK


def test_the_op_checks_its_arguments_before_anything_else():
    import torch
    import mvpnet_amd.ops as ops
    g, ix = torch.zeros(1, 5, 3, 8), torch.zeros(1, 5, 3, dtype=torch.int64)
    assert 'lift_gather_backward' in ops.__all__
    with pytest.raises(RuntimeError, match='float32 gradient and int64 indices'):
        ops.lift_gather_backward(g.double(), ix, 96)
    with pytest.raises(RuntimeError, match='float32 gradient and int64 indices'):
        ops.lift_gather_backward(g, ix.int(), 96)
    with pytest.raises(RuntimeError, match=r'\(B,N,k,C\)'):
        ops.lift_gather_backward(g[:, :4], ix, 96)
    with pytest.raises(RuntimeError, match='P > 0'):
        ops.lift_gather_backward(g, ix, 0)
    with pytest.raises(RuntimeError, match='GPU only'):   # a CPU tensor like any other: no fallback
        ops.lift_gather_backward(g, ix, 96)

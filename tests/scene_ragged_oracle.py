"""NumPy restatement of what mvp_scene_chunks_count_f32 / mvp_scene_chunks_fill_f32 and mvp_pack_chunks_f32 compute (test infrastructure,
never imported by the product): the window tests of scene2chunks_legacy (mvpnet/utils/chunk_util.py:4-53) in the arithmetic pinned in
include/mvp_hip.h, and the pad rule of mvpnet/test_mvpnet_3d.py:146-154 as a counter hash."""
import numpy as np

from tests import scene_prep_oracle as SO
from tests.train_sample_oracle import lowbias32, chunk_seed


def window_tests(points, corners, chunk_size, margin):
    """points (n,3) f32, corners (nc,2) f32 -> inner (nc,n), outer (nc,n) bool."""
    xy = np.asarray(points, np.float32)[:, :2]
    lo = np.asarray(corners, np.float32).reshape(-1, 2)
    size, mg = np.asarray(chunk_size, np.float64), np.asarray(margin, np.float64)
    xyd, lod = xy.astype(np.float64), lo.astype(np.float64)
    hi = lod + size
    with np.errstate(invalid='ignore'):
        inner = ((xy[None] >= lo[:, None]) & (xyd[None] <= hi[:, None])).all(-1)
        outer = ((xyd[None] >= (lod - mg)[:, None]) & (xyd[None] <= (hi + mg)[:, None])).all(-1)
    return inner, outer


def scene_chunks(points, corners, chunk_size, margin, thresh, base_point_ind=None):
    """-> dict kept (C,), lengths (C,), index (total,) int64, zbox (C,2) f32, base_bits (C,W) uint32 or None."""
    points = np.asarray(points, np.float32)
    inner, outer = window_tests(points, corners, chunk_size, margin)
    kept = np.nonzero(inner.sum(1) >= thresh)[0]
    lists = [np.nonzero(outer[w])[0].astype(np.int64) for w in kept]
    zbox = np.zeros((len(kept), 2), np.float32)
    for c, ind in enumerate(lists):
        z = points[ind, 2]
        zbox[c] = (np.min(z), np.max(z)) if len(z) else (np.inf, -np.inf)  # numpy.min / max hand a NaN on, like torch.amin / amax
    bits = None
    if base_point_ind is not None:
        bits = SO.pack_bits(outer[kept][:, np.asarray(base_point_ind)].reshape(len(kept), -1))
    return dict(kept=kept, lengths=np.array([len(i) for i in lists], np.int64),
                index=np.concatenate(lists) if lists else np.zeros(0, np.int64), zbox=zbox, base_bits=bits)


def pad_slots(n_c, N_c, seed, c):
    """(N_c,) int64: which member of chunk c (position in its list) fills each of its N_c slots."""
    assert N_c >= n_c >= 1
    sc = np.uint32(chunk_seed(seed, c))
    s = np.arange(n_c, N_c, dtype=np.uint32)
    pad = (lowbias32(s ^ sc ^ np.uint32(0x85EBCA6B)).astype(np.uint64) * np.uint64(n_c)) >> np.uint64(32)
    return np.concatenate([np.arange(n_c, dtype=np.int64), pad.astype(np.int64)])


def pack_chunks(points, index, offsets, out_base, out_len, seed=0):
    """-> flat float32 array: chunk c as a (3, out_len[c]) matrix at out_base[c]; floats no chunk covers stay NaN."""
    points = np.asarray(points, np.float32)
    out = np.full(int(max(b + 3 * n for b, n in zip(out_base, out_len))) if len(out_len) else 0, np.nan, np.float32)
    for c in range(len(out_len)):
        members = np.asarray(index[offsets[c]:offsets[c + 1]])
        choice = members[pad_slots(len(members), out_len[c], seed, c)]
        out[out_base[c]:out_base[c] + 3 * out_len[c]] = points[choice].T.reshape(-1)
    return out

"""The keep mask of the folded dropout, restated in numpy from the comments and code of mvpnet_amd/csrc/dropout.h (struct Dropout,
make_dropout, lowbias32) -- nothing of the library is imported here, so a test that compares a kernel with this mask compares it with
what the header SAYS the mask is, not with another kernel's idea of it.

    p32    = float32(p)
    thresh = uint32(clamp(float64(p32) * 2^32, 1, 2^32 - 1))          (truncated; p == 0: thresh = 0, everything is kept)
    seed32 = (seed ^ (seed >> 32)) mod 2^32                            (the 64 -> 32-bit fold of the seed)
    e      = r * C + c  mod 2^32                                       (row-major element index; C = the row length of the dropped tensor)
    keep   = lowbias32(e + seed32 * 0x9E3779B9  mod 2^32) >= thresh
    scale  = float32(1) / (float32(1) - p32)                           (one float32 division)"""
import numpy as np

GOLDEN = 0x9E3779B9


def lowbias32(x):
    """The 32-bit bijection of dropout.h on a uint32 array (or scalar): xorshift 16, * 0x7feb352d, xorshift 15, * 0x846ca68b, xorshift 16."""
    x = np.asarray(x).astype(np.uint64) & np.uint64(0xffffffff)   # (64-bit lanes, masked after every product: no overflow warnings)
    m = np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def threshold(p):
    """-> (thresh as a Python int, scale as np.float32) of make_dropout(p, ...); p == 0: (0, 1)."""
    p32 = np.float32(p)
    if p32 == np.float32(0):
        return 0, np.float32(1)
    if not (np.float32(0) < p32 < np.float32(1)):
        raise ValueError('p must lie in [0, 1)')
    t = float(p32) * 4294967296.0
    t = min(max(t, 1.0), 4294967295.0)
    return int(t), np.float32(1) / (np.float32(1) - p32)


def fold_seed(seed):
    seed = int(seed) & 0xffffffffffffffff
    return (seed ^ (seed >> 32)) & 0xffffffff


def keep_mask(p, seed, R, C):
    """-> (keep: bool (R, C), scale: np.float32).  R * C must fit the 32-bit element counter, as make_dropout demands."""
    R, C = int(R), int(C)
    if R * C >= 1 << 32:
        raise ValueError('R * C must be below 2^32')
    thresh, scale = threshold(p)
    off = (fold_seed(seed) * GOLDEN) & 0xffffffff
    e = (np.arange(R * C, dtype=np.uint64) + np.uint64(off)) & np.uint64(0xffffffff)
    return (lowbias32(e) >= np.uint32(thresh)).reshape(R, C), scale

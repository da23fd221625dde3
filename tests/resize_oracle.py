"""NumPy restatement of mvp_resize_frames_u8 / mvp_prepare_labels_u16 (include/mvp_hip.h) and of scene.sample_train_batch_2d: Pillow's
`resize(size, BILINEAR)` on uint8 RGB, its `resize(size, NEAREST)` on a 16-bit label image, the label mapping and the flip.  TEST
INFRASTRUCTURE: held to Pillow itself by tests/test_resize_cpu.py through tests/golden/resize.npz, and the library is held to it."""
import math

import numpy as np

from tests import frames_oracle as FO

PRECISION_BITS = 32 - 8 - 2


def bilinear_table(inS, outS):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter, one axis -> xmin (outS), count (outS), coef (outS,
    ksize) int32, ksize.  Python floats are doubles: the arithmetic is the C code's, operation by operation."""
    scale = inS / outS
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin, count, coef = np.zeros(outS, np.int32), np.zeros(outS, np.int32), np.zeros((outS, ksize), np.int32)
    for xx in range(outS):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), inS)
        w = []
        for x in range(hi - lo):
            v = (x + lo - center + 0.5) * ss
            v = -v if v < 0.0 else v
            w.append(1.0 - v if v < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmin[xx], count[xx] = lo, hi - lo
    return xmin, count, coef, ksize


def nearest_table(inS, outS):
    """the source index of Pillow's NEAREST on a 16-bit image, one axis -> (outS,) int32"""
    scale = inS / outS
    return np.array([min(int(scale * (x + 0.5)), inS - 1) for x in range(outS)], np.int32)


def _pass(img, inS, outS, axis):
    """one pass over `axis` of an (..., 3) uint8 image -> uint8 (the rounded intermediate)"""
    xmin, count, coef, _ = bilinear_table(inS, outS)
    img = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((outS,) + img.shape[1:], np.int64)
    for xx in range(outS):
        k = coef[xx, :count[xx]].astype(np.int64)
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, img[xmin[xx]:xmin[xx] + count[xx]], axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize_bilinear(img, size, vertical_first=False):
    """img (H,W,3) uint8, size = PIL's (w, h) -> (h,w,3) uint8: Pillow's two passes, horizontal first, the intermediate rounded to uint8;
    a pass whose axis keeps its size does not run.  vertical_first: the other order (what the kernel must NOT compute)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape[:2]
    w, h = size
    passes = [(W, w, 1), (H, h, 0)]
    for inS, outS, axis in (passes[::-1] if vertical_first else passes):
        if inS != outS:
            img = _pass(img, inS, outS, axis)
    return img


def resize_frames(frames, picked, size):
    """frames (Ftot,H,W,3) uint8, picked (Nf,) clamped, size (w, h) -> (Nf,h,w,3) uint8"""
    rows = [min(max(int(r), 0), len(frames) - 1) for r in np.asarray(picked).ravel()]
    return np.stack([resize_bilinear(frames[r], size) for r in rows])


def resize_nearest(label, size):
    """label (H,W) of any integer type, size (w, h) -> (h,w): Pillow's NEAREST on a 16-bit image"""
    H, W = label.shape
    w, h = size
    return label[nearest_table(H, h)[:, None].astype(np.int64), nearest_table(W, w)[None, :].astype(np.int64)]


def prepare_labels(labels, picked, size=None, flip=None, mapping=None, ignore_value=-100):
    """labels (Ftot,H,W) uint16, picked (Nf,) clamped -> (Nf,h,w) int64: resize, flip, mapping (ignore_value for a raw id past the table)"""
    out = []
    for i, r in enumerate(np.asarray(picked).ravel()):
        lab = labels[min(max(int(r), 0), len(labels) - 1)]
        if size is not None:
            lab = resize_nearest(lab, size)
        if flip is not None and np.asarray(flip).ravel()[i]:
            lab = lab[:, ::-1]
        lab = lab.astype(np.int64)
        if mapping is not None:
            mapping = np.asarray(mapping, np.int64)
            lab = np.where(lab < len(mapping), mapping[np.minimum(lab, len(mapping) - 1)], np.int64(ignore_value))
        out.append(lab)
    return np.ascontiguousarray(np.stack(out), dtype=np.int64)


def scannet_label_mapping(tsv_text, labelids_text, ignore_value=-100):
    """the `raw_to_scannet` table of mvpnet/data/scannet_2d.py:86-103 from the two files' texts"""
    lines = tsv_text.splitlines()
    head = lines[0].split('\t')
    ci, cn = head.index('id'), head.index('nyu40id')
    pairs = [(int(r.split('\t')[ci]), int(r.split('\t')[cn])) for r in lines[1:] if r.strip()]
    raw_to_nyu40 = np.zeros(max(k for k, _ in pairs) + 1, np.int64)
    for k, v in pairs:
        raw_to_nyu40[k] = v
    ids = [int(l.split('\t')[0]) for l in labelids_text.splitlines() if l.strip()]
    nyu40_to_scannet = np.full(41, ignore_value, np.int64)
    nyu40_to_scannet[ids] = np.arange(len(ids))
    return nyu40_to_scannet[raw_to_nyu40]


def sample_train_batch_2d(images, labels, picked, resize=None, factor=None, order=None, flip=None, mean_std=None, label_mapping=None,
                          channels_last=False):
    """The recipe of ScanNet2D.__getitem__ (scannet_2d.py:146-181) for the frames `picked`, fed the draws: resize (when the size differs) ->
    jitter -> flip -> / 255 -> normalise.  -> image (B,3,h,w) float32 [(B,h,w,3) when channels_last], seg_label (B,h,w) int64"""
    H, W = images.shape[1:3]
    size = None if resize is None or tuple(resize) == (W, H) else tuple(resize)
    small = resize_frames(images, picked, size if size else (W, H))
    image = FO.prepare_frames(small, np.arange(len(small)), factor, order, flip, mean_std, channels_last)
    return image, prepare_labels(labels, picked, size, flip, label_mapping)

"""NumPy restatement of mvp_prepare_frames_u8 (include/mvp_hip.h): the colour jitter of PIL's ImageEnhance chain on uint8 RGB, the
loader's `/ 255.` and normalisation, the horizontal flip.  TEST INFRASTRUCTURE: held to PIL itself by tests/test_frames_cpu.py through
tests/golden/frames.npz, and the kernels are held to it."""
import numpy as np


def gray(img):
    """PIL's convert('L') of an (H,W,3) uint8 image -> (H,W) int64"""
    p = img.astype(np.int64)
    return (p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 0x8000) >> 16


def blend(d, p, f):
    """d, p integer arrays, f the factor: uint8 of PIL's ImageChops blend(degenerate, image, f)"""
    f = np.float32(f)
    t = d.astype(np.float32) + f * (p.astype(np.int64) - d.astype(np.int64)).astype(np.float32)  # float32 throughout, two roundings
    out = np.where(t > 0, np.where(t >= 255, np.float32(255), t), np.float32(0))
    return out.astype(np.int64).astype(np.uint8)  # (truncation)


def mean_gray(img):
    """PIL's int(mean + 0.5) of the grey image, in integers"""
    s, n = int(gray(img).sum()), img.shape[0] * img.shape[1]
    return (2 * s + n) // (2 * n)


def jitter(img, factor, order):
    """img (H,W,3) uint8, factor (3,) = brightness, contrast, saturation, order (3,) codes -> (H,W,3) uint8"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    seen = False
    for op in [int(o) for o in order]:
        if op == 0:
            img = blend(np.zeros_like(img), img, factor[0])
        elif op == 1:
            if seen:
                continue
            seen = True
            img = blend(np.full_like(img, mean_gray(img)), img, factor[1])
        elif op == 2:
            img = blend(np.repeat(gray(img)[..., None], 3, axis=2), img, factor[2])
    return img


def value_table(mean_std=None):
    """(3,256) float32: what byte u of channel c becomes -- the reference's NumPy float32 arithmetic, scannet_2d3d.py:246-251"""
    v = np.arange(256, dtype=np.float32) / np.float32(255.)
    v = np.repeat(v[None], 3, axis=0)
    if mean_std is not None:
        ms = np.asarray(mean_std, dtype=np.float32).reshape(2, 3)
        v = (v - ms[0][:, None]) / ms[1][:, None]
    return v.astype(np.float32)


def prepare_frames(frames, picked, factor=None, order=None, flip=None, mean_std=None, channels_last=False):
    """frames (Ftot,H,W,3) uint8, picked (Nf,) -> (Nf,3,H,W) float32, or (Nf,H,W,3) when channels_last"""
    table = value_table(mean_std)
    out = []
    for i, row in enumerate(np.asarray(picked).ravel()):
        img = frames[min(max(int(row), 0), len(frames) - 1)]
        if order is not None:
            img = jitter(img, np.asarray(factor).reshape(-1, 3)[i], np.asarray(order).reshape(-1, 3)[i])
        val = np.stack([table[c][img[..., c]] for c in range(3)], axis=-1)  # (H,W,3)
        if flip is not None and np.asarray(flip).ravel()[i]:
            val = val[:, ::-1]
        out.append(val if channels_last else val.transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)

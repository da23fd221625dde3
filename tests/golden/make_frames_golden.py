"""Writes tests/golden/frames.npz: colour-jitter vectors from PIL itself (needs Pillow; made with 12.2.0).

    python tests/golden/make_frames_golden.py

torchvision's ColorJitter on a PIL image calls ImageEnhance.{Brightness,Contrast,Color}(img).enhance(factor) in the drawn order
(torchvision/transforms/_functional_pil.py); those calls are made here directly, for fixed factors and orders.  Per group g of one
image size: g_images (n,H,W,3) uint8, and per case g_case_image (index into g_images), g_factor (3,) float32 = brightness, contrast,
saturation, g_order (3,) uint8 (0 / 1 / 2, 3 = no step), g_out (H,W,3) uint8.  PIL's blend takes the factor as a C float, so the float32
value in the file is exactly what PIL used.
"""
import itertools
import os

import numpy as np
from PIL import Image, ImageEnhance

ENHANCERS = {0: ImageEnhance.Brightness, 1: ImageEnhance.Contrast, 2: ImageEnhance.Color}
PERMS = [tuple(p) for p in itertools.permutations((0, 1, 2))]
SHORT = [(0, 3, 3), (1, 3, 3), (2, 3, 3), (0, 2, 3), (2, 1, 3), (1, 0, 3)]  # single-op and two-op orders
FACTORS = [(0.6, 0.7, 0.8),      # below 1
           (1.4, 1.35, 1.3),     # above 1: the clip at 255 is hit
           (1.0, 1.0, 1.0),      # exactly 1: nothing changes
           (1.4, 0.6, 1.2)]


def pil_jitter(img, factor, order):
    im = Image.fromarray(img, 'RGB')
    for op in order:
        if int(op) in ENHANCERS:
            im = ENHANCERS[int(op)](im).enhance(float(factor[int(op)]))
    return np.asarray(im, dtype=np.uint8)


def half_step(h, w, k):
    """mean grey exactly k + 0.5: half the pixels (k,k,k), half (k+1,k+1,k+1) -- the rounding of the contrast mean"""
    flat = np.full((h * w, 3), k, np.uint8)
    flat[1::2] = k + 1
    return flat.reshape(h, w, 3)


def images_for(rs, h, w):
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8),          # random
            rs.randint(118, 131, (h, w, 3)).astype(np.uint8),        # low contrast
            np.tile(np.array([200, 90, 30], np.uint8), (h, w, 1)),   # constant
            rs.randint(180, 256, (h, w, 3)).astype(np.uint8)]        # bright: clips under a factor above 1
    if (h * w) % 2 == 0:
        imgs.append(half_step(h, w, 101))
    return np.stack(imgs)


def group(images, cases):
    factor = np.array([c[1] for c in cases], np.float32)
    order = np.array([c[2] for c in cases], np.uint8)
    idx = np.array([c[0] for c in cases], np.int64)
    out = np.stack([pil_jitter(images[i], f, o) for i, f, o in zip(idx, factor, order)])
    return {'images': images, 'case_image': idx, 'factor': factor, 'order': order, 'out': out}


def main():
    rs = np.random.RandomState(20)
    data = {}
    for name, (h, w) in (('s5x7', (5, 7)), ('s6x8', (6, 8))):
        images = images_for(rs, h, w)
        cases = [(i, f, o) for i in range(len(images)) for f in FACTORS for o in PERMS + SHORT]
        for k, v in group(images, cases).items():
            data[name + '_' + k] = v
    # one frame of the lifting resolution: smooth ramps with noise, like a photograph has
    yy, xx = np.mgrid[0:120, 0:160]
    big = np.stack([xx * 255 // 159, yy * 255 // 119, (xx + yy) * 255 // 278], axis=-1) + rs.randint(-20, 21, (120, 160, 3))
    big = np.clip(big, 0, 255).astype(np.uint8)[None]
    for k, v in group(big, [(0, FACTORS[1], (1, 2, 0)), (0, FACTORS[0], (2, 0, 1)), (0, FACTORS[3], (0, 1, 2))]).items():
        data['s120x160_' + k] = v
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'frames.npz')
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), 'bytes,', sum(len(data[g + '_out']) for g in ('s5x7', 's6x8', 's120x160')), 'cases')


if __name__ == '__main__':
    main()

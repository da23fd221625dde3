"""Preparing a training batch's frames on the GPU from a raw uint8 store, measured next to the same result composed from torch ops and to
what the tree offered before (a float store, no jitter).  Prints ONE JSON line (and writes it to --out).

    python tools/bench_frames.py [--chunks 32] [--picks 3] [--frames 1500] [--height 120] [--width 160] [--windows 7] [--out FILE]
                                 [--profile-only]

The store: --frames synthetic frames (seeded bytes) of --height x --width, resident on the device; every call prepares chunks x picks of
them, drawn once (repeats included).  Method: everything is warmed up first; the variants ALTERNATE inside the same process, window after
window, each timed with device events over 20 calls per window; the figure is the median over the windows and `spread` the
(max - min) / median over them.

  (a) prepare_frames  ops.prepare_frames with a jitter, the normaliser and the flip: one memset and two launches.
  (b) torch_ops       the same result from torch ops on the device, following the definition in include/mvp_hip.h step by step (integer
                      tensors for the pixels, float32 tensors for the blend, the byte table gathered on the device); its bits are asserted
                      equal to (a)'s before anything is timed.
  (c) float_gather    what the tree offered before, WITHOUT a jitter: a float32 normalised store, `store[picked]`, then
                      `torch.where(flip, images.flip(-1), images)` as augment.DeviceAugmentation does it.
  bound               the bytes (a) moves (the picked frames read twice, the floats written once) against HBM.

--profile-only runs (a) alone a few times: the process to put behind `rocprofv3 --kernel-trace --stats --`.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_scene_prep import stats, device_ms, alternate, count_syncs  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
NORMALIZER = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
SCANNET_FRAMES = 125000  # about what the 1201 training scenes keep at every 20th frame


def byte_table(device):
    """(3,256) float32, the value of byte u in channel c: IEEE float32 divisions on the host (NumPy's), uploaded once"""
    v = np.arange(256, dtype=np.float32) / np.float32(255.)
    mean, std = (np.asarray(x, dtype=np.float32) for x in NORMALIZER)
    return torch.from_numpy(((v[None] - mean[:, None]) / std[:, None]).astype(np.float32)).to(device)


def torch_prepare(frames, picked, factor, order, flip, table):
    """mvp_prepare_frames_u8 from torch ops; every intermediate is a tensor of the whole batch"""
    shape = tuple(picked.shape)
    x = frames[picked.reshape(-1)].to(torch.int32)  # (Nf,H,W,3)
    Nf, H, W, _ = x.shape
    n = H * W
    factor, order = factor.reshape(Nf, 3), order.reshape(Nf, 3).long()
    for i in range(3):
        op = order[:, i]
        f = factor.gather(1, op.clamp(max=2)[:, None]).view(Nf, 1, 1, 1)
        gray = (x[..., 0] * 19595 + x[..., 1] * 38470 + x[..., 2] * 7471 + 0x8000) >> 16
        s = gray.sum((1, 2), dtype=torch.int64)
        m = ((2 * s + n) // (2 * n)).to(torch.int32).view(Nf, 1, 1, 1)
        opv = op.view(Nf, 1, 1, 1)
        d = torch.where(opv == 0, torch.zeros_like(x), torch.where(opv == 1, m.expand_as(x), gray[..., None].expand_as(x)))
        t = d.float() + f * (x - d).float()
        y = torch.where(t > 0, t.clamp(max=255.0), torch.zeros_like(t)).to(torch.int32)
        x = torch.where(opv <= 2, y, x)
    xl = x.long()
    val = torch.stack([table[c][xl[..., c]] for c in range(3)], dim=1)  # (Nf,3,H,W)
    val = torch.where(flip.reshape(Nf, 1, 1, 1).bool(), val.flip(-1), val)
    return val.view(shape + (3, H, W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chunks', type=int, default=32)
    ap.add_argument('--picks', type=int, default=3)
    ap.add_argument('--frames', type=int, default=1500)
    ap.add_argument('--height', type=int, default=120)
    ap.add_argument('--width', type=int, default=160)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile-only', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_frames needs the GPU: nothing here is measured on a CPU')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import augment as A
    dev = torch.device('cuda:0')
    B, nv, F, H, W = args.chunks, args.picks, args.frames, args.height, args.width
    gen = torch.Generator(device=dev).manual_seed(1)
    store = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, generator=gen, device=dev)
    picked = torch.randint(0, F, (B, nv), generator=gen, device=dev)
    factor, order = A.draw_color_jitter((B, nv), (0.4, 0.4, 0.4), dev, generator=gen)
    flip = A.draw_flip((B, nv), 0.5, dev, generator=gen)
    table = byte_table(dev)
    store_f = torch.stack([table[c][store[..., c].long()] for c in range(3)], dim=1)  # (F,3,H,W) float32: the store of variant (c)

    a = lambda: ops.prepare_frames(store, picked, factor=factor, order=order, flip=flip, normalizer=NORMALIZER)
    b = lambda: torch_prepare(store, picked, factor, order, flip, table)

    def c():
        images = store_f[picked].contiguous()
        return torch.where(flip.bool().view(B, nv, 1, 1, 1), images.flip(-1), images)
    for _ in range(3):
        ra, rb, rc = a(), b(), c()
    torch.cuda.synchronize()
    if args.profile_only:
        for _ in range(5):
            a()
        torch.cuda.synchronize()
        return
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)), '(a) and (b) must give the same bits'
    plain = ops.prepare_frames(store, picked, flip=flip, normalizer=NORMALIZER)
    assert torch.equal(plain.view(torch.int32), rc.view(torch.int32)), '(a) without a jitter and (c) must give the same bits'
    del ra, rb, rc, plain
    tm = alternate({'a': a, 'b': b, 'c': c}, args.windows, lambda f: device_ms(f, 20))
    sa, sb, sc = stats(tm['a']), stats(tm['b']), stats(tm['c'])
    noise = lambda x, y: (x['max_ms'] - x['min_ms']) + (y['max_ms'] - y['min_ms'])
    frame_bytes = H * W * 3
    moved = B * nv * frame_bytes * (2 + 4)
    res = {'device': torch.cuda.get_device_name(0), 'chunks': B, 'picks': nv, 'store_frames': F, 'height': H, 'width': W,
           'a_prepare_frames': dict(sa, host_syncs=count_syncs(a)), 'b_torch_ops': dict(sb, host_syncs=count_syncs(b)),
           'c_float_gather_no_jitter': dict(sc, host_syncs=count_syncs(c)),
           'b_over_a': round(sb['median_ms'] / sa['median_ms'], 2), 'c_over_a': round(sc['median_ms'] / sa['median_ms'], 2),
           'a_beats_b_beyond_the_spread': bool(sb['median_ms'] - sa['median_ms'] > noise(sa, sb)),
           'a_beats_c_beyond_the_spread': bool(sc['median_ms'] - sa['median_ms'] > noise(sa, sc)),
           'a_equals_b_bit_for_bit': True,
           'bound_a': {'bytes_moved': moved, 'hbm_bound_ms': round(moved / HBM_PEAK * 1e3, 5)},
           'store_bytes': {'this_run_uint8': F * frame_bytes, 'this_run_float32': F * frame_bytes * 4,
                           'scannet_frames': SCANNET_FRAMES, 'scannet_uint8': SCANNET_FRAMES * frame_bytes,
                           'scannet_float32': SCANNET_FRAMES * frame_bytes * 4}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

"""The gradient of the lift with respect to the 2D feature map: the atomic route (mvp_lift_gather_backward_f32: a memset of the (B,P,C)
map + one float atomic per element) beside the gather route (mvp_lift_backward_f32: transposed-index build + one store per map row).
Prints ONE JSON line (and writes it to --out).  Not part of bench.py.

    python tools/bench_lift_backward.py [--shape workload|dense|both] [--windows 9] [--reps 10] [--only atomic|gather] [--out FILE]

Shapes: workload B = 32, nv = 3, 120 x 160, N = 8192, k = 3, C = 64; dense B = 2, nv = 5, 240 x 320, N = 32768, k = 5, C = 64.  The
indices come from a real ops.lift of mvpnet_amd.synthetic chunks, so the list lengths are the workload's (reported as `lists`).

Method: everything is warmed up first; the routes ALTERNATE inside the same process, window after window; a window is `reps` calls between
two device events; the figure is the median over the windows and `spread` the (max - min) / median over them.  Beside the two routes:
`zero_map_launch` = the gather kernel with no lists (N = 0: it writes the whole map and reads nothing) and `memset` = the zero fill of the
map that the atomic route starts with.  `gather_is_default`: the gather route's median is no higher than the atomic route's beyond the
atomic route's own spread.  --only atomic|gather runs one route alone, for a kernel trace of it (the time of each of the gather route's
two launches, and with `bytes` the achieved fraction of the HBM peak, come from there).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {'workload': dict(B=32, nv=3, h=120, w=160, N=8192, k=3, C=64), 'dense': dict(B=2, nv=5, h=240, w=320, N=32768, k=5, C=64)}


def stats(xs):
    med = statistics.median(xs)
    return {'median_us': round(med * 1e3, 2), 'min_us': round(min(xs) * 1e3, 2), 'max_us': round(max(xs) * 1e3, 2),
            'spread': round((max(xs) - min(xs)) / med, 4), 'windows': len(xs)}


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def indices(dev, B, nv, h, w, N, k, **_):
    """knn_indices (B,N,k) of a real lift of synthetic chunks."""
    import mvpnet_amd.ops as ops
    from mvpnet_amd.synthetic import make_batch
    bt = make_batch(500, B, config=3, nb_pts=N, nv=nv, h=h, w=w, k=k, with_feature=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = t(np.repeat(bt['cam_matrix'][None, None, :3, :3], nv, 1).repeat(B, 0))
    feat = torch.zeros(B, nv, h, w, 4, device=dev)
    return ops.lift(feat, t(bt['depth_mm'].astype(np.int16)), t(bt['kinv']), cam, t(bt['pose']), t(bt['points']), k=k, box=t(bt['pixel_box']))[2]


def measure(dev, shape, windows, reps, only=None):
    from mvpnet_amd import _lib as L
    B, nv, h, w, N, k, C = (shape[key] for key in ('B', 'nv', 'h', 'w', 'N', 'k', 'C'))
    P, E = nv * h * w, N * k
    knn = indices(dev, **shape)
    g = torch.randn(B, N, k, C, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    out_a, out_g = torch.empty(B, P, C, device=dev), torch.empty(B, P, C, device=dev)
    ws = torch.empty(L.lib().mvp_lift_backward_workspace_bytes(B, P, N, k), dtype=torch.uint8, device=dev)
    atomic = lambda: L.call('mvp_lift_gather_backward_f32', g, L.ptr(g), L.ptr(knn), B, P, C, N, k, L.ptr(out_a))
    gather = lambda: L.call('mvp_lift_backward_f32', g, L.ptr(g), L.ptr(knn), B, P, C, N, k, L.ptr(ws), L.ptr(out_g))
    if only:
        fn = atomic if only == 'atomic' else gather
        for _ in range(3):
            fn()
        return {'shape': shape, only: stats([device_ms(fn, reps) for _ in range(windows)])}
    for _ in range(3):
        atomic(), gather()
    torch.cuda.synchronize()
    ix = knn.view(B, E)
    valid = (ix >= 0) & (ix < P)
    lengths = torch.zeros(B * P, dtype=torch.int64, device=dev)
    lengths.scatter_add_(0, (ix + torch.arange(B, device=dev).view(B, 1) * P)[valid], torch.ones(int(valid.sum()), dtype=torch.int64, device=dev))
    res = {'shape': shape, 'lists': {'edges': B * E, 'valid': int(valid.sum()), 'pixels_named': int((lengths > 0).sum()), 'pixels': B * P,
                                     'max': int(lengths.max()), 'over_16': int((lengths > 16).sum())},
           'max_abs_difference_of_the_routes': float((out_a - out_g).abs().max())}
    zero_map = lambda: L.call('mvp_lift_backward_f32', g, L.ptr(g), L.ptr(knn), B, P, C, 0, k, L.ptr(ws), L.ptr(out_g))
    fill = lambda: out_a.zero_()
    for _ in range(3):
        zero_map(), fill()
    tm = {'atomic': [], 'gather': [], 'zero_map_launch': [], 'memset': []}
    for _ in range(windows):
        tm['atomic'].append(device_ms(atomic, reps))
        tm['gather'].append(device_ms(gather, reps))
        tm['zero_map_launch'].append(device_ms(zero_map, reps))
        tm['memset'].append(device_ms(fill, reps))
    for key, xs in tm.items():
        res[key] = stats(xs)
    a, n = statistics.median(tm['atomic']), statistics.median(tm['gather'])
    res['gather_over_atomic'] = round(n / a, 3)
    res['gather_is_default'] = bool(n <= a * (1.0 + res['atomic']['spread']))
    res['bytes'] = {'map_written': B * P * C * 4, 'gradient_read': int(valid.sum()) * C * 4, 'index_read_per_pass': B * E * 8}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=['workload', 'dense', 'both'], default='both')
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--only', choices=['atomic', 'gather'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_lift_backward needs the GPU: nothing here is measured on a CPU')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'reps_per_window': args.reps}
    for name in (['workload', 'dense'] if args.shape == 'both' else [args.shape]):
        res[name] = measure(dev, SHAPES[name], args.windows, args.reps, args.only)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

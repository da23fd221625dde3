"""The fused scene cloud (ops.CloudFuser: insert, finish, lookup) beside what a user could write before it from this library's parts:
ops.unproject -> voxel keys in torch -> torch.unique(return_inverse=True) -> index_add_ in float64.  Prints ONE JSON line (and writes it
to --out).  Not part of bench.py.

    python tools/bench_fuse_cloud.py [--frames 96] [--height 120] [--width 160] [--voxel 0.05] [--windows 9] [--reps 5] [--out FILE]

Scene: mvpnet_amd.synthetic.make_rgbd_scene(3, frames, h, w) with random uint8 colour frames.  Both routes return the points, the colours,
the counts and every pixel's point index; they are compared once (keys and counts must be equal; the composition's float64 means may
differ from the integer means in the last bit, reported as `max_abs_point_difference`).

Method: everything is warmed up first; the routes ALTERNATE inside the same process, window after window; a window is `reps` calls between
two device events (both routes read sizes back to the host inside the window: that wait is part of what a caller pays); the figure is
the median over the windows and `spread` the (max - min) / median over them.  `fused_is_faster` is claimed only when the gap between the
medians exceeds the two spreads together.  `insert`: the insert launch alone on an already filled table (every pixel finds its voxel),
with the bytes the frames hold (depth, colours, cameras) over its time = the achieved rate of reading the frames.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    med = statistics.median(xs)
    return {'median_ms': round(med, 4), 'min_ms': round(min(xs), 4), 'max_ms': round(max(xs), 4), 'spread': round((max(xs) - min(xs)) / med, 4),
            'windows': len(xs)}


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def composition(depth, kinv, pose, images, voxel):
    """The torch route: the same validity rule and keys, float64 sums."""
    import mvpnet_amd.ops as ops
    F = depth.size(0)
    xyz, mask = ops.unproject(depth[None], kinv.expand(F, 3, 3)[None].contiguous(), pose[None])
    x = xyz.view(-1, 3)
    i = torch.floor(x.double() / voxel)
    valid = mask.view(-1) & (torch.isfinite(x) & (x.abs() < 32768)).all(1) & ((i >= -2 ** 20) & (i < 2 ** 20)).all(1)
    b = i[valid].long() + 2 ** 20
    keys, inverse = torch.unique((b[:, 2] << 42) | (b[:, 1] << 21) | b[:, 0], return_inverse=True)
    n = keys.numel()
    count = torch.zeros(n, dtype=torch.int64, device=x.device).index_add_(0, inverse, torch.ones_like(inverse))
    points = (torch.zeros((n, 3), dtype=torch.float64, device=x.device).index_add_(0, inverse, x[valid].double()) / count[:, None]).float()
    csum = torch.zeros((n, 3), dtype=torch.int64, device=x.device).index_add_(0, inverse, images.view(-1, 3)[valid].long())
    colors = ((2 * csum + count[:, None]) // (2 * count[:, None])).to(torch.uint8)
    pixel_point = torch.full((x.size(0),), -1, dtype=torch.int32, device=x.device)
    pixel_point[valid] = inverse.int()
    return points, colors, count.int(), pixel_point.view(depth.shape), keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--height', type=int, default=120)
    ap.add_argument('--width', type=int, default=160)
    ap.add_argument('--voxel', type=float, default=0.05)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.windows < 7:
        ap.error('at least 7 windows')
    if not torch.cuda.is_available():
        sys.exit('bench_fuse_cloud.py needs the GPU: a CPU run says nothing about these times')
    from mvpnet_amd.ops.fuse_cloud import CloudFuser
    from mvpnet_amd.synthetic import make_rgbd_scene
    dev = torch.device('cuda:0')
    sc = make_rgbd_scene(3, args.frames, h=args.height, w=args.width)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, kinv, pose = t(sc['depth_mm'].astype(np.int16)), t(sc['kinv']), t(sc['pose'])
    images = t(np.random.RandomState(12).randint(0, 256, sc['depth_mm'].shape + (3,)).astype(np.uint8))
    pixels = depth.numel()

    def fused():
        fuser = CloudFuser(args.voxel, pixels, dev)
        points, colors, count = fuser.add(depth, kinv, pose, images).finish()
        return points, colors, count, fuser.lookup(depth, kinv, pose), fuser.keys

    torch_route = lambda: composition(depth, kinv, pose, images, args.voxel)
    for _ in range(3):
        a, b = fused(), torch_route()
    torch.cuda.synchronize()
    same = all(torch.equal(a[j], b[j]) for j in (2, 3, 4))
    res = {'frames': args.frames, 'height': args.height, 'width': args.width, 'voxel': args.voxel, 'pixels': pixels, 'voxels': int(a[4].numel()),
           'device': torch.cuda.get_device_name(0), 'keys_counts_and_pixel_points_equal': same,
           'colors_equal': bool(torch.equal(a[1], b[1])), 'max_abs_point_difference': float((a[0] - b[0]).abs().max())}
    filled = CloudFuser(args.voxel, pixels, dev).add(depth, kinv, pose, images)
    insert = lambda: filled.add(depth, kinv, pose, images)
    insert()
    tm = {'fused': [], 'torch_composition': [], 'insert': []}
    for _ in range(args.windows):
        tm['fused'].append(device_ms(fused, args.reps))
        tm['torch_composition'].append(device_ms(torch_route, args.reps))
        tm['insert'].append(device_ms(insert, args.reps))
    res.update({name: stats(xs) for name, xs in tm.items()})
    gap = abs(res['fused']['median_ms'] - res['torch_composition']['median_ms'])
    noise = res['fused']['spread'] * res['fused']['median_ms'] + res['torch_composition']['spread'] * res['torch_composition']['median_ms']
    res['fused_is_faster'] = bool(res['fused']['median_ms'] < res['torch_composition']['median_ms'] and gap > noise)
    res['torch_composition_is_faster'] = bool(res['torch_composition']['median_ms'] < res['fused']['median_ms'] and gap > noise)
    frame_bytes = depth.numel() * 2 + images.numel() + args.frames * (9 + 16) * 4
    res['insert']['frame_bytes'] = frame_bytes
    res['insert']['achieved_GB_per_s'] = round(frame_bytes / (res['insert']['median_ms'] * 1e-3) / 1e9, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

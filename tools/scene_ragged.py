"""A ragged scene end to end, measured: prepare_scene_bucketed + infer_scene next to prepare_scene + infer_scene (the per-chunk path: chunks
of a real scene have different sizes, so its batches hold one chunk each).  Prints ONE JSON line (and writes it to --out).

    python tools/scene_ragged.py [--points 200000] [--frames 48] [--repeats 5] [--min-nb-pts 2048] [--batch-size 32] [--out FILE]

Scene: synthetic.make_rgbd_scene (a 6.5 x 5.5 m room), chunks of 1.5 m at stride 0.5 m with the reference's threshold of 1000 points,
every chunk fed with all its points; model: MVPNet3D around PN2SSG with its default centroids (2048, 512, 128, 32) in eval mode, a
stand-in for the 2D network (the same in both paths).
Method: each path runs once first (that warms every shape it uses), then the two ALTERNATE --repeats times in this process; every figure
is a host clock around work that ends in a device synchronise; reported are the median over the repeats and the spread (max - min) /
median.  `faster_by_more_than_the_spread` compares the slowest bucketed repeat with the fastest per-chunk repeat, end to end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Feature2D(torch.nn.Module):
    """Stands in for the frozen 2D network: 64 feature channels that are fixed multiples of the image's three."""

    def forward(self, data):
        x = data['image']
        return {'feature': torch.cat([x * (0.05 * (i + 1)) for i in range(22)], 1)[:, :64].contiguous()}


def stats(xs):
    med = statistics.median(xs)
    return {'median_ms': round(med, 3), 'min_ms': round(min(xs), 3), 'max_ms': round(max(xs), 3), 'spread': round((max(xs) - min(xs)) / med, 4)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=200000)
    ap.add_argument('--frames', type=int, default=48)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-nb-pts', type=int, default=2048)
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_ragged needs the GPU: nothing here is measured on a CPU')
    from mvpnet_amd.mvpnet3d import MVPNet3D
    from mvpnet_amd.pn2 import PN2SSG
    from mvpnet_amd.scene import prepare_scene, prepare_scene_bucketed, infer_scene
    from mvpnet_amd.synthetic import make_rgbd_scene
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    h, w = 60, 80
    sc = make_rgbd_scene(0, args.frames, n_pts=args.points, h=h, w=w)
    pts, depth, pose = t(sc['points']), t(sc['depth_mm'].astype(np.int16)), t(sc['pose'])
    images = torch.from_numpy(np.random.RandomState(1).standard_normal((args.frames, 3, h, w)).astype(np.float32)).to(dev)
    torch.manual_seed(0)
    model = MVPNet3D(Feature2D(), '', PN2SSG(64, 20, dropout_prob=0.0), in_channels=64).to(dev).eval()
    kw = dict(chunk_size=(1.5, 1.5), chunk_stride=0.5, chunk_thresh=1000, chunk_margin=(0.2, 0.2), num_rgbd_frames=3, k=3, min_nb_pts=args.min_nb_pts)
    gen = lambda: torch.Generator(device=dev).manual_seed(7)  # the same base points in both paths and every repeat

    def per_chunk():
        (batches, inds, n), prep_ms = timed(lambda: prepare_scene(pts, depth, sc['cam_matrix'], pose, images, generator=gen(), **kw))
        out, infer_ms = timed(lambda: infer_scene(model, batches, inds, n))
        return batches, inds, out, prep_ms, infer_ms

    def bucketed():
        (batches, inds, n, _), prep_ms = timed(lambda: prepare_scene_bucketed(pts, depth, sc['cam_matrix'], pose, images, generator=gen(),
                                                                             batch_size=args.batch_size, **kw))
        out, infer_ms = timed(lambda: infer_scene(model, batches, inds, n))
        return batches, inds, out, prep_ms, infer_ms

    paths = {'per_chunk': per_chunk, 'bucketed': bucketed}
    first = {k: fn() for k, fn in paths.items()}  # warm-up of every shape; also what the two paths are compared on
    times = {k: {'prepare': [], 'infer': [], 'total': []} for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            _, _, _, prep_ms, infer_ms = fn()
            times[k]['prepare'].append(prep_ms)
            times[k]['infer'].append(infer_ms)
            times[k]['total'].append(prep_ms + infer_ms)
    res = {'device': torch.cuda.get_device_name(0), 'points': args.points, 'frames': args.frames, 'min_nb_pts': args.min_nb_pts,
           'batch_size': args.batch_size, 'repeats': args.repeats}
    for k in paths:
        batches, inds, _, _, _ = first[k]
        true_rows = sum(int(i.numel()) for i in inds)
        rows = sum(b['points'].size(0) * b['points'].size(2) for b in batches)
        res[k] = {'chunks': len(inds), 'batches': len(batches), 'true_rows': true_rows, 'rows_fed': rows, 'rows_fed_over_true_rows': round(rows / true_rows, 4),
                  'chunk_points_min_max': [min(int(i.numel()) for i in inds), max(int(i.numel()) for i in inds)],
                  'prepare': stats(times[k]['prepare']), 'infer_scene': stats(times[k]['infer']), 'end_to_end': stats(times[k]['total'])}
    (emean, elabel, ecnt), (mean, label, cnt) = first['per_chunk'][2], first['bucketed'][2]
    voted = ecnt > 0
    res['agreement'] = {'vote_counts_equal': bool(torch.equal(cnt, ecnt)), 'max_abs_mean_logit_difference': float((mean - emean).abs().max()),
                        'labels_changed': int((label != elabel).sum()), 'points_voted': int(voted.sum())}
    med = lambda k, what: statistics.median(times[k][what])
    res['speedup'] = {what: round(med('per_chunk', what) / med('bucketed', what), 2) for what in ('prepare', 'infer', 'total')}
    res['faster_by_more_than_the_spread'] = bool(max(times['bucketed']['total']) < min(times['per_chunk']['total']))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

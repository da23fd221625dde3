"""Whole-scene voting on the GPU, measured at the reference's shape (mvpnet/test_3d_scene.py: a scene of --points points, --votes
subsamples of --nb-pts points, --classes classes), beside what a user could assemble without it.  Prints ONE JSON line (and writes it
to --out).  Not part of bench.py.

    python tools/bench_scene_vote.py [--points 150000] [--nb-pts 32768] [--votes 3] [--classes 20] [--windows 7] [--reps 20] [--out FILE]
                                     [--no-sklearn] [--only fused|composed]

Method: everything is warmed up first; the two device variants ALTERNATE inside the same process, window after window; a window is
`reps` calls between two device events; the figure is the median over the windows and `spread` the (max - min) / median over them.

  fused      (a) ops.vote_nearest (grid build + one query launch that also adds the logits) followed by mvp_vote_finish_f32.
  composed   (b) what the library allowed before: the scene copied V times as queries of mvp_knn3_grid_f32, column 0 of its (V,n,3) int64
             index, a torch gather and sum in vote order, mvp_vote_finish_f32.  Its result is compared with (a)'s, bit for bit.
  sklearn    (c) the reference's loop on the host's cores, once, for context: NearestNeighbors(1, 'ball_tree').fit / kneighbors per vote
             and the `+=` (host clock).
  swept      share of the (point, vote) searches of (a) that swept all keys.
  --only     one variant alone, for a kernel trace of it.
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=150000)
    ap.add_argument('--nb-pts', type=int, default=32768)
    ap.add_argument('--votes', type=int, default=3)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--only', choices=['fused', 'composed'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_scene_vote needs the GPU: nothing here is measured on a CPU')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import _lib as L
    from tests.scene_vote_oracle import room_cloud  # the jittered room surface cloud of the tests and the fixture
    dev = torch.device('cuda:0')
    n, nb, V, C = args.points, args.nb_pts, args.votes, args.classes
    pts_np = room_cloud(n, 0)
    rs = np.random.RandomState(1)
    inds = np.stack([rs.choice(n, nb, replace=False) for _ in range(V)])
    pts = torch.from_numpy(pts_np).to(dev)
    keys = pts[torch.from_numpy(inds).to(dev)].contiguous()  # (V,nb,3)
    rows = torch.randn(V, nb, C, generator=torch.Generator().manual_seed(2)).to(dev)
    logits = rows.transpose(1, 2)  # (V,C,nb): the network's transposed view of row-major rows
    count = torch.full((n,), V, dtype=torch.int32, device=dev)
    mean = torch.empty((n, C), dtype=torch.float32, device=dev)
    label = torch.empty(n, dtype=torch.int64, device=dev)
    finish = lambda s: L.call('mvp_vote_finish_f32', s, L.ptr(s), L.ptr(count), n, C, L.ptr(mean), L.ptr(label))

    def fused():
        s = ops.vote_nearest(pts, keys, logits)
        finish(s)
        return s

    ws_bytes = int(L.lib().mvp_knn3_grid_workspace(V, n, nb))
    if ws_bytes == 0:
        raise SystemExit('bench_scene_vote: mvp_knn3_grid_workspace declines this shape (too few pairs or keys for the grid): nothing to compare with')
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def composed():
        q = pts.expand(V, n, 3).contiguous()
        idx = torch.empty((V, n, 3), dtype=torch.int64, device=dev)
        L.call('mvp_knn3_grid_f32', q, L.ptr(q), L.ptr(keys), V, n, nb, 1.0, L.ptr(idx), None, None, L.ptr(ws), ws.numel())
        nn = idx[:, :, 0]
        s = logits[0].t()[nn[0]]
        for v in range(1, V):
            s = s + logits[v].t()[nn[v]]
        finish(s)
        return s

    res = {'device': torch.cuda.get_device_name(0), 'points': n, 'nb_pts': nb, 'votes': V, 'classes': C, 'reps_per_window': args.reps}
    if args.only:
        fn = fused if args.only == 'fused' else composed
        for _ in range(3):
            fn()
        res[args.only] = stats([device_ms(fn, args.reps) for _ in range(args.windows)])
    else:
        for _ in range(3):
            a, b = fused(), composed()
        la = label.clone()
        fused()
        res['composed_equals_fused'] = bool(torch.equal(a, b)) and bool(torch.equal(la, label))
        tm = {'fused': [], 'composed': []}
        for _ in range(args.windows):
            tm['fused'].append(device_ms(fused, args.reps))
            tm['composed'].append(device_ms(composed, args.reps))
        res['fused'], res['composed'] = stats(tm['fused']), stats(tm['composed'])
        res['composed_over_fused'] = round(statistics.median(tm['composed']) / statistics.median(tm['fused']), 3)
        swept = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.vote_nearest(pts, keys, logits, swept=swept)
        res['swept'] = {'searches': n * V, 'swept': int(swept.item()), 'share': round(int(swept.item()) / (n * V), 6)}
        res['bytes_written_fused'] = n * C * 4 * 2 + n * 8  # sum, mean, label
        if not args.no_sklearn:
            from sklearn.neighbors import NearestNeighbors
            lg = rows.cpu().numpy()
            t0 = time.perf_counter()
            total = np.zeros((n, C), np.float32)
            for v in range(V):
                nbrs = NearestNeighbors(n_neighbors=1, algorithm='ball_tree').fit(pts_np[inds[v]])
                _, nn = nbrs.kneighbors(pts_np)
                total += lg[v][nn[:, 0]]
            total = total / V
            lab = np.argmax(total, axis=1)
            res['sklearn_host_ms_once'] = round((time.perf_counter() - t0) * 1e3, 1)
            res['sklearn_labels_differing'] = int((lab != la.cpu().numpy()).sum())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

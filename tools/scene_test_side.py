"""The test side on one MI355X at two operating points; writes a plain-text record (--out, default profiles/scene_test_side.txt).  Not
part of bench.py.

    python tools/scene_test_side.py [--points 150000] [--windows 7] [--finish-reps 50] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/scene_test_side.py --kernels-only
        (the finish launches alone, for a kernel trace in a run of its own: profiles/scene_finish_kernel_stats.csv)

Point 1, scene.infer_scene_3d: a synthetic scene (synthetic.make_rgbd_scene, the points only) at the reference script's defaults -- 1.5 m
windows at stride 0.5, thresh 1000, 2048 points at least -- through the full-size PN2SSG (in_channels 0, random weights, eval mode),
beside the same chunks fed ONE at a time through scene.infer_scene, each padded to max(n, 2048): the reference's loop shape
(mvpnet/test_3d_chunks.py:106-167) on this code base.  Both sides include the chunker.
Point 2, the finish: ops.ensemble_softmax + metric.DeviceEvaluator.update on M models' (n,C) logits beside the equivalent torch
expression on the device (softmax, sum, argmax, bincount) and beside the host path that existed before (the logits' argmax is taken on
the device for it too: .cpu() of the labels plus metric.Evaluator); the ensemble kernel alone against the HBM figure of DESIGN.md 5.
Method: everything is warmed up, the sides ALTERNATE inside one process, window after window, each window between two device events with
its reads inside; the figure is the median over the windows, `spread` the (max - min) / median."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8e12  # bytes/s, the figure DESIGN.md 5 divides by


def stats(xs):
    med = statistics.median(xs)
    return 'median %.3f ms  min %.3f  max %.3f  spread %.3f  windows %d' % (med, min(xs), max(xs), (max(xs) - min(xs)) / med, len(xs))


def device_ms(fn, reps=1):
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
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--finish-reps', type=int, default=50)
    ap.add_argument('--models', type=int, default=4)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--kernels-only', action='store_true', help='launch the finish kernels 60 times each and exit: the subject of a kernel trace')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_test_side.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_test_side needs the GPU: nothing here is measured on a CPU')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import metric
    from mvpnet_amd import scene as S
    from mvpnet_amd.pn2 import PN2SSG
    from mvpnet_amd.synthetic import make_rgbd_scene
    dev = torch.device('cuda:0')
    if args.kernels_only:
        n, M, C = args.points, args.models, args.classes
        g = torch.Generator().manual_seed(2)
        rows = [(torch.randn(n, C, generator=g) * 3).to(dev) for _ in range(M)]
        cols = [x.t().contiguous().t() for x in rows]  # the (C,n) network output viewed as rows: the dword path
        gt = torch.randint(0, C, (n,), generator=g).to(dev)
        ev = metric.DeviceEvaluator(['c%d' % i for i in range(C)])
        for _ in range(60):
            ev.update(ops.ensemble_softmax(rows)[1], gt)
            ops.ensemble_softmax(cols)
        torch.cuda.synchronize()
        return
    lines = ['the test side: scene.infer_scene_3d and the scene finish   (tools/scene_test_side.py)', 'device: %s' % torch.cuda.get_device_name(0), '']

    # ---- point 1 ----
    torch.manual_seed(0)
    model = PN2SSG(0, 20).to(dev).eval()
    pts = torch.from_numpy(make_rgbd_scene(0, 2, n_pts=args.points, h=30, w=40)['points'].astype(np.float32)).to(dev)
    n = pts.size(0)
    kw = dict(chunk_size=(1.5, 1.5), chunk_stride=0.5, chunk_thresh=1000, chunk_margin=(0.2, 0.2))

    def batched():
        return S.infer_scene_3d(model, pts, min_nb_pts=2048, pad_seed=5, **kw)

    def one_by_one():
        csr = S.CH.scene2chunks_csr(pts, kw['chunk_size'], kw['chunk_stride'], thresh=kw['chunk_thresh'], margin=kw['chunk_margin'])
        lengths = csr['lengths']
        base, at = [], 0
        for c in lengths:
            base.append(at)
            at += max(c, 2048)
        flat, _ = ops.pack_cloud(pts, csr['index'], csr['offsets'], lengths, base, [max(c, 2048) for c in lengths], seed=5)
        singles = [{'points': flat[3 * b:3 * (b + max(c, 2048))].view(1, 3, max(c, 2048))} for b, c in zip(base, lengths)]
        return S.infer_scene(model, singles, list(torch.split(csr['index'], lengths)), n)

    a, b = batched(), one_by_one()
    lengths = S.CH.scene2chunks_csr(pts, kw['chunk_size'], kw['chunk_stride'], thresh=kw['chunk_thresh'], margin=kw['chunk_margin'])['lengths']
    batches, _ = S.plan_buckets(lengths, min_nb_pts=2048)
    voted = a[2] > 0
    lines += ['point 1: infer_scene_3d, synthetic.make_rgbd_scene(0) with %d points, windows 1.5 m at stride 0.5, thresh 1000, min 2048; PN2SSG(0, 20) '
              'full size, random weights, eval' % n,
              '  chunks %d (points per chunk: min %d, median %d, max %d)   batches %d (sizes %s)'
              % (len(lengths), min(lengths), int(statistics.median(lengths)), max(lengths), len(batches), sorted({N for N, _ in batches})),
              '  results of the two sides: counts equal %s   max |mean-logit difference| %.3e   labels agreeing on voted points %.6f'
              % (bool(torch.equal(a[2], b[2])), float((a[0] - b[0]).abs().max()), float((a[1][voted] == b[1][voted]).float().mean()))]
    batched(), one_by_one()
    tm = {'batched': [], 'single': []}
    for i in range(args.windows):
        print('scene_test_side: window %d' % i, file=sys.stderr, flush=True)
        tm['batched'].append(device_ms(batched))
        tm['single'].append(device_ms(one_by_one))
    mb, ms = statistics.median(tm['batched']), statistics.median(tm['single'])
    lines += ['  ms per scene, whole call (chunker, pack, forward, vote):',
              '    infer_scene_3d (bucketed batches)        : ' + stats(tm['batched']),
              '    one chunk at a time through infer_scene  : ' + stats(tm['single']),
              '    scenes/s %.2f against %.2f   chunks/s %.0f against %.0f   one-at-a-time / batched %.2f'
              % (1e3 / mb, 1e3 / ms, len(lengths) * 1e3 / mb, len(lengths) * 1e3 / ms, ms / mb), '']
    del a, b

    # ---- point 2 ----
    M, C = args.models, args.classes
    g = torch.Generator().manual_seed(2)
    logits = [(torch.randn(n, C, generator=g) * 3).to(dev) for _ in range(M)]
    gt = torch.randint(0, C, (n,), generator=g).to(dev)
    gt[::11] = -100
    names = ['c%d' % i for i in range(C)]
    dev_ev, torch_mat, host_ev = metric.DeviceEvaluator(names), torch.zeros((C, C), dtype=torch.int64, device=dev), metric.Evaluator(names)

    def finish_kernels():
        _, label = ops.ensemble_softmax(logits)
        dev_ev.update(label, gt)

    def finish_torch():
        prob = torch.softmax(logits[0], 1)
        for x in logits[1:]:
            prob = prob + torch.softmax(x, 1)
        label = prob.argmax(1)
        keep = gt >= 0
        torch_mat.add_(torch.bincount(gt[keep] * C + label[keep], minlength=C * C).view(C, C))

    def finish_host():
        _, label = ops.ensemble_softmax(logits)
        host_ev.update(label.cpu().numpy(), gt.cpu().numpy())

    def kernel_only():
        ops.ensemble_softmax(logits)

    for fn in (finish_kernels, finish_torch, finish_host, kernel_only):
        fn(), fn()
    same = np.array_equal(dev_ev.confusion_matrix, host_ev.confusion_matrix)
    tf = {'kernels': [], 'torch': [], 'host': [], 'kernel': []}
    for _ in range(args.windows):
        tf['kernels'].append(device_ms(finish_kernels, args.finish_reps))
        tf['torch'].append(device_ms(finish_torch, args.finish_reps))
        tf['host'].append(device_ms(finish_host, args.finish_reps))
        tf['kernel'].append(device_ms(kernel_only, args.finish_reps))
    nbytes = M * n * C * 4 + n * (C * 4 + 8)
    mk = statistics.median(tf['kernel'])
    lines += ['point 2: the finish, n = %d, C = %d, M = %d (%d calls per window; nothing is read back inside a window except on the host path)'
              % (n, C, M, args.finish_reps),
              '  ops.ensemble_softmax + DeviceEvaluator.update (2 launches)          : ' + stats(tf['kernels']),
              '  torch on the device (softmax x M, adds, argmax, mask, bincount, add) : ' + stats(tf['torch']),
              '  ops.ensemble_softmax + .cpu() of labels and gt + metric.Evaluator    : ' + stats(tf['host']),
              '  ops.ensemble_softmax alone (with its two output allocations)         : ' + stats(tf['kernel']),
              '  the ensemble call moves %d bytes: %.3f TB/s achieved by the whole call, %.3f of the %.0f TB/s HBM peak'
              % (nbytes, nbytes / (mk * 1e-3) / 1e12, nbytes / (mk * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12),
              '  confusion matrices of the device and the host evaluator equal: %s' % same]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

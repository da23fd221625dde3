"""The whole-scene test of the 2D baseline on one MI355X: scene.infer_scene_2d beside the per-chunk loop it replaces, on the same scene.
Prints ONE JSON line (and writes it to --out).  Not part of bench.py.

    python tools/bench_scene_2d.py [--points 200000] [--frames 96] [--views 5] [--ks 1,3] [--windows 5] [--kernel-reps 20] [--out FILE]

Scene: synthetic.make_rgbd_scene with 160x120 frames, 1.5 m windows at stride 0.5; network: the real UNetResNet34 (20 classes, random
weights, eval mode).  Method: everything is warmed up first; the two paths ALTERNATE inside the same process, window after window, one
call per window between two device events (a call holds a device-to-host read, so the figure is the call as a user pays it); the
figure is the median over the windows and `spread` the (max - min) / median over them.

  scene     (a) scene.infer_scene_2d: every distinct picked frame through the 2D network once, pixel k-NN in bucketed batches, one
                lift_vote launch, mvp_vote_finish_f32.
  loop      (b) the existing MVPNet2D on one chunk at a time (B = 1, its own `views` frames: the reference's loop), dist.vote_scene.
  net_2d    the 2D network alone: on the distinct frames in batches of 32 (what (a) runs) and on chunks x views frames in batches of
            `views` (what (b) runs).
  stages    the chunker + frame selection alone, (a)'s whole preparation (chunks, logit store, bucketed pixel k-NN), and (b)'s per-chunk
            frame gathers + un-projection + pixel k-NN without the network.
  kernel    mvp_lift_vote_f32 alone on (a)'s inputs, with its nominal bytes (k-NN rows + k logit rows per position + the sums) per
            second, beside the three launches it replaces on the same indices -- mvp_lift_gather_f32 into (chunks, Nmax, k, C),
            mean over k, mvp_vote_gather_f32 -- with every chunk padded to the longest one (`padding` = padded rows / real rows: that
            path has no ragged form; its frame logits are gathered per chunk beforehand, outside the timing)."""
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
    ap.add_argument('--points', type=int, default=200000)
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--views', type=int, default=5)
    ap.add_argument('--ks', default='1,3')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--kernel-reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_scene_2d needs the GPU: nothing here is measured on a CPU')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import _lib as L
    from mvpnet_amd import dist as D
    from mvpnet_amd import scene as S
    from mvpnet_amd.mvpnet2d import MVPNet2D
    from mvpnet_amd.synthetic import make_rgbd_scene
    from mvpnet_amd.unet_resnet34 import UNetResNet34
    dev = torch.device('cuda:0')
    h, w, nv, C = 120, 160, args.views, 20
    sc = make_rgbd_scene(0, args.frames, n_pts=args.points, h=h, w=w)
    pts = torch.from_numpy(sc['points']).to(dev)
    depth = torch.from_numpy(sc['depth_mm'].astype(np.int16)).to(dev)
    pose = torch.from_numpy(sc['pose']).to(dev)
    images = torch.randn(args.frames, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    torch.manual_seed(2)
    model = MVPNet2D(UNetResNet34(C)).to(dev).eval()
    chunk = dict(chunk_size=(1.5, 1.5), chunk_stride=0.5, chunk_thresh=1000, chunk_margin=(0.2, 0.2))
    base, ov = S.CH.compute_rgbd_overlap(pts, depth, sc['cam_matrix'], pose, generator=torch.Generator(device=dev).manual_seed(3), packed=True)
    n = pts.size(0)
    res = {'device': torch.cuda.get_device_name(0), 'points': n, 'frames': args.frames, 'frame_size': [w, h], 'views': nv, 'classes': C}

    for k in [int(x) for x in args.ks.split(',')]:
        print('bench_scene_2d: k = %d' % k, file=sys.stderr, flush=True)
        kw = dict(num_rgbd_frames=nv, k=k, overlap=(base, ov), **chunk)
        csr = S._scene_chunks(pts, depth, sc['cam_matrix'], pose, (base, ov), nv, chunk['chunk_size'], chunk['chunk_stride'], chunk['chunk_thresh'],
                              chunk['chunk_margin'], 2000, 0.1, None)
        batch = S._scene_batcher(dev, depth, sc['cam_matrix'], pose, images, None, 'bench_scene_2d', k)
        chunk_inds = list(torch.split(csr['index'], csr['lengths']))
        num_chunks, width = len(chunk_inds), max(csr['lengths'])
        chunk_pts = [pts[ind].t().contiguous()[None] for ind in chunk_inds]

        def scene_path():
            return S.infer_scene_2d(model, pts, depth, sc['cam_matrix'], pose, images, **kw)

        def loop_path():
            logits = torch.zeros((num_chunks, C, width), device=dev)
            with torch.no_grad():
                for c in range(num_chunks):
                    out = model(batch(csr['picked'][c:c + 1], chunk_pts[c], csr['pixel_box'][c:c + 1]))['seg_logit']
                    logits[c, :, :out.size(2)] = out[0]
            return D.vote_scene(logits, chunk_inds, n)

        a, b = scene_path(), loop_path()
        scene_path(), loop_path()
        r = {'chunks': num_chunks, 'chunk_views': num_chunks * nv, 'positions': int(sum(csr['lengths'])),
             'count_equal': bool(torch.equal(a[2], b[2])), 'labels_differing': int((a[1] != b[1]).sum()),
             'max_abs_mean_difference': float((a[0] - b[0]).abs().max())}
        tm = {'scene': [], 'loop': []}
        for _ in range(args.windows):
            tm['scene'].append(device_ms(scene_path))
            tm['loop'].append(device_ms(loop_path))
        r['scene'], r['loop'] = stats(tm['scene']), stats(tm['loop'])
        r['loop_over_scene'] = round(statistics.median(tm['loop']) / statistics.median(tm['scene']), 3)

        print('bench_scene_2d: paths timed', file=sys.stderr, flush=True)
        # the 2D network alone, as each path runs it
        parts = S._scene_2d_inputs(model, pts, depth, sc['cam_matrix'], pose, images, lift_depth=None, num_base_pts=2000, radius=0.1, generator=None,
                                   image_normalizer=None, channels_last=False, frame_batch=32, **kw)
        U = parts['logit'].size(0)
        r['distinct_frames'] = U
        distinct = torch.unique(parts['picked'])
        net = model.net_2d

        def net_distinct():
            with torch.no_grad():
                for lo in range(0, U, 32):
                    net({'image': images[distinct[lo:lo + 32]].contiguous()})

        def net_per_chunk():
            with torch.no_grad():
                for c in range(num_chunks):
                    net({'image': images[parts['picked'][c]].contiguous()})

        net_distinct(), net_per_chunk()
        r['net_2d_distinct'] = stats([device_ms(net_distinct) for _ in range(args.windows)])
        r['net_2d_per_chunk'] = stats([device_ms(net_per_chunk) for _ in range(args.windows)])

        # where the rest of each path goes: the chunker + frame selection, (a)'s whole preparation (chunks, store, bucketed k-NN), and
        # (b)'s per-chunk un-projection + pixel k-NN (B = 1) without the network
        def chunks_only():
            S._scene_chunks(pts, depth, sc['cam_matrix'], pose, (base, ov), nv, chunk['chunk_size'], chunk['chunk_stride'], chunk['chunk_thresh'],
                            chunk['chunk_margin'], 2000, 0.1, None)

        def prepare_only():
            S._scene_2d_inputs(model, pts, depth, sc['cam_matrix'], pose, images, lift_depth=None, num_base_pts=2000, radius=0.1, generator=None,
                               image_normalizer=None, channels_last=False, frame_batch=32, **kw)

        def knn_per_chunk():
            for c in range(num_chunks):
                d = batch(csr['picked'][c:c + 1], chunk_pts[c], csr['pixel_box'][c:c + 1])
                xyz, mask = ops.unproject(d['depth'], d['kinv'], d['pose'], d['pixel_box'])
                ops.pixel_knn(xyz, mask, chunk_pts[c].transpose(1, 2).contiguous(), k, cam=d['cam_matrix'], pose=d['pose'])

        r['stages'] = {'scene_chunks': stats([device_ms(chunks_only) for _ in range(args.windows)]),
                       'scene_prepare_all': stats([device_ms(prepare_only) for _ in range(args.windows)]),
                       'loop_gather_unproject_knn': stats([device_ms(knn_per_chunk) for _ in range(args.windows)])}

        # the kernel alone, beside the three launches it replaces
        plan = D._vote_plan(parts['chunk_inds'], n, dev)
        fused = lambda: ops.lift_vote(parts['logit'], parts['view_frame'], parts['knn'], parts['knn_base'], None, n, plan=plan)
        knn_pad = torch.full((num_chunks, width, k), -1, dtype=torch.int64, device=dev)
        for c, (b0, ln) in enumerate(zip(parts['knn_base'], csr['lengths'])):
            knn_pad[c, :ln] = parts['knn'][b0:b0 + ln]
        logit_cl = parts['logit'].permute(0, 2, 3, 1)[parts['view_frame'].long()].contiguous()  # (chunks,nv,h,w,C): the loop's per-chunk 2D output

        def composed():
            gathered, _ = ops.lift_gather(logit_cl, None, knn_pad)       # (chunks,Nmax,k,C)
            means = gathered.mean(2)                                     # (chunks,Nmax,C)
            s = torch.empty((n, C), dtype=torch.float32, device=dev)
            cnt = torch.empty((n,), dtype=torch.int32, device=dev)
            L.call('mvp_vote_gather_f32', s, L.ptr(means), means.stride(0), means.stride(1), means.stride(2), L.ptr(plan['chunk_offsets']), num_chunks,
                   L.ptr(plan['pt_offsets']), L.ptr(plan['pt_slots']), n, C, L.ptr(s), L.ptr(cnt))
            return s, cnt

        (fs, fc), (cs, cc) = fused(), composed()
        tk = {'lift_vote': [], 'composed': []}
        for _ in range(args.windows):
            tk['lift_vote'].append(device_ms(fused, args.kernel_reps))
            tk['composed'].append(device_ms(composed, args.kernel_reps))
        positions = r['positions']
        nominal = positions * k * 8 + positions * k * C * 4 + n * C * 4 + n * 4 + positions * 4
        r['kernel'] = {'lift_vote': stats(tk['lift_vote']), 'lift_gather_mean_vote_gather': stats(tk['composed']),
                       'composed_over_lift_vote': round(statistics.median(tk['composed']) / statistics.median(tk['lift_vote']), 3),
                       'lift_vote_nominal_bytes': nominal,
                       'lift_vote_nominal_GBps': round(nominal / statistics.median(tk['lift_vote']) / 1e6, 1),
                       'padding': round(num_chunks * width / positions, 3), 'count_equal': bool(torch.equal(fc, cc)),
                       'max_abs_sum_difference': float((fs - cs).abs().max())}
        res['k%d' % k] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

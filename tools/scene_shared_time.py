"""The whole-scene test of MVPNet on one MI355X: scene.infer_scene_shared (every distinct frame through the 2D network once per store)
beside the path it restates (scene.prepare_scene_bucketed then scene.infer_scene: every batch runs the 2D network on its own B * nv
frames), on the same synthetic scene.  Writes a plain-text record (--out, default profiles/scene_shared.txt).  Not part of bench.py.

    python tools/scene_shared_time.py [--points 200000] [--frames 96] [--windows 7] [--kernel-reps 50] [--out FILE]

Model: the YAML's real UNetResNet34 + PN2SSG (config.build_model_mvpnet_3d, no checkpoint: random weights, frozen folded 2D branch, eval
mode); scene: synthetic.make_rgbd_scene with 160x120 frames, 1.5 m windows at stride 0.5, 3 views, k = 3, the overlap computed once.
Method: both paths are warmed up, then ALTERNATE inside the same process, window after window, one whole call per window between two
device events (each call holds its device-to-host reads, so the figure is the call as a user pays it); the figure is the median over the
windows, `spread` the (max - min) / median over them.  The lifting entries are timed alone on one batch of the scene's shape (B = 32,
3 views, 8192 points, C = 64): mvp_lift_store_f32 on a store of the batch's distinct frames against mvp_lift_f32 on the materialised
(B,nv,h,w,C) tensor, same workspace and outputs, alternating; each call is the prepare launch plus the search / gather launch, and the
prepare launch is the same kernel on both sides."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument('--points', type=int, default=200000)
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--kernel-reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_shared.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_shared_time needs the GPU: nothing here is measured on a CPU')
    import json
    import yaml
    import mvpnet_amd.ops as ops
    from mvpnet_amd import _lib as L
    from mvpnet_amd import config as C
    from mvpnet_amd import scene as S
    from mvpnet_amd.synthetic import make_rgbd_scene
    dev = torch.device('cuda:0')
    with open(os.path.join(ROOT, 'tests', 'golden', 'configs.json')) as f:
        cfg = C.load_cfg(text=yaml.safe_dump(json.load(f)['mvpnet_3d_unet_resnet34_pn2ssg']))
    torch.manual_seed(0)
    model = C.build_model_mvpnet_3d(cfg, load_2d_ckpt=False).to(dev).eval()
    seen = [0]
    model.net_2d.register_forward_pre_hook(lambda mod, inp: seen.__setitem__(0, seen[0] + inp[0]['image'].size(0)))

    h, w, nv, k = 120, 160, 3, 3
    sc = make_rgbd_scene(0, args.frames, n_pts=args.points, h=h, w=w)
    pts = torch.from_numpy(sc['points']).to(dev)
    depth = torch.from_numpy(sc['depth_mm'].astype(np.int16)).to(dev)
    pose = torch.from_numpy(sc['pose']).to(dev)
    images = torch.randn(args.frames, 3, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    overlap = S.CH.compute_rgbd_overlap(pts, depth, sc['cam_matrix'], pose, generator=torch.Generator(device=dev).manual_seed(3), packed=True)
    kw = dict(chunk_size=(1.5, 1.5), chunk_stride=0.5, chunk_thresh=1000, chunk_margin=(0.2, 0.2), num_rgbd_frames=nv, k=k, overlap=overlap,
              pad_seed=5)

    def parent_path():
        batches, inds, n, _ = S.prepare_scene_bucketed(pts, depth, sc['cam_matrix'], pose, images, **kw)
        return S.infer_scene(model, batches, inds, n)

    def shared_path():
        return S.infer_scene_shared(model, pts, depth, sc['cam_matrix'], pose, images, **kw)

    lines = ['scene.infer_scene_shared beside prepare_scene_bucketed + infer_scene   (tools/scene_shared_time.py)',
             'device: %s' % torch.cuda.get_device_name(0),
             'scene: synthetic.make_rgbd_scene(0), %d points, %d frames of %dx%d, %d views per chunk, k = %d, windows 1.5 m at stride 0.5'
             % (pts.size(0), args.frames, w, h, nv, k),
             'model: UNetResNet34 + PN2SSG from the YAML, random weights, eval mode', '']
    seen[0] = 0
    a = parent_path()
    frames_parent, seen[0] = seen[0], 0
    b = shared_path()
    frames_shared = seen[0]
    csr = S._scene_chunks(pts, depth, sc['cam_matrix'], pose, overlap, nv, kw['chunk_size'], kw['chunk_stride'], kw['chunk_thresh'], kw['chunk_margin'],
                          2000, 0.1, None)
    chunks = len(csr['lengths'])
    lines += ['chunks: %d   (chunk views: %d, distinct picked frames: %d)' % (chunks, chunks * nv, int(torch.unique(csr['picked']).numel())),
              'frames through the 2D network per scene:   parent path %d   infer_scene_shared %d   (ratio %.2f)'
              % (frames_parent, frames_shared, frames_parent / max(frames_shared, 1))]
    voted = a[2] > 0
    lines += ['results of the two paths (informational: with MIOpen a frame\'s feature bits may depend on the 2D batch size):',
              '  counts equal: %s   max |mean-logit difference|: %.3e   labels agreeing on voted points: %.6f'
              % (bool(torch.equal(a[2], b[2])), float((a[0] - b[0]).abs().max()), float((a[1][voted] == b[1][voted]).float().mean())), '']
    parent_path(), shared_path()  # second warm-up of every shape
    tm = {'parent': [], 'shared': []}
    for i in range(args.windows):
        print('scene_shared_time: window %d' % i, file=sys.stderr, flush=True)
        tm['parent'].append(device_ms(parent_path))
        tm['shared'].append(device_ms(shared_path))
    lines += ['ms per scene, whole call (chunker and frame selection included on both sides):',
              '  prepare_scene_bucketed + infer_scene : ' + stats(tm['parent']),
              '  infer_scene_shared                   : ' + stats(tm['shared']),
              '  parent / shared                      : %.3f' % (statistics.median(tm['parent']) / statistics.median(tm['shared'])), '']

    # the parts: the 2D network alone on each path's frames, in each path's batch sizes
    batches = S.prepare_scene_bucketed(pts, depth, sc['cam_matrix'], pose, images, **kw)[0]
    distinct = torch.unique(csr['picked'])

    def net_parent():
        with torch.no_grad():
            for bt in batches:
                x = bt['images']
                model.net_2d({'image': x.reshape(-1, *x.shape[2:])})

    def net_shared():
        with torch.no_grad():
            for lo in range(0, distinct.numel(), 32):
                model.net_2d({'image': images[distinct[lo:lo + 32]].contiguous()})

    net_parent(), net_shared()
    t2 = {'parent': [], 'shared': []}
    for _ in range(args.windows):
        t2['parent'].append(device_ms(net_parent))
        t2['shared'].append(device_ms(net_shared))
    lines += ['the 2D network alone on each path\'s frames:',
              '  per batch, B * nv frames (%d in all) : ' % frames_parent + stats(t2['parent']),
              '  distinct frames, 32 at a time (%d)   : ' % distinct.numel() + stats(t2['shared']), '']

    # the lifting entries alone on one batch of the YAML's shape
    B, N, Cf = 32, 8192, int(model.feat_aggreg.in_channels)
    g = torch.Generator().manual_seed(4)
    first = int(torch.randint(0, max(chunks - B, 1), (1,), generator=g))
    sel = csr['picked'][first:first + B]
    B = sel.size(0)
    cam = torch.from_numpy(sc['cam_matrix'][:3, :3].astype(np.float32)).to(dev).expand(B, nv, 3, 3).contiguous()
    kinv = torch.from_numpy(np.linalg.inv(sc['cam_matrix'][:3, :3]).astype(np.float32)).to(dev).expand(B, nv, 3, 3).contiguous()
    qpts = torch.stack([pts[ind[torch.randint(0, ind.numel(), (N,), generator=g).to(dev)]]
                        for ind in torch.split(csr['index'], csr['lengths'])[first:first + B]]).contiguous()
    frames_b, slot = torch.unique(sel, return_inverse=True)
    store = torch.randn(frames_b.numel(), h, w, Cf, generator=g).to(dev)
    view_slot = slot.to(torch.int32).contiguous()
    feature = store[slot].contiguous()
    bdepth, bpose, box = depth[sel].contiguous(), pose[sel].contiguous(), csr['pixel_box'][first:first + B].contiguous()
    ws = torch.empty(L.lib().mvp_lift_workspace_bytes(B, nv, h, w, N), dtype=torch.uint8, device=dev)
    knn = torch.empty((B, N, k), dtype=torch.int64, device=dev)
    gfeat = torch.empty((B, N, k, Cf), dtype=torch.float32, device=dev)
    gxyz = torch.empty((B, N, k, 3), dtype=torch.float32, device=dev)

    def lift_plain():
        L.call('mvp_lift_f32', bdepth, L.ptr(bdepth), 1, L.ptr(kinv), L.ptr(cam), L.ptr(bpose), L.ptr(box), L.ptr(qpts), L.ptr(feature), B, nv, h, w, N,
               Cf, k, L.ptr(ws), L.ptr(knn), L.ptr(gfeat), L.ptr(gxyz), None, None)

    def lift_store():
        L.call('mvp_lift_store_f32', bdepth, L.ptr(bdepth), 1, L.ptr(kinv), L.ptr(cam), L.ptr(bpose), L.ptr(box), L.ptr(qpts), L.ptr(store),
               L.ptr(view_slot), store.size(0), B, nv, h, w, N, Cf, k, L.ptr(ws), L.ptr(knn), L.ptr(gfeat), L.ptr(gxyz))

    lift_plain()
    want = (knn.clone(), gfeat.clone(), gxyz.clone())
    lift_store()
    same = torch.equal(knn, want[0]) and torch.equal(gfeat, want[1]) and torch.equal(gxyz, want[2])
    tl = {'plain': [], 'store': []}
    for _ in range(args.windows):
        tl['plain'].append(device_ms(lift_plain, args.kernel_reps))
        tl['store'].append(device_ms(lift_store, args.kernel_reps))
    lines += ['the lifting entries alone, B = %d chunks x %d views of %dx%d, N = %d, C = %d, k = %d, %d distinct frames in the store (prepare launch + '
              'search / gather launch per call, %d calls per window):' % (B, nv, w, h, N, Cf, k, store.size(0), args.kernel_reps),
              '  mvp_lift_f32 (lift_knn_gather_kernel<3, 256>, (B,nv,h,w,C) feature)      : ' + stats(tl['plain']),
              '  mvp_lift_store_f32 (lift_knn_gather_store_kernel<3, 256>, shared store)  : ' + stats(tl['store']),
              '  store / plain: %.3f   outputs bit-equal: %s' % (statistics.median(tl['store']) / statistics.median(tl['plain']), same),
              '  the materialised tensor the store call does not need: %d bytes per batch' % (feature.numel() * 4)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

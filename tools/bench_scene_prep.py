"""Scene preparation on the GPU, measured: the RGB-D overlap kernel, batched frame selection and prepare_scene, each next to what a
user would write without them.  Prints ONE JSON line (and writes it to --out).

    python tools/bench_scene_prep.py [--frames 1500] [--base 2000] [--chunks 64] [--picks 3] [--windows 7] [--out FILE]

Method: everything is warmed up first; the variants of one comparison ALTERNATE inside the same process, window after window; a
window is timed with device events (host clock around a synchronise for the Python-loop baselines, which synchronise anyway); the
figure is the median over the windows and `spread` the (max - min) / median over them.

  overlap    mvp_frame_overlap_u16 over all frames; beside it, on the first --torch-frames frames (the plain formulation needs
             fb * h * w * nb * 12 bytes of temporaries, so it goes frame batch by frame batch), the kernel and the torch formulation:
             un-project, broadcast difference -> squared sum -> argmin -> threshold -> scatter.
  bound      the kernel's VALU bound: F * h * w * nb pair evaluations x 8 non-fused fp32 operations (3 sub, 3 mul, 2 add of the pinned
             expression) over HALF the fp32 vector peak (the 157.3 TFLOP/s figure counts a fused multiply-add as two operations on
             each half of a packed instruction; non-fused packed operations reach half of it).
  select     select_frames_batched for all chunks against a Python loop of chunks.select_frames over the same chunks, with the
             host synchronisations of each (counted by torch's sync debug mode where it is available).
  pipeline   prepare_scene wall time for the fixture-style scene (96 frames of 80x60, 60000 points, 2000 base points).
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_VECTOR_PEAK = 157.3e12  # FLOP/s, fused multiply-adds counted twice (MI355X)
HBM_PEAK = 8.0e12            # bytes/s
OPS_PER_PAIR = 8             # (dx*dx + dy*dy) + dz*dz with dx, dy, dz formed first: 3 sub, 3 mul, 2 add, nothing fused


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


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(variants, windows, timer):
    """variants: {name: fn}; -> {name: [ms per window]} with the variants taking turns inside every window."""
    out = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            out[k].append(timer(fn))
    return out


def count_syncs(fn):
    """host synchronisations of fn() as torch's sync debug mode reports them; None where the mode is not available"""
    try:
        torch.cuda.set_sync_debug_mode('warn')
    except Exception:
        return None
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
        return sum('synchroniz' in str(x.message) for x in w)
    finally:
        torch.cuda.set_sync_debug_mode('default')


def torch_overlap(depth_mm, kinv, pose, base, radius, frame_batch):
    """what a user would write today with this repository's un-projection and plain torch"""
    import mvpnet_amd.ops as ops
    F, h, w = depth_mm.shape
    nb = base.size(0)
    xyz, mask = ops.unproject(depth_mm[None], kinv[None], pose[None])
    xyz, mask = xyz.view(F, h * w, 3), mask.view(F, h * w)
    ok = torch.isfinite(pose).all(-1).all(-1)
    r2 = torch.tensor(radius, dtype=torch.float32, device=base.device) ** 2
    out = torch.zeros((F, nb), dtype=torch.int32, device=base.device)
    for lo in range(0, F, frame_batch):
        hi = min(F, lo + frame_batch)
        d2 = ((xyz[lo:hi, :, None, :] - base[None, None]) ** 2).sum(-1)  # (fb, hw, nb)
        best, j = d2.min(-1)
        hit = (best < r2) & mask[lo:hi] & ok[lo:hi, None]
        out[lo:hi].scatter_add_(1, j, hit.int())
    return (out > 0).t()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1500)
    ap.add_argument('--base', type=int, default=2000)
    ap.add_argument('--chunks', type=int, default=64)
    ap.add_argument('--picks', type=int, default=3)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--torch-frames', type=int, default=96)
    ap.add_argument('--torch-frame-batch', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_scene_prep needs the GPU: nothing here is measured on a CPU')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import _lib as L
    from mvpnet_amd.chunks import scene2chunks_legacy, select_frames, chunk_base_masks
    from mvpnet_amd.scene import prepare_scene
    from mvpnet_amd.synthetic import make_rgbd_scene
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    h, w = 60, 80
    F, nb, C, n = args.frames, args.base, args.chunks, args.picks
    sc = make_rgbd_scene(0, F, n_pts=60000, h=h, w=w)
    pts = t(sc['points'])
    depth, pose = t(sc['depth_mm'].astype(np.int16)), t(sc['pose'])
    kinv = t(np.repeat(sc['kinv'][None], F, 0))
    base_ind = torch.randperm(pts.size(0), generator=torch.Generator(device=dev).manual_seed(1), device=dev)[:nb]
    base = pts[base_ind].contiguous()
    res = {'device': torch.cuda.get_device_name(0), 'frames': F, 'h': h, 'w': w, 'base_points': nb, 'chunks': C, 'picks': n}

    # ---- overlap ------------------------------------------------------------------------------------------------------------
    bits = torch.empty((F, (nb + 31) // 32), dtype=torch.int32, device=dev)
    kernel_all = lambda: L.call('mvp_frame_overlap_u16', depth, L.ptr(depth), L.ptr(kinv), L.ptr(pose), L.ptr(base), F, h, w, nb, 0.1, L.ptr(bits))
    Ft = min(args.torch_frames, F)
    d_s, k_s, p_s = depth[:Ft].contiguous(), kinv[:Ft].contiguous(), pose[:Ft].contiguous()
    bits_s = torch.empty((Ft, (nb + 31) // 32), dtype=torch.int32, device=dev)
    kernel_sub = lambda: L.call('mvp_frame_overlap_u16', d_s, L.ptr(d_s), L.ptr(k_s), L.ptr(p_s), L.ptr(base), Ft, h, w, nb, 0.1, L.ptr(bits_s))
    torch_sub = lambda: torch_overlap(d_s, k_s, p_s, base, 0.1, args.torch_frame_batch)
    for _ in range(3):
        kernel_all(), kernel_sub()
    same = torch.equal(ops.unpack_bits(bits_s, nb).t(), torch_sub())  # also the warm-up of the torch formulation
    tm = alternate({'kernel_all_frames': lambda: device_ms(kernel_all, 20), 'kernel_subset': lambda: device_ms(kernel_sub, 50),
                    'torch_subset': lambda: device_ms(torch_sub, 1)}, args.windows, lambda f: f())
    pairs = F * h * w * nb
    bound_ms = pairs * OPS_PER_PAIR / (FP32_VECTOR_PEAK / 2) * 1e3
    k_all = stats(tm['kernel_all_frames'])
    res['overlap'] = {'kernel_all_frames': k_all, 'subset_frames': Ft, 'kernel_subset': stats(tm['kernel_subset']), 'torch_subset': stats(tm['torch_subset']),
                      'torch_frame_batch': args.torch_frame_batch, 'torch_equals_kernel_on_subset': bool(same),
                      'torch_over_kernel_subset': round(statistics.median(tm['torch_subset']) / statistics.median(tm['kernel_subset']), 1),
                      'bits_set': int(ops.unpack_bits(bits, nb).sum())}
    bytes_moved = depth.numel() * 2 + F * (9 + 16) * 4 + bits.numel() * 4 * 2  # depth, cameras, memset + merged rows; the base points stay in L2
    memory_bound_ms = bytes_moved / HBM_PEAK * 1e3
    res['bound'] = {'pair_evaluations': pairs, 'ops_per_pair': OPS_PER_PAIR, 'nonfused_fp32_peak_ops_per_s': FP32_VECTOR_PEAK / 2, 'valu_bound_ms': round(bound_ms, 4),
                    'bytes_moved': int(bytes_moved), 'memory_bound_ms': round(memory_bound_ms, 5), 'limiting_bound': 'VALU' if bound_ms > memory_bound_ms else 'memory',
                    'share_of_bound': round(max(bound_ms, memory_bound_ms) / k_all['median_ms'], 3)}

    # ---- selection ----------------------------------------------------------------------------------------------------------
    inds, _ = scene2chunks_legacy(pts, (1.5, 1.5), 0.5, thresh=1000, margin=(0.2, 0.2), return_bbox=True)
    take = np.linspace(0, len(inds) - 1, C).round().astype(int)
    masks = chunk_base_masks([inds[i] for i in take], base_ind, pts.size(0))  # (C,nb) bool
    kernel_all()
    ch_bits = ops.pack_bits(masks)
    overlaps = ops.unpack_bits(bits, nb).t().contiguous()  # (nb,F) bool, what the parent commit's select_frames reads
    picked = torch.empty((C, n), dtype=torch.int64, device=dev)
    batched = lambda: L.call('mvp_select_frames_u32', bits, L.ptr(bits), L.ptr(ch_bits), F, C, (nb + 31) // 32, n, L.ptr(picked), None)
    batched_op = lambda: ops.select_frames_batched(overlaps, masks, n)  # from the bool matrices: packing included
    loop = lambda: [select_frames(overlaps[m], n) for m in masks]
    for _ in range(3):
        batched(), batched_op()
    same = loop() == picked.tolist()
    tm = alternate({'kernel': lambda: device_ms(batched, 100), 'op_from_bool': lambda: device_ms(batched_op, 20), 'python_loop': lambda: host_ms(loop)},
                   args.windows, lambda f: f())
    res['select'] = {'kernel': stats(tm['kernel']), 'op_from_bool': stats(tm['op_from_bool']), 'python_loop': stats(tm['python_loop']),
                     'loop_equals_kernel': bool(same), 'host_syncs_batched': count_syncs(batched_op), 'host_syncs_python_loop': count_syncs(loop),
                     'python_loop_over_kernel': round(statistics.median(tm['python_loop']) / statistics.median(tm['kernel']), 1)}

    # ---- pipeline -----------------------------------------------------------------------------------------------------------
    Fp = 96
    scp = make_rgbd_scene(0, Fp, n_pts=60000, h=h, w=w)
    ppts, pdepth, ppose = t(scp['points']), t(scp['depth_mm'].astype(np.int16)), t(scp['pose'])
    images = torch.zeros((Fp, 3, h, w), device=dev)
    prep = lambda: prepare_scene(ppts, pdepth, scp['cam_matrix'], ppose, images, chunk_size=(1.5, 1.5), chunk_stride=0.5, chunk_thresh=1000,
                                 chunk_margin=(0.2, 0.2), num_rgbd_frames=n, k=3, num_base_pts=nb)
    nchunks = len(prep()[1])
    prep()
    res['pipeline'] = dict(stats([host_ms(prep) for _ in range(args.windows)]), frames=Fp, points=60000, chunks=nchunks, what='prepare_scene wall time, host clock around a synchronise')
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

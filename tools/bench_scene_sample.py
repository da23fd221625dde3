"""A 3D-baseline training batch drawn on the GPU (scene.sample_train_batch_3d), measured next to what the tree offered before.
Prints ONE JSON line (and writes it to --out).

    python tools/bench_scene_sample.py [--rows 8] [--points 150000] [--nb-pts 32768] [--windows 9] [--reps 20] [--out FILE] [--profile-only]

The shape is configs/scannet/3d_baselines/pn2ssg_rgb_scene.yaml's: 8 rows of 32768 points with colours, RandomRotateZ; the store holds one
synthetic scene of --points points per row (seeded uniform points, labels and uint8 colours), resident on the device.
Method: everything is warmed up first; the variants ALTERNATE inside the same process, window after window; each window times --reps calls
with device events ((b) synchronises by itself: the host clock around a synchronise, one call); the figure is the median over the windows
and `spread` the (max - min) / median over them.

  (a) batch_3d     scene.sample_train_batch_3d(dataset='ScanNet3DScene', use_color=True, z_rot=(-pi, pi)): the seed draw, ops.sample_scenes,
                   the angle draws, ops.gather_cloud.  `sample` and `gather` time the two ops alone.
  (b) python_loop  what the parent commit offers for the same job: per row chunks.crop_pad_choice (one torch.randperm(n) on the device,
                   n read from the host's offsets), torch gathers of points, labels and colours, `/ 255`, and one bmm with the matrices
                   of augment.draw_z_rotation's law built on the host; its host synchronisations are counted by torch's sync debug mode.
  bound            the gather's traffic: per slot 8 bytes of choice, 12 + 8 + 3 scattered bytes read (each at least one 32-byte sector:
                   3 sectors) and 12 + 8 + 12 bytes written, against HBM.

--profile-only runs (a) alone a few times: the process to put behind `rocprofv3 --kernel-trace --stats --`.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_scene_prep import stats, device_ms, host_ms, alternate, count_syncs  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


def python_loop(store, rows_host, nb_pts, generator):
    """what a user wrote with the parent commit: one row at a time"""
    from mvpnet_amd.chunks import crop_pad_choice
    off = store['scene_offsets_host']
    dev = store['points'].device
    pts, lab, col = [], [], []
    for s in rows_host:
        lo, hi = int(off[s]), int(off[s + 1])
        choice = crop_pad_choice(hi - lo, nb_pts, generator=generator, device=dev) + lo
        pts.append(store['points'][choice])
        lab.append(store['seg_label'][choice])
        col.append(store['colors'][choice])
    angle = np.random.uniform(-math.pi, math.pi, len(rows_host))
    c, s = np.cos(angle), np.sin(angle)
    z, o = np.zeros_like(c), np.ones_like(c)
    rot = torch.from_numpy(np.stack([c, -s, z, s, c, z, z, z, o], -1).reshape(-1, 3, 3).astype(np.float32)).to(dev)
    points = torch.bmm(torch.stack(pts), rot.transpose(1, 2)).transpose(1, 2).contiguous()
    feature = (torch.stack(col).float() / 255.).transpose(1, 2).contiguous()
    return {'points': points, 'seg_label': torch.stack(lab), 'feature': feature}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=8)
    ap.add_argument('--points', type=int, default=150000)
    ap.add_argument('--nb-pts', type=int, default=32768)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile-only', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_scene_sample needs the GPU: nothing here is measured on a CPU')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import augment as A
    from mvpnet_amd import scene as SC
    dev = torch.device('cuda:0')
    B, n, nb_pts = args.rows, args.points, args.nb_pts
    rs = np.random.RandomState(3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    label = rs.randint(0, 20, B * n).astype(np.int64)
    label[rs.rand(B * n) < 0.15] = -100
    off = np.arange(B + 1, dtype=np.int64) * n
    store = dict(points=t((rs.rand(B * n, 3) * np.array([8.0, 6.0, 3.0])).astype(np.float32)), seg_label=t(label),
                 colors=t(rs.randint(0, 256, (B * n, 3)).astype(np.uint8)), scene_offsets=t(off), scene_offsets_host=off)
    rows_host = list(range(B))
    rows = t(np.array(rows_host, np.int64))
    gen = torch.Generator(device=dev).manual_seed(1)
    kw = dict(dataset='ScanNet3DScene', nb_pts=nb_pts, use_color=True, z_rot=(-math.pi, math.pi))
    batch = lambda: SC.sample_train_batch_3d(store, rows, generator=gen, **kw)
    seed = torch.tensor([5], dtype=torch.int64, device=dev)
    sample = lambda: ops.sample_scenes(store['scene_offsets'], rows, nb_pts, seed=seed, Ntot=B * n)
    choice, rot = sample()['choice'], A.draw_z_rotation(B, device=dev, generator=gen)
    gather = lambda: ops.gather_cloud(store['points'], store['scene_offsets'], rows, choice, seg_label=store['seg_label'], colors=store['colors'], rot=rot)
    loop = lambda: python_loop(store, rows_host, nb_pts, gen)
    for _ in range(3):
        batch(), sample(), gather(), loop()
    torch.cuda.synchronize()
    if args.profile_only:
        for _ in range(5):
            batch()
        torch.cuda.synchronize()
        return
    tm = alternate({'batch_3d': lambda: device_ms(batch, args.reps), 'sample': lambda: device_ms(sample, args.reps),
                    'gather': lambda: device_ms(gather, args.reps), 'python_loop': lambda: host_ms(loop)}, args.windows, lambda f: f())
    a, b = stats(tm['batch_3d']), stats(tm['python_loop'])
    res = {'device': torch.cuda.get_device_name(0), 'rows': B, 'points_per_scene': n, 'nb_pts': nb_pts, 'reps_per_window': args.reps,
           'a_batch_3d': dict(a, host_syncs=count_syncs(batch)), 'a_sample_scenes': stats(tm['sample']), 'a_gather_cloud': stats(tm['gather']),
           'b_python_loop': dict(b, host_syncs=count_syncs(loop)), 'b_over_a': round(b['median_ms'] / a['median_ms'], 2)}
    gap = b['median_ms'] - a['median_ms']
    noise = (a['max_ms'] - a['min_ms']) + (b['max_ms'] - b['min_ms'])
    res['a_beats_b_beyond_the_spread'] = bool(gap > noise)
    slots = B * nb_pts
    moved = slots * (8 + 3 * 32 + 32)
    res['bound_gather'] = {'bytes_moved': moved, 'hbm_bound_ms': round(moved / HBM_PEAK * 1e3, 5)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

"""Drawing a training batch on the GPU, measured next to what the tree offered before and to the reference's NumPy loop.
Prints ONE JSON line (and writes it to --out).

    python tools/bench_train_sample.py [--chunks 32] [--points 150000] [--nb-pts 8192] [--tries 10] [--base 2000] [--picks 3]
                                       [--frames 48] [--windows 7] [--out FILE] [--profile-only]

The store: one synthetic scene per chunk (make_rgbd_scene, --points points, --frames frames of 40x30), resident on the device.
Method: everything is warmed up first; the two device variants ALTERNATE inside the same process, window after window; (a) is timed with
device events over several repetitions, (b) with the host clock around a synchronise (it synchronises anyway); the figure is the median
over the windows and `spread` the (max - min) / median over them.

  (a) sample_select  chunks.sample_train_chunks + ops.select_frames_batched with frame ranges: the sampling and selection part of
                     scene.sample_train_batch (`batch`: the whole call, frame gathers included).
  (b) python_loop    what the tree offered before: per chunk a Python loop of torch masks over the scene, `nonzero`,
                     chunks.crop_pad_choice and chunks.select_frames, on the device; its host synchronisations are counted by torch's
                     sync debug mode.
  (c) numpy_loop     the reference's algorithm (scannet_2d3d.py:341-381, :199-220) restated in NumPy on ONE host core, once.
  bound              the counting pass: B * n * 20 bytes read (12 of xyz, 8 of the int64 label) against HBM, and B * n * T box tests
                     of ~10 VALU operations (4 compares, 3 ands, 2 ballots and their counts) against the plain VALU rate.

--profile-only runs (a) alone a few times: the process to put behind `rocprofv3 --kernel-trace --stats --`.
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
from tools.bench_scene_prep import stats, device_ms, host_ms, alternate, count_syncs  # noqa: E402

HBM_PEAK = 8.0e12              # bytes/s
VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9  # plain (non-packed, non-fused) vector operations per second: CUs x SIMDs x lanes x clock
STEP_MS = 6.2                  # the B = 32 training step this loader has to feed (README)


def labels_for(points, seed):
    """seeded labels, 15 % unlabelled, one third of the room 90 % unlabelled (tries fail there)"""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 20, len(points)).astype(np.int64)
    u = rs.rand(len(points))
    lab[np.where(points[:, 0] < 2.2, u < 0.9, u < 0.15)] = -100
    return lab


def torch_loop(store, soc_host, nb_pts, tries, picks, size, margin, thresh, overlaps):
    """what a user wrote with the parent commit: one chunk at a time"""
    from mvpnet_amd.chunks import crop_pad_choice, select_frames
    off, foff = store['scene_offsets_host'], store['frame_offsets_host']
    half = 0.5 * torch.tensor(size, dtype=torch.float32, device=store['points'].device)
    mg = torch.tensor(margin, dtype=torch.float32, device=half.device)
    out = []
    for s in soc_host:
        pts, lab = store['points'][off[s]:off[s + 1]], store['seg_label'][off[s]:off[s + 1]]
        xy = pts[:, :2]
        mask = None
        for _ in range(tries):
            c = xy[int(torch.randint(len(pts), (1,)))]
            lo, hi = (c - half) - mg, (c + half) + mg
            cand = ((xy >= lo) & (xy <= hi)).all(1)
            m = int(cand.sum())
            if m and float((lab[cand] >= 0).float().mean()) >= thresh:
                mask = cand
                break
        if mask is None:
            mask = torch.ones(len(pts), dtype=torch.bool, device=pts.device)
            lo, hi = xy.min(0).values - mg, xy.max(0).values + mg
        idx = mask.nonzero()[:, 0]
        choice = idx[crop_pad_choice(idx.numel(), nb_pts, device=pts.device)]
        base_in = mask[store['base_point_ind'][s]]
        frames = select_frames(overlaps[s][base_in], picks)
        out.append((pts[choice].t(), lab[choice], torch.cat([lo, hi]), [int(foff[s]) + f for f in frames]))
    return out


def numpy_loop(host, soc_host, nb_pts, tries, picks, size, margin, thresh):
    """the reference's loader work for one batch, on one core"""
    size, margin = np.array(size, np.float32), np.array(margin, np.float32)
    for s in soc_host:
        pts, lab = host['points'][s], host['labels'][s]
        xy = pts[:, :2]
        mask = None
        for _ in range(tries):
            c = xy[np.random.randint(len(pts))]
            cand = np.all(np.logical_and(xy >= (c - 0.5 * size) - margin, xy <= (c + 0.5 * size) + margin), axis=1)
            if cand.any() and np.mean(lab[cand] >= 0) >= thresh:
                mask = cand
                break
        if mask is None:
            mask = np.ones(len(pts), bool)
        m = int(mask.sum())
        choice = np.hstack([np.arange(m), np.random.randint(m, size=nb_pts - m)]) if m < nb_pts else np.random.choice(m, nb_pts, replace=False)
        _ = pts[mask][choice], lab[mask][choice]
        left = host['overlaps'][s][mask[host['base'][s]]].copy()
        for _ in range(picks):
            f = left.sum(0).argmax()
            left[left[:, f]] = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chunks', type=int, default=32)
    ap.add_argument('--points', type=int, default=150000)
    ap.add_argument('--nb-pts', type=int, default=8192)
    ap.add_argument('--tries', type=int, default=10)
    ap.add_argument('--base', type=int, default=2000)
    ap.add_argument('--picks', type=int, default=3)
    ap.add_argument('--frames', type=int, default=48)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile-only', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_sample needs the GPU: nothing here is measured on a CPU')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import chunks as CH
    from mvpnet_amd import scene as SC
    from mvpnet_amd.synthetic import make_rgbd_scene
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, n, nb_pts, T, nbp, nv, F = args.chunks, args.points, args.nb_pts, args.tries, args.base, args.picks, args.frames
    h, w = 30, 40
    size, margin, thresh = (1.5, 1.5), (0.2, 0.2), 0.3
    rs = np.random.RandomState(3)
    host = dict(points=[], labels=[], base=[], overlaps=[])
    depth, pose, bits, cam, kinv = [], [], [], [], []
    for s in range(B):
        sc = make_rgbd_scene(100 + s, F, n_pts=n, h=h, w=w)
        base = rs.choice(n, nbp, replace=False).astype(np.int64)
        d, p = t(sc['depth_mm'].astype(np.int16)), t(sc['pose'])
        b = ops.rgbd_overlap(d, t(np.repeat(sc['kinv'][None], F, 0)), p, t(sc['points'][base]), packed=True)
        host['points'].append(sc['points'])
        host['labels'].append(labels_for(sc['points'], s))
        host['base'].append(base)
        host['overlaps'].append(ops.unpack_bits(b, nbp).t().cpu().numpy())
        depth.append(d), pose.append(p), bits.append(b), cam.append(sc['cam_matrix'][:3, :3]), kinv.append(sc['kinv'])
    off = np.arange(B + 1, dtype=np.int64) * n
    foff = np.arange(B + 1, dtype=np.int64) * F
    store = dict(points=t(np.concatenate(host['points'])), seg_label=t(np.concatenate(host['labels'])), scene_offsets=t(off),
                 base_point_ind=t(np.stack(host['base'])), overlap_bits=torch.cat(bits), frame_offsets=t(foff), depth=torch.cat(depth),
                 pose=torch.cat(pose), images=torch.zeros((B * F, 3, h, w), device=dev), cam=t(np.stack(cam)), kinv=t(np.stack(kinv)),
                 scene_offsets_host=off, frame_offsets_host=foff)
    soc_host = list(range(B))
    soc = t(np.array(soc_host, np.int64))
    gen = torch.Generator(device=dev).manual_seed(1)
    kw = dict(chunk_size=size, chunk_margin=margin, chunk_thresh=thresh, num_tries=T)
    begin, count = store['frame_offsets'][soc], store['frame_offsets'][soc + 1] - store['frame_offsets'][soc]

    def sample_select():
        ch = CH.sample_train_chunks(store['points'], store['seg_label'], store['scene_offsets'], soc, nb_pts, base_point_ind=store['base_point_ind'],
                                    generator=gen, **kw)
        ch['picked'] = ops.select_frames_batched(store['overlap_bits'], ch['base_bits'], nv, frame_begin=begin, frame_count=count)
        return ch
    batch = lambda: SC.sample_train_batch(store, soc, nb_pts=nb_pts, num_rgbd_frames=nv, k=3, generator=gen, **kw)
    for _ in range(3):
        ch = sample_select()
        batch()
    torch.cuda.synchronize()
    if args.profile_only:
        for _ in range(5):
            sample_select()
        torch.cuda.synchronize()
        return
    res = {'device': torch.cuda.get_device_name(0), 'chunks': B, 'points_per_scene': n, 'nb_pts': nb_pts, 'tries': T, 'base_points': nbp,
           'picks': nv, 'frames_per_scene': F,
           'last_draw': {'fallbacks': int((ch['try_index'] < 0).sum()), 'later_try': int((ch['try_index'] > 0).sum()),
                         'pads': int((ch['num_members'] < nb_pts).sum()), 'median_members': int(ch['num_members'].median())}}
    overlaps_dev = [t(o) for o in host['overlaps']]
    loop = lambda: torch_loop(store, soc_host, nb_pts, T, nv, size, margin, thresh, overlaps_dev)
    loop()
    tm = alternate({'sample_select': lambda: device_ms(sample_select, 20), 'batch': lambda: device_ms(batch, 20),
                    'python_loop': lambda: host_ms(loop)}, args.windows, lambda f: f())
    a, b = stats(tm['sample_select']), stats(tm['python_loop'])
    res['a_sample_select'] = dict(a, host_syncs=count_syncs(sample_select), share_of_step=round(a['median_ms'] / STEP_MS, 4), step_ms=STEP_MS)
    res['a_whole_batch'] = stats(tm['batch'])
    res['b_python_loop'] = dict(b, host_syncs=count_syncs(loop))
    gap = b['median_ms'] - a['median_ms']
    noise = (a['max_ms'] - a['min_ms']) + (b['max_ms'] - b['min_ms'])
    res['b_over_a'] = round(b['median_ms'] / a['median_ms'], 1)
    res['a_beats_b_beyond_the_spread'] = bool(gap > noise)
    np.random.seed(0)
    t0 = time.perf_counter()
    numpy_loop(host, soc_host, nb_pts, T, nv, size, margin, thresh)
    res['c_numpy_loop_one_core_once_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
    read = B * n * 20
    res['bound_counting_pass'] = {'bytes_read': read, 'hbm_bound_ms': round(read / HBM_PEAK * 1e3, 5), 'box_tests': B * n * T,
                                  'valu_ops_per_test': 10, 'valu_bound_ms': round(B * n * T * 10 / VALU_LANE_OPS * 1e3, 5)}
    res['bound_counting_pass']['limiting_bound'] = 'VALU' if res['bound_counting_pass']['valu_bound_ms'] > res['bound_counting_pass']['hbm_bound_ms'] else 'HBM'
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

"""What the meters of a training iteration cost (mvp_seg_loss_meter_f32 against the three launches and the read-back they replace).

  part 1  the launches alone at (32, 20, 8192), channels-last rows, HIP events around a device-bound loop of library calls:
            loss            mvp_seg_loss_f32
            loss+2conf      + two mvp_seg_confusion_f32 (SegAccuracy's and SegIoU's)
            loss+2conf+read + the `.tolist()` of SegAccuracy.update_dict: a host synchronisation per iteration
            fused           ONE mvp_seg_loss_meter_f32
            meters-only     the same launch without a loss (DeviceMeters.update_dict)
  part 2  mvpnet3d.train_step on the bench's model and shapes at B = 4 and B = 32 with the iteration's meters
            old way         SegAccuracy.update_dict + SegIoU.update_dict after the step
            on loss_fn      SegLoss(meters=DeviceMeters)
            none            no meters

One process.  Every step runs under a time limit of its own (a watchdog thread ends the process when a step overruns, also while the
main thread waits in a device synchronise); variants alternate inside a step, each figure is the median over the repeats with the
min .. max spread beside it.  usage: python tools/exp/seg_meter_time.py [--out profiles/seg_meter.txt] [--skip-step]"""
import argparse
import faulthandler
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mvpnet_amd import _lib as L  # noqa: E402
from mvpnet_amd import metric as M  # noqa: E402
from mvpnet_amd.mvpnet3d import MVPNet3D, SegLoss, prefetch_geometry, train_step  # noqa: E402

DEV = torch.device('cuda:0')
LINES = []


def say(text=''):
    print(text, flush=True)
    LINES.append(text)


class limit:
    """`with limit(seconds):` -- the step's own time limit"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def alternate(variants, n, repeats, warmup):
    """variants: [(name, fn)] -> {name: [us per call, one per repeat]}, the variants taking turns inside every repeat"""
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            out[name].append(window_us(fn, n))
    return out


def report(title, times, unit='us', scale=1.0):
    say(title)
    for name, v in times.items():
        v = np.asarray(v) * scale
        say('  {:<18s} median {:9.2f} {}   min {:9.2f}   max {:9.2f}   ({} repeats)'.format(name, np.median(v), unit, v.min(), v.max(), len(v)))


def launches():
    B, C, N, W = 32, 20, 8192, 20
    g = torch.Generator(device=DEV).manual_seed(1)
    logit = (torch.randn(B, N, C, device=DEV, generator=g) * 3).transpose(1, 2)
    label = torch.randint(0, C, (B, N), device=DEV, generator=g)
    label[torch.rand(B, N, device=DEV, generator=g) < 0.1] = -100
    weight = torch.rand(C, device=DEV, generator=g) + 0.5
    acc, loss = torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros((), device=DEV)
    mat1, mat2 = (torch.zeros(C, C, dtype=torch.int64, device=DEV) for _ in range(2))
    ni, nf = M.meter_state_sizes(C, W)
    si, sf = torch.zeros(ni, dtype=torch.int64, device=DEV), torch.zeros(nf, dtype=torch.float64, device=DEV)
    sb, sc, sn = logit.stride()
    head = (L.ptr(logit), B, C, N, sb, sc, sn, L.ptr(label))

    def old_loss():  # (timing only: acc is not re-zeroed, so only the first launch's last workgroup writes the loss -- one 4-byte store)
        L.call('mvp_seg_loss_f32', logit, *head, L.ptr(weight), -100, L.ptr(acc), L.ptr(loss))

    def old_conf():
        old_loss()
        L.call('mvp_seg_confusion_f32', logit, *head, -100, L.ptr(mat1))
        L.call('mvp_seg_confusion_f32', logit, *head, -100, L.ptr(mat2))

    def old_read():
        old_conf()
        torch.stack([mat1.diagonal().sum(), mat1.sum()]).tolist()

    def fused():
        L.call('mvp_seg_loss_meter_f32', logit, *head, L.ptr(weight), -100, L.ptr(acc), L.ptr(loss), L.ptr(si), L.ptr(sf), W)

    def meters_only():
        L.call('mvp_seg_loss_meter_f32', logit, *head, None, -100, None, None, L.ptr(si), L.ptr(sf), W)

    times = alternate([('loss', old_loss), ('loss+2conf', old_conf), ('loss+2conf+read', old_read), ('fused', fused), ('meters-only', meters_only)],
                      n=200, repeats=9, warmup=20)
    report('launches at ({}, {}, {}) rows, us per iteration (HIP events, 200 iterations per window)'.format(B, C, N), times)
    return times


class Supplied2D(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.feature = None

    def forward(self, data):
        return {'feature': self.feature}


def bench_batch(B):
    from mvpnet_amd.synthetic import make_batch
    uniq = min(B, 8)
    bt = make_batch(1000, uniq, config=3)
    rep = (B + uniq - 1) // uniq
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate([a] * rep)[:B])).to(DEV)
    nv = bt['depth_mm'].shape[1]
    cam = np.repeat(bt['cam_matrix'][None, None, :3, :3], nv, 1).repeat(uniq, 0)
    batch = {'images': torch.zeros(B, nv, 3, 120, 160, device=DEV), 'points': t(bt['points'].transpose(0, 2, 1)), 'seg_label': t(bt['seg_label']),
             'depth': t(bt['depth_mm'].astype(np.int16)), 'cam_matrix': t(cam), 'kinv': t(bt['kinv']), 'pose': t(bt['pose']),
             'pixel_box': t(bt['pixel_box']), 'k': 3}
    return batch, t(bt['feature_2d']).view(B * nv, 120, 160, 64).permute(0, 3, 1, 2)


def steps(B, n, repeats):
    from mvpnet_amd.pn2 import PN2SSG
    from mvpnet_amd.optim import FusedAdam
    torch.manual_seed(0)
    batch, feature = bench_batch(B)
    net2d = Supplied2D()
    net2d.feature = feature
    model = MVPNet3D(net2d, '', PN2SSG(64, 20), in_channels=64).to(DEV).train()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    weight = torch.linspace(0.5, 1.5, 20, device=DEV)
    plain, metered = SegLoss(weight=weight), SegLoss(weight=weight, meters=M.DeviceMeters(20))
    acc, iou = M.SegAccuracy(), M.SegIoU(20)
    state = {'cur': prefetch_geometry(model, dict(batch))}

    def step(loss_fn, old_meters):
        nxt = dict(batch)
        _, preds = train_step(model, loss_fn, opt, state['cur'], next_batch=nxt)
        if old_meters:
            with torch.no_grad():
                acc.update_dict(preds, state['cur'])
                iou.update_dict(preds, state['cur'])
        state['cur'] = nxt

    times = alternate([('none', lambda: step(plain, False)), ('on loss_fn', lambda: step(metered, False)), ('old way', lambda: step(plain, True))],
                      n=n, repeats=repeats, warmup=5)
    report('train_step at B = {}, ms per step (HIP events, {} steps per window)'.format(B, n), times, unit='ms', scale=1e-3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    say('{}; {}'.format(torch.cuda.get_device_name(0), L.lib().mvp_version().decode()))
    with limit(120):
        t = launches()
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = float(np.max(t['loss']) - np.min(t['loss']))
    say('  fused - loss = {:+.2f} us (spread of the loss launch: {:.2f} us)'.format(med['fused'] - med['loss'], spread))
    if not args.skip_step:
        for B, n in ((4, 40), (32, 20)):
            with limit(240):
                t = steps(B, n, repeats=7)
            med = {k: float(np.median(v)) * 1e-3 for k, v in t.items()}
            spread = float(np.max(t['none']) - np.min(t['none'])) * 1e-3
            say('  on loss_fn - none = {:+.3f} ms, old way - none = {:+.3f} ms (spread of the step without meters: {:.3f} ms)'.format(
                med['on loss_fn'] - med['none'], med['old way'] - med['none'], spread))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()

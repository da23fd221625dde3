"""What the eager solver tail costs a replayed training step: mvpnet3d.GraphedTrainStep(solver='eager') -- the plain FusedAdam and torch's
MultiStepLR issued from Python behind every replay -- against solver='captured' -- FusedAdam(capturable=True) and DeviceMultiStepLR as
nodes of the graph -- on the benchmark's configs[2] model and batch (bench.py's builders), one GPU, at B chunks per GPU.

Per mode and B:  host ms per step() call (time.perf_counter around the call alone, the stream drained before each call, median of
--steps calls) and step ms to completion (HIP events around blocks of 20 back-to-back steps, median block / 20; the same blocks by
perf_counter with a synchronize).  Every step copies the batch into the static inputs, as bench.py --graph does.  Warm-up: 10 steps
after the capture.  The modes are measured in turn, eager first, each on a fresh model and optimizer with the learning rate at 0 as in
bench.py (the launches do not depend on it).

    python tools/exp/solver_tail_time.py --batches 4 32 --out profiles/solver_captured.txt"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch
import yaml


def measure(B, solver, steps, dev):
    import bench
    from mvpnet_amd import config as C
    from mvpnet_amd.mvpnet3d import GraphedTrainStep, SegLoss
    with open(os.path.join(ROOT, 'tests', 'golden', 'configs.json')) as f:
        cfg = C.load_cfg(text=yaml.safe_dump(json.load(f)['mvpnet_3d_unet_resnet34_pn2ssg']))
    batch, feature, _ = bench.build_batch(0, B, dev)
    torch.manual_seed(0)
    net2d = bench.SuppliedFeature2D()
    net2d.feature = feature
    model = C.build_model_mvpnet_3d(cfg, net2d, load_2d_ckpt=False).to(dev).train()
    loss_fn = SegLoss(weight=torch.linspace(0.5, 1.5, 20, device=dev))
    cfg.OPTIMIZER.BASE_LR = 0.0
    captured = solver == 'captured'
    optimizer = C.build_optimizer(cfg, model, capturable=captured)
    scheduler = C.build_scheduler(cfg, optimizer, capturable=captured)
    step = GraphedTrainStep(model, loss_fn, optimizer, dict(batch), dict(batch), scheduler=scheduler, solver=solver)
    for _ in range(10):
        step.step(batch, batch)
    torch.cuda.synchronize(dev)
    host = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step.step(batch, batch)
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize(dev)
    event_ms, wall_ms = [], []
    for _ in range(7):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        start.record()
        for _ in range(20):
            step.step(batch, batch)
        stop.record()
        torch.cuda.synchronize(dev)
        wall_ms.append((time.perf_counter() - t0) * 1e3 / 20)
        event_ms.append(start.elapsed_time(stop) / 20)
    count = float(optimizer.state[next(p for p in model.parameters() if p.grad is not None)]['step'])
    return {'B': B, 'solver': solver, 'optimizer': type(optimizer).__name__ + ('(capturable)' if captured else ''),
            'scheduler': type(scheduler).__name__, 'host_ms_per_call_median': statistics.median(host), 'host_ms_per_call_min': min(host),
            'step_ms_events_median': statistics.median(event_ms), 'step_ms_events_min': min(event_ms), 'step_ms_events_max': max(event_ms),
            'step_ms_wall_median': statistics.median(wall_ms), 'updates_counted': count}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[4, 32])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = ['# tools/exp/solver_tail_time.py on {} (torch {}): GraphedTrainStep, configs[2] model, one GPU'.format(
        torch.cuda.get_device_name(0), torch.__version__)]
    for B in args.batches:
        for solver in ('eager', 'captured'):
            r = measure(B, solver, args.steps, dev)
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

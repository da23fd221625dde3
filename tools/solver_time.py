"""Times the end of a stage-one training iteration on the parameter shapes of UNetResNet34(num_classes=20): the optimizer step and the
gradient clip of mvpnet_amd.optim (csrc/solver.hip) against torch's.

    python tools/solver_time.py [--reps 100] [--warmup 20] [--out FILE.json]

(a) one step: optim.FusedSGD  vs  torch.optim.SGD as torch builds it by default (foreach on the GPU: what config.build_optimizer returned
    before FusedSGD existed)  vs  torch.optim.SGD(fused=True) where the installed torch has it;
(b) clip + step: optim.clip_grad_norm_ + FusedSGD.step()  and  optim.total_grad_norm + FusedSGD.step(grad_scale=)  vs
    nn.utils.clip_grad_norm_ + the default torch.optim.SGD step; and the two clips alone.
Every variant owns a copy of the parameters and of one set of seeded gradients (84 MB each: the variants are run ROUND-ROBIN, so each
starts with cold caches like a step after a backward pass would).  One repetition = HIP events around the calls on the current stream,
host work included (the stream is idle when a repetition starts: a host-bound path shows as such); the median over the repetitions is
reported, the torch default twice (`torch` and `torch_again`): their difference is the spread a real difference has to exceed.
Bytes are those the rule must move: 20 B per element for the step (p, buffer read and written, gradient read), 12 B for the in-place
clip (gradient read twice, written once), 4 B for the norm alone.  Prints one JSON document; needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from mvpnet_amd import optim  # noqa: E402
from mvpnet_amd.unet_resnet34 import UNetResNet34  # noqa: E402

KW = dict(lr=0.005, momentum=0.9, dampening=0.0, weight_decay=1e-4)  # configs/scannet/unet_resnet34.yaml over the defaults
MAX_NORM = 1.0  # far below the norm of the random gradients: the clip scales


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('solver_time.py measures on the GPU; none found')
    if args.reps < 50:
        raise SystemExit('--reps must be at least 50')
    dev = torch.device('cuda:0')
    shapes = [tuple(p.shape) for p in UNetResNet34(num_classes=20).parameters()]
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(1)
    values = [torch.randn(s, generator=gen, device=dev) * 0.05 for s in shapes]
    grads = [torch.randn(s, generator=gen, device=dev) for s in shapes]

    def fresh():
        ps = [nn.Parameter(v.clone()) for v in values]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps

    def restore(ps):  # (outside the timed window: the in-place clips shrink the gradients every repetition)
        torch._foreach_copy_([p.grad for p in ps], grads)

    variants = {}

    def add(name, make_opt, body, nbytes, resets=False):
        ps = fresh()
        opt = make_opt(ps) if make_opt is not None else None
        variants[name] = {'run': (lambda: body(ps, opt)), 'bytes': nbytes, 'reset': (lambda: restore(ps)) if resets else None, 'ms': []}

    step = lambda ps, opt: opt.step()
    torch_sgd = lambda ps: torch.optim.SGD(ps, **KW)
    add('step/fused_sgd', lambda ps: optim.FusedSGD(ps, **KW), step, 20 * numel)
    add('step/torch', torch_sgd, step, 20 * numel)
    add('step/torch_again', torch_sgd, step, 20 * numel)
    try:
        add('step/torch_fused', lambda ps: torch.optim.SGD(ps, fused=True, **KW), step, 20 * numel)
        variants['step/torch_fused']['run']()
    except (RuntimeError, TypeError, ValueError) as e:  # an older torch
        variants.pop('step/torch_fused', None)
        print('torch.optim.SGD(fused=True) is not available here:', e, file=sys.stderr)

    def ours_clip_step(ps, opt):
        optim.clip_grad_norm_(ps, MAX_NORM)
        opt.step()

    def ours_deferred(ps, opt):
        _, coef = optim.total_grad_norm(ps, MAX_NORM)
        opt.step(grad_scale=coef)

    def torch_clip_step(ps, opt):
        nn.utils.clip_grad_norm_(ps, MAX_NORM)
        opt.step()

    add('clip_step/ours_in_place', lambda ps: optim.FusedSGD(ps, **KW), ours_clip_step, 32 * numel, resets=True)
    add('clip_step/ours_deferred', lambda ps: optim.FusedSGD(ps, **KW), ours_deferred, 24 * numel)
    add('clip_step/torch', torch_sgd, torch_clip_step, 32 * numel, resets=True)
    add('clip_step/torch_again', torch_sgd, torch_clip_step, 32 * numel, resets=True)
    add('clip/ours', None, lambda ps, opt: optim.clip_grad_norm_(ps, MAX_NORM), 12 * numel, resets=True)
    add('clip/torch', None, lambda ps, opt: nn.utils.clip_grad_norm_(ps, MAX_NORM), 12 * numel, resets=True)
    add('clip/torch_again', None, lambda ps, opt: nn.utils.clip_grad_norm_(ps, MAX_NORM), 12 * numel, resets=True)
    add('norm/ours', None, lambda ps, opt: optim.total_grad_norm(ps, MAX_NORM), 4 * numel)

    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(args.warmup + args.reps):
        for v in variants.values():  # round-robin: A/B in one process, every variant on cold caches
            if v['reset'] is not None:
                v['reset']()
            torch.cuda.synchronize()
            begin.record()
            v['run']()
            end.record()
            end.synchronize()
            if it >= args.warmup:
                v['ms'].append(begin.elapsed_time(end))
    out = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'tensors': len(shapes), 'parameters': numel,
           'reps': args.reps, 'warmup': args.warmup, 'variants': {}}
    for name, v in variants.items():
        ms = sorted(v['ms'])
        med = statistics.median(ms)
        out['variants'][name] = {'median_us': round(med * 1e3, 2), 'min_us': round(ms[0] * 1e3, 2), 'p90_us': round(ms[int(0.9 * len(ms))] * 1e3, 2),
                                 'bytes': v['bytes'], 'tb_per_s': round(v['bytes'] / (med * 1e-3) / 1e12, 3)}
    for group in ('step', 'clip_step', 'clip'):
        a, b = out['variants'][group + '/torch']['median_us'], out['variants'][group + '/torch_again']['median_us']
        out['variants'][group + '/torch']['spread_us'] = round(abs(a - b), 2)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

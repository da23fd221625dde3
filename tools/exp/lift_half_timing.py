"""ops.lift on a bfloat16 feature map against the path it replaces, at the headline shape (B = 32, nv = 3, 120x160, C = 64, N = 8192, k = 3),
in one process, alternating, between HIP events:
  (a) feat_bf16.float() followed by ops.lift on the result   (what UNetResNet34.frozen_inference(compute_dtype=bfloat16) + MVPNet3D did)
  (b) ops.lift(feat_bf16)                                    (the rows widened inside the gather)
and the half lift alone against the float32 lift alone (c: ops.lift on a float32 map that exists already).
Prints one line per repeat and a summary; checks once that (a) and (b) give the same bits.  Needs the MI355X.
usage: python tools/exp/lift_half_timing.py [--calls 50] [--repeats 5] [--dtype bfloat16|float16]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
import mvpnet_amd.ops as ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dtype', default='bfloat16', choices=['bfloat16', 'float16'])
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    B = 32
    batch, feature, _ = bench.build_batch(0, B, dev)
    nv, h, w, C = 3, 120, 160, 64
    half = feature.permute(0, 2, 3, 1).contiguous().view(B, nv, h, w, C).to(getattr(torch, args.dtype))
    wide = half.float()  # (c) reads a float32 map that is already there
    pts = batch['points'].transpose(1, 2).contiguous()
    geo = (batch['depth'], batch['kinv'], batch['cam_matrix'], batch['pose'], pts)
    kw = dict(k=3, box=batch['pixel_box'])

    paths = {'a_float_then_lift': lambda: ops.lift(half.float(), *geo, **kw), 'b_lift_half': lambda: ops.lift(half, *geo, **kw),
             'c_lift_float32_alone': lambda: ops.lift(wide, *geo, **kw)}
    with torch.no_grad():
        ra, rb = paths['a_float_then_lift'](), paths['b_lift_half']()
        same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                   for x, y in zip(ra, rb))
        del ra, rb
        for fn in paths.values():  # warm-up of every path
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        rows = {name: [] for name in paths}
        for r in range(args.repeats):
            for name, fn in paths.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(args.calls):
                    fn()
                e.record()
                torch.cuda.synchronize()
                rows[name].append(s.elapsed_time(e) * 1e3 / args.calls)
            print('repeat %d: ' % r + ', '.join('%s %.1f us' % (name, rows[name][-1]) for name in paths), flush=True)
    out = {'shape': dict(B=B, nv=nv, h=h, w=w, C=C, N=pts.size(1), k=3), 'dtype': args.dtype, 'calls': args.calls, 'bit_equal': bool(same),
           'us_per_call': {name: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v)) for name, v in rows.items()},
           'device': torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()

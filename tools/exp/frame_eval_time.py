"""ops.frame_confusion and ops.label_histogram against the two-launch compositions they replace, on the YAML's validation shape
(configs/scannet/unet_resnet34.yaml): VAL.BATCH_SIZE = 32 frames, labels 968 x 1296 -> 120 x 160 through the label mapping, C = 20, logits
contiguous and channels-last.  HIP events around `--reps` calls after a warm-up, the versions alternating over `--rounds` rounds; per
version the median over the rounds and their min .. max (the run-to-run spread of this script).  Results are compared before timing.

    python tools/exp/frame_eval_time.py [--out profiles/frame_eval.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mvpnet_amd import metric, ops  # noqa: E402

DEV = torch.device('cuda:0')
NF, C, FTOT, H, W, SIZE = 32, 20, 40, 968, 1296, (160, 120)


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def compare(title, versions, reps, rounds, lines):
    times = {name: [] for name, _ in versions}
    for _ in range(rounds):
        for name, fn in versions:
            times[name].append(timed(fn, reps))
    lines.append(title)
    for name, _ in versions:
        v = times[name]
        lines.append('  %-46s %8.1f us   (%.1f .. %.1f over %d rounds)' % (name, statistics.median(v), min(v), max(v), rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    g = torch.Generator(device=DEV).manual_seed(1)
    labels = torch.from_numpy(np.random.RandomState(1).randint(0, 48, (FTOT, H, W)).astype(np.uint16)).to(DEV)
    mapping = torch.full((41,), -100, dtype=torch.int64, device=DEV)
    mapping[torch.tensor(metric.EVAL_CLASS_IDS, device=DEV)] = torch.arange(20, device=DEV)
    picked = torch.randperm(FTOT, generator=g, device=DEV)[:NF]
    nchw = torch.randn((NF, C, SIZE[1], SIZE[0]), generator=g, device=DEV)
    lines = ['%s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__),
             '%d frames, labels %d x %d -> %d x %d, C = %d; %d calls per timing' % (NF, H, W, SIZE[1], SIZE[0], C, args.reps)]
    for layout, logit in (('NCHW', nchw), ('channels-last', nchw.contiguous(memory_format=torch.channels_last))):
        mat = torch.zeros((C, C), dtype=torch.int64, device=DEV)

        def fused():
            ops.frame_confusion(logit, labels, picked, size=SIZE, mapping=mapping, out=mat)

        def two_launches():
            metric.confusion_matrix(logit, ops.prepare_labels(labels, picked, size=SIZE, mapping=mapping), out=mat)

        one = ops.frame_confusion(logit, labels, picked, size=SIZE, mapping=mapping)
        assert torch.equal(one, metric.confusion_matrix(logit, ops.prepare_labels(labels, picked, size=SIZE, mapping=mapping))) and int(one.sum()) > 0
        compare('confusion matrix, %s logits' % layout, [('ops.frame_confusion', fused), ('ops.prepare_labels + metric.confusion_matrix', two_launches)],
                args.reps, args.rounds, lines)
    hist = torch.zeros((C,), dtype=torch.int64, device=DEV)

    def fused_hist():
        ops.label_histogram(labels, C, picked=picked, size=SIZE, mapping=mapping, out=hist)

    def bincount():
        lab = ops.prepare_labels(labels, picked, size=SIZE, mapping=mapping)
        return torch.bincount(lab[lab != -100], minlength=C)

    assert torch.equal(ops.label_histogram(labels, C, picked=picked, size=SIZE, mapping=mapping), bincount())
    compare('label histogram, 20 bins (torch.bincount and the mask before it synchronise)',
            [('ops.label_histogram', fused_hist), ('ops.prepare_labels + torch.bincount', bincount)], args.reps, args.rounds, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()

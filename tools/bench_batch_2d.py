"""One batch of the 2D stage on the GPU (scene.sample_train_batch_2d) from stores of different frame sizes, and its pieces alone.  Prints
ONE JSON line (and writes it to --out).

    python tools/bench_batch_2d.py [--batch 32] [--frames 256] [--windows 7] [--out FILE] [--profile-only]

The stores: --frames synthetic frames (seeded bytes, raw ids below 1358) of 640x480, 160x120 and 1296x968 (a quarter of --frames), resident
on the device; every call makes a batch of --batch frames drawn once, resized to the YAML's (160, 120), with the YAML's jitter, flip and
normaliser and a label mapping.  Method: everything is warmed up first; the variants of one store ALTERNATE inside the same process,
window after window, each timed with device events over 20 calls per window; the figure is the median over the windows and `spread` the
(max - min) / median over them.  A record, not a comparison: nothing in the tree made such a batch before.

  batch       scene.sample_train_batch_2d: the draws, ops.resize_frames (none at 160x120), ops.prepare_frames, ops.prepare_labels
  resize      ops.resize_frames alone (one launch; at 160x120 the plain gather)
  frames      ops.prepare_frames on the resized frames alone (a memset and two launches)
  labels      ops.prepare_labels alone (one launch)
  bytes       what the batch moves at least: the picked frames read once by the resize, its uint8 result written and read twice, the floats
              written; the label rows that are read (whole: the pixels read in a row lie closer than a 32-byte sector) and the int64 labels.

--profile-only runs `batch` of the 640x480 store alone a few times: the process to put behind `rocprofv3 --kernel-trace --stats --`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_scene_prep import stats, device_ms, alternate, count_syncs  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
NORMALIZER = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
SIZE = (160, 120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile-only', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_batch_2d needs the GPU: nothing here is measured on a CPU')
    import mvpnet_amd.ops as ops
    from mvpnet_amd import augment as A
    from mvpnet_amd import scene as SC
    dev = torch.device('cuda:0')
    B = args.batch
    gen = torch.Generator(device=dev).manual_seed(1)
    mapping = torch.randint(0, 20, (1358,), generator=gen, device=dev)
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'resize': list(SIZE), 'stores': {}}
    for name, (H, W), F in (('640x480', (480, 640), args.frames), ('160x120', (120, 160), args.frames), ('1296x968', (968, 1296), max(args.frames // 4, 1))):
        store = {'images': torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, generator=gen, device=dev),
                 'labels': torch.randint(0, 1358, (F, H, W), dtype=torch.int16, generator=gen, device=dev).view(torch.uint16)}
        picked = A.draw_frames(B, F, dev, generator=gen)
        kw = dict(resize=SIZE, color_jitter=(0.4, 0.4, 0.4), image_normalizer=NORMALIZER, flip=0.5, label_mapping=mapping, generator=gen)
        small = ops.resize_frames(store['images'], picked, SIZE)
        rows = torch.arange(B, device=dev)
        factor, order = A.draw_color_jitter(B, (0.4, 0.4, 0.4), dev, generator=gen)
        flip = A.draw_flip(B, 0.5, dev, generator=gen)
        variants = {'batch': lambda: SC.sample_train_batch_2d(store, picked, **kw),
                    'resize': lambda: ops.resize_frames(store['images'], picked, SIZE),
                    'frames': lambda: ops.prepare_frames(small, rows, factor=factor, order=order, flip=flip, normalizer=NORMALIZER),
                    'labels': lambda: ops.prepare_labels(store['labels'], picked, SIZE, flip=flip, mapping=mapping)}
        for _ in range(3):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        if args.profile_only:
            if name == '640x480':
                for _ in range(5):
                    variants['batch']()
                torch.cuda.synchronize()
                return
            continue
        tm = alternate(variants, args.windows, lambda f: device_ms(f, 20))
        out_px = SIZE[0] * SIZE[1]
        resized = (H, W) != (SIZE[1], SIZE[0])
        label_read = SIZE[1] * W * 2  # (the rows that are read, whole: the pixels read in a row lie closer than a 32-byte sector)
        moved = B * ((H * W * 3 + out_px * 3 if resized else 0) + out_px * 3 * 2 + out_px * 12 + label_read + out_px * 8)
        res['stores'][name] = dict({k: stats(v) for k, v in tm.items()}, store_frames=F, host_syncs_batch=count_syncs(variants['batch']),
                                   bytes_moved=moved, hbm_bound_ms=round(moved / HBM_PEAK * 1e3, 5))
        del store, small
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

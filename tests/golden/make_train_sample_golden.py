"""Writes tests/golden/train_sample.npz: what the REFERENCE's training loaders do on the fixture scene, draw by draw.

    python -m tests.golden.make_train_sample_golden /path/to/the/reference/checkout

`ScanNet2D3DChunks.__getitem__` (mvpnet/data/scannet_2d3d.py:323-416, num_rgbd_frames = 0) and `ScanNet3DChunks.__getitem__`
(mvpnet/data/scannet_3d.py:135-189, float64 chunk_size / chunk_margin) run unmodified on objects made with `object.__new__` (their
constructors read ScanNet's files) over tests/train_sample_oracle's fixture cloud and seeded labels.  `np.random.randint` /
`np.random.choice` are wrapped to record the draws, a profile hook reads the locals of `__getitem__` when it returns (`flag`, `chunk_min`,
`chunk_max`, `chunk_mask`), and modules the loaders import but these paths never call (natsort, open3d, torchvision) are stubbed when they
are not installed.  Per draw the file keeps the centres tried, the try index (-1 = the whole-scene fallback), the box
`hstack([chunk_min - margin, chunk_max + margin])` of :393 (NaN where the reference defines none: the 3D class's fallback), the number
of members and the member mask as packed bits; the cloud and the labels are regenerated from their seeds.  The script asserts that the
returned points start with `points[mask]` (the pad prefix) or are a subset of it (the crop), and that the set of draws holds a first-try
pass, a pass after at least two failed tries, a fallback, a pad, a crop and a float64-bounds draw."""
import os
import sys
import types

import numpy as np

from tests import train_sample_oracle as TO


def _stub_missing():
    for name in ('natsort', 'open3d', 'tqdm', 'torchvision', 'torchvision.transforms', 'torchvision.transforms.transforms',
                 'torchvision.transforms.functional'):
        try:
            __import__(name)
        except Exception:
            mod = types.ModuleType(name)
            mod.tqdm = lambda x, *a, **k: x
            sys.modules[name] = mod
            if '.' in name:
                setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)


class Recorder:
    """np.random.randint / np.random.choice with a log of (function, first argument, result)."""

    def __enter__(self):
        self.log = []
        self.randint, self.choice = np.random.randint, np.random.choice

        def randint(*a, **k):
            r = self.randint(*a, **k)
            self.log.append(('randint', a[0], r if 'size' in k else int(r)))
            return r

        def choice(*a, **k):
            r = self.choice(*a, **k)
            self.log.append(('choice', a[0], r))
            return r
        np.random.randint, np.random.choice = randint, choice
        return self

    def __exit__(self, *exc):
        np.random.randint, np.random.choice = self.randint, self.choice


def call_with_locals(fn, *args):
    """fn(*args) and the local variables of the `__getitem__` frame at its return."""
    seen = {}

    def hook(frame, event, arg):
        if event == 'return' and frame.f_code.co_name == '__getitem__':
            seen.update(frame.f_locals)
    sys.setprofile(hook)
    try:
        out = fn(*args)
    finally:
        sys.setprofile(None)
    return out, seen


def main(reference_root):
    sys.path.insert(0, reference_root)
    _stub_missing()
    from mvpnet.data.scannet_2d3d import ScanNet2D3DChunks
    from mvpnet.data.scannet_3d import ScanNet3DChunks
    P = TO.FIXTURE
    points = TO.fixture_points()
    n = len(points)
    identity = np.array(list(range(20)) + [-100], np.int64)  # the nyu40 -> class table of this run: raw label 20 = unlabelled
    rows = []
    for kind in P['label_kinds']:
        label = TO.fixture_labels(points, kind)
        raw = np.where(label < 0, 20, label)
        data = [dict(scan_id='fixture', points=points.astype(np.float64), seg_label=raw)]  # the cache holds float64 points; :332 casts
        for seed in range(P['seeds']):
            for nb_pts in P['nb_pts']:
                ds = object.__new__(ScanNet2D3DChunks)
                ds.data, ds.scan_ids, ds.nyu40_to_scannet = data, ['fixture'], identity
                ds.chunk_size = np.array(P['chunk_size'], dtype=np.float32)
                ds.chunk_margin = np.array(P['chunk_margin'], dtype=np.float32)
                ds.chunk_thresh, ds.nb_pts, ds.num_rgbd_frames = P['chunk_thresh'], nb_pts, 0
                ds.z_rot, ds.to_tensor = None, False
                rows.append(run(ds, points, label, kind, seed, nb_pts, False))
            ds = object.__new__(ScanNet3DChunks)
            ds.data, ds.scan_ids, ds.label_mapping = [dict(data[0], seg_label=label)], ['fixture'], None
            ds.chunk_size, ds.chunk_margin, ds.chunk_thresh = np.array(P['chunk_size']), np.array(P['chunk_margin']), P['chunk_thresh']
            ds.use_color, ds.transform = False, None
            rows.append(run(ds, points, label, kind, seed, 0, True))
    tries = np.array([r['try_index'] for r in rows])
    m = np.array([r['m'] for r in rows])
    nb = np.array([r['nb_pts'] for r in rows])
    f64 = np.array([r['f64'] for r in rows])
    assert (tries == 0).any(), 'a first-try pass'
    assert (tries >= 2).any(), 'a pass after at least two failed tries'
    assert (tries == -1).any(), 'a fallback'
    assert ((nb > 0) & (m < nb)).any() and ((nb > 0) & (m >= nb)).any(), 'a pad and a crop'
    assert f64.any() and (f64 & (tries >= 1)).any(), 'float64-bounds draws'
    T = P['num_tries']
    centers = np.full((len(rows), T), -1, np.int32)
    for i, r in enumerate(rows):
        centers[i, :len(r['centers'])] = r['centers']
    kinds = np.array([P['label_kinds'].index(r['kind']) for r in rows], np.int8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'train_sample.npz')
    np.savez_compressed(path, kind=kinds, seed=np.array([r['seed'] for r in rows], np.int32), nb_pts=nb.astype(np.int32), f64=f64,
                        centers=centers, try_index=tries.astype(np.int32), box=np.stack([r['box'] for r in rows]), m=m.astype(np.int32),
                        mask_bits=np.stack([np.packbits(r['mask'], bitorder='little') for r in rows]))
    print('%d draws: tries %s, %d fallbacks, %d pads, %d crops, %d float64' % (
        len(rows), np.bincount(tries[tries >= 0]).tolist(), int((tries < 0).sum()), int(((nb > 0) & (m < nb)).sum()),
        int(((nb > 0) & (m >= nb)).sum()), int(f64.sum())))
    print('wrote', path, os.path.getsize(path), 'bytes')


def run(ds, points, label, kind, seed, nb_pts, f64):
    np.random.seed(1000 * seed + 7 * len(kind) + (1 if f64 else 0) + nb_pts)
    with Recorder() as rec:
        out, loc = call_with_locals(ds.__getitem__, 0)
    centers = [r for f, a, r in rec.log if f == 'randint' and a == len(points) and isinstance(r, int)]
    flag, mask = bool(loc['flag']), np.asarray(loc['chunk_mask'], bool)
    try_index = len(centers) - 1 if flag else -1
    assert flag or len(centers) == 10
    m = int(mask.sum())
    if f64 and not flag:
        box = np.full(4, np.nan)  # scannet_3d.py:173-176 recomputes no bounds
    else:
        box = np.hstack([loc['chunk_min'] - ds.chunk_margin, loc['chunk_max'] + ds.chunk_margin])  # :393
    assert box.dtype == (np.float64 if f64 else np.float32)
    if f64:
        assert np.array_equal(out['points'], points[mask]) and np.array_equal(out['seg_label'], label[mask])
    elif m < nb_pts:
        assert np.array_equal(out['points'][:m], points[mask]) and np.array_equal(out['seg_label'][:m], label[mask])
        pad = [r for f, a, r in rec.log if f == 'randint' and a == m and not isinstance(r, int)]
        assert len(pad) == 1 and np.array_equal(out['points'][m:], points[mask][pad[0]])
    else:
        pick = [r for f, a, r in rec.log if f == 'choice']
        assert len(pick) == 1 and len(np.unique(pick[0])) == nb_pts and np.array_equal(out['points'], points[mask][pick[0]])
    return dict(kind=kind, seed=seed, nb_pts=nb_pts, f64=f64, centers=centers, try_index=try_index, box=box.astype(np.float64), m=m, mask=mask)


if __name__ == '__main__':
    main(sys.argv[1])

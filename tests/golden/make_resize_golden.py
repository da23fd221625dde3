"""Writes tests/golden/resize.npz, resize_labels.tsv, resize_labelids.txt and configs_2d.json: what PILLOW computes for the 2D stage's
resizes, and the reference's label table and 2D config as data.

    python -m tests.golden.make_resize_golden /path/to/the/reference/checkout

resize.npz -- sizes are written H x W -> h x w; Pillow's `size` is (w, h):
  b<H>x<W>_<h>x<w>_in (4,H,W,3) uint8, _out (4,h,w,3) uint8: `Image.fromarray(img).resize((w, h), Image.BILINEAR)` of a random image, a
      0 / 255 checkerboard (the sums reach both ends of clip8), a constant and a smooth ramp with noise.  13x17 -> 5x7: a non-integer
      ratio, 4-5 taps, windows cut at the edges; 11x9 -> 4x9 the vertical pass alone, 7x10 -> 7x4 the horizontal one; 5x7 -> 10x14 an
      enlargement; 96x128 -> 24x32 the production ratio (8 taps); 100x131 -> 37x53.
  n<H>x<W>_<h>x<w>_in (2,H,W) uint16, _out (2,h,w) uint16: `Image.fromarray(lab).resize((w, h), Image.NEAREST)` of "I;16" images, values
      up to 65520.
  label_table (T,) int64: the `raw_to_scannet` table that mvpnet/data/scannet_2d.py:86-103 builds -- its own read_label_mapping and
      load_class_mapping, imported, on the two files below.
resize_labels.tsv: the header and a few dozen rows of the reference's scannetv2-labels.combined.tsv (the 20 benchmark classes' ids, ids
  that map to none of them, gaps between ids); resize_labelids.txt: its labelids.txt.
configs_2d.json: {'unet_resnet34': configs/scannet/unet_resnet34.yaml parsed by PyYAML, 'defaults': the tree of mvpnet/config/sem_seg_2d.py
  imported with a dict stand-in for yacs, as make_golden.py::gen_config_defaults dumps the other two tasks}."""
import copy
import importlib.util
import json
import os
import sys
import types

import numpy as np

from tests.golden.make_train_sample_golden import _stub_missing

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = [((13, 17), (5, 7)), ((11, 9), (4, 9)), ((7, 10), (7, 4)), ((5, 7), (10, 14)), ((96, 128), (24, 32)), ((100, 131), (37, 53))]
TSV_ROWS = 30  # the first rows of the file (the frequent categories), the first row of every benchmark class they miss ...
TSV_EXTRA = (100, 230, 399, 580)  # ... and a few later ones: ids far apart, so the table has gaps (raw ids that map to nyu40 id 0)


def images_of(rs, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (yy[..., None] * 255.0 / max(H - 1, 1) * np.array([1.0, 0.5, 0.0]) + xx[..., None] * 255.0 / max(W - 1, 1) * np.array([0.0, 0.5, 1.0]))
    ramp = np.clip(ramp + rs.randint(-6, 7, (H, W, 3)), 0, 255)
    checker = np.repeat((((yy + xx) % 2) * 255)[..., None], 3, axis=2)
    return np.stack([rs.randint(0, 256, (H, W, 3)), checker, np.full((H, W, 3), 173), ramp]).astype(np.uint8)


def config_defaults_2d(reference_root):
    class CN(dict):
        def __getattr__(self, name):
            try:
                return self[name]
            except KeyError:
                raise AttributeError(name)

        def __setattr__(self, name, value):
            self[name] = value

        def clone(self):
            return copy.deepcopy(self)

    yacs, yacs_config = types.ModuleType('yacs'), types.ModuleType('yacs.config')
    yacs_config.CfgNode = CN
    yacs.config = yacs_config
    sys.modules['yacs'], sys.modules['yacs.config'] = yacs, yacs_config
    for m in [m for m in sys.modules if m == 'common.config' or m.startswith('common.config.')]:
        del sys.modules[m]
    spec = importlib.util.spec_from_file_location('ref_cfg_sem_seg_2d', os.path.join(reference_root, 'mvpnet', 'config', 'sem_seg_2d.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def plain(node):  # tuples -> lists (JSON)
        if isinstance(node, dict):
            return {k: plain(v) for k, v in node.items()}
        if isinstance(node, (tuple, list)):
            return [plain(v) for v in node]
        return node
    return plain(mod._C)


def main(reference_root):
    from PIL import Image
    sys.path.insert(0, reference_root)
    rs = np.random.RandomState(20)
    out = {}
    for (H, W), (h, w) in PAIRS:
        name = '%dx%d_%dx%d' % (H, W, h, w)
        imgs = images_of(rs, H, W)
        res = np.stack([np.asarray(Image.fromarray(im).resize((w, h), Image.BILINEAR)) for im in imgs])
        assert res.shape == (4, h, w, 3) and res.dtype == np.uint8
        out['b' + name + '_in'], out['b' + name + '_out'] = imgs, res
        labs = rs.randint(0, 65521, (2, H, W)).astype(np.uint16)
        labs[0, 0, 0], labs[1, -1, -1] = 65520, 65520
        got = []
        for lab in labs:
            im = Image.fromarray(lab)
            assert im.mode == 'I;16', im.mode
            got.append(np.asarray(im.resize((w, h), Image.NEAREST)))
        got = np.stack(got)
        assert got.shape == (2, h, w) and got.dtype == np.uint16
        out['n' + name + '_in'], out['n' + name + '_out'] = labs, got

    # the label files, cut down, and the reference's table from them
    meta = os.path.join(reference_root, 'mvpnet', 'data', 'meta_files')
    with open(os.path.join(meta, 'scannetv2-labels.combined.tsv')) as f:
        lines = f.read().splitlines()
    with open(os.path.join(meta, 'labelids.txt')) as f:
        classes = [l.split('\t')[0] for l in f.read().splitlines() if l.strip()]
    col = lines[0].split('\t').index('nyu40id')
    first = {}
    for i, line in enumerate(lines[1:], 1):
        first.setdefault(line.split('\t')[col], i)
    rows = sorted(set(range(1, 1 + TSV_ROWS)) | {first[c] for c in classes} | set(TSV_EXTRA))
    keep = [lines[0]] + [lines[i] for i in rows]
    tsv_path, ids_path = os.path.join(HERE, 'resize_labels.tsv'), os.path.join(HERE, 'resize_labelids.txt')
    with open(tsv_path, 'w') as f:
        f.write('\n'.join(keep) + '\n')
    with open(os.path.join(meta, 'labelids.txt')) as f, open(ids_path, 'w') as g:
        g.write(f.read())
    _stub_missing()
    from mvpnet.data.scannet_2d import read_label_mapping, load_class_mapping
    mapping = read_label_mapping(tsv_path, label_from='id', label_to='nyu40id', as_int=True)  # scannet_2d.py:88-103, line by line
    raw_to_nyu40 = np.zeros(max(mapping.keys()) + 1, dtype=np.int64)
    for key, value in mapping.items():
        raw_to_nyu40[key] = value
    scannet_mapping = load_class_mapping(ids_path)
    assert len(scannet_mapping) == 20
    nyu40_to_scannet = np.full(shape=41, fill_value=-100, dtype=np.int64)
    nyu40_to_scannet[list(scannet_mapping.keys())] = np.arange(len(scannet_mapping))
    out['label_table'] = nyu40_to_scannet[raw_to_nyu40]
    assert sorted(set(out['label_table'].tolist())) == [-100] + list(range(20))

    path = os.path.join(HERE, 'resize.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; label table of', len(out['label_table']), 'ids')

    import yaml
    with open(os.path.join(reference_root, 'configs', 'scannet', 'unet_resnet34.yaml')) as f:
        cfgs = {'unet_resnet34': yaml.safe_load(f), 'defaults': config_defaults_2d(reference_root)}
    path = os.path.join(HERE, 'configs_2d.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main(sys.argv[1])

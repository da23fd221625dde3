"""The 2D stage without a GPU: the NumPy oracle (tests/resize_oracle.py) against Pillow's own results (tests/golden/resize.npz), the
library's host table functions against the oracle, and the config / model plumbing of `sem_seg_2d` against the reference's data
(tests/golden/configs_2d.json, resize_labels.tsv, resize_labelids.txt).  No kernel runs."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from tests import resize_oracle as RO
from tests.conftest import GOLDEN

PAIRS = ['13x17_5x7', '11x9_4x9', '7x10_7x4', '5x7_10x14', '96x128_24x32', '100x131_37x53']  # H x W -> h x w
AXES = sorted({(13, 5), (17, 7), (11, 4), (10, 4), (5, 10), (7, 14), (96, 24), (128, 32), (100, 37), (131, 53), (640, 160), (1296, 160), (968, 120),
               (480, 120)})


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'resize.npz'))


# ---- the oracle is Pillow ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIRS)
def test_oracle_bilinear_equals_pillow(golden, pair):
    src, pil = golden['b' + pair + '_in'], golden['b' + pair + '_out']
    h, w = pil.shape[1:3]
    assert len(src) == 4
    got = RO.resize_frames(src, np.arange(4), (w, h))
    assert got.dtype == np.uint8 and np.array_equal(got, pil)


def test_the_pass_order_is_observable(golden):
    """vertical-first differs from Pillow where both axes change by a non-trivial ratio: the fixtures tell the two orders apart"""
    src, pil = golden['b13x17_5x7_in'], golden['b13x17_5x7_out']
    other = np.stack([RO.resize_bilinear(im, (7, 5), vertical_first=True) for im in src])
    assert int((other != pil).sum()) >= 10


@pytest.mark.parametrize('pair', PAIRS)
def test_oracle_nearest_equals_pillow(golden, pair):
    src, pil = golden['n' + pair + '_in'], golden['n' + pair + '_out']
    h, w = pil.shape[1:3]
    assert src.dtype == np.uint16 and int(src.max()) == 65520
    assert np.array_equal(np.stack([RO.resize_nearest(lab, (w, h)) for lab in src]), pil)


def test_the_product_rule_differs_from_the_accumulating_one():
    """100 -> 37 and 131 -> 53: the index Pillow takes for 16-bit images is not the one an accumulated coordinate gives"""
    def accumulating(inS, outS):
        step, at, out = inS / outS, inS / outS * 0.5, []
        for _ in range(outS):
            out.append(min(int(at), inS - 1))
            at += step
        return np.array(out, np.int32)
    assert any(not np.array_equal(RO.nearest_table(a, b), accumulating(a, b)) for a, b in ((100, 37), (131, 53)))


# ---- the library's host tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inS,outS', AXES)
def test_library_tables_equal_the_oracle(inS, outS):
    from mvpnet_amd.ops import resize as R
    xmin, count, coef, ksize = R.bilinear_table(inS, outS)
    exmin, ecount, ecoef, eksize = RO.bilinear_table(inS, outS)
    assert ksize == eksize and coef.shape == (outS, ksize) and coef.dtype == np.int32
    assert np.array_equal(xmin, exmin) and np.array_equal(count, ecount) and np.array_equal(coef, ecoef)
    assert int(count.max()) <= ksize and int((xmin + count).max()) <= inS and int(xmin.min()) >= 0
    index = R.nearest_table(inS, outS)
    assert index.dtype == np.int32 and np.array_equal(index, RO.nearest_table(inS, outS))
    assert 0 <= int(index.min()) and int(index.max()) <= inS - 1


def test_tap_counts_of_the_production_sizes():
    from mvpnet_amd.ops import resize as R
    assert int(R.bilinear_table(640, 160)[1].max()) == 8 and R.bilinear_table(640, 160)[3] == 9
    assert int(R.bilinear_table(1296, 160)[1].max()) == 17 and R.bilinear_table(1296, 160)[3] == 19
    assert R.bilinear_table(5, 10)[3] == 3  # an enlargement: the support is one input pixel


def test_table_argument_errors():
    import ctypes
    from mvpnet_amd import _lib as L
    lib = L.lib()
    k = ctypes.c_int32(0)
    assert lib.mvp_resize_bilinear_table(0, 4, None, None, None, ctypes.byref(k)) == -1
    assert lib.mvp_resize_bilinear_table(8, 4, None, None, None, None) == -3
    assert lib.mvp_resize_bilinear_table(8, 4, None, None, None, ctypes.byref(k)) == 0 and k.value == 5
    assert lib.mvp_resize_nearest_table(8, 0, ctypes.c_void_p(16)) == -1
    assert lib.mvp_resize_nearest_table(8, 4, None) == -3
    dummy = ctypes.c_void_p(16)
    # precondition failures of the two device entry points return before any HIP call (safe without a GPU)
    assert lib.mvp_resize_frames_u8(dummy, 1, 8, 8, dummy, 1, 4, 4, None, dummy, dummy, None) == -1      # the width changes: xtab is needed
    assert lib.mvp_resize_frames_u8(dummy, 1, 8, 8, dummy, 1, 8, 4, dummy, dummy, dummy, None) == -1     # the height does not: no ytab
    assert lib.mvp_resize_frames_u8(dummy, 1, 2000, 8, dummy, 1, 10, 4, dummy, dummy, dummy, None) == -2  # 401 taps
    assert lib.mvp_resize_frames_u8(dummy, 1, 600, 8, dummy, 1, 20, 4, dummy, dummy, dummy, None) == -2   # 61 taps fit, 272 rows in LDS do not
    assert lib.mvp_resize_frames_u8(None, 1, 8, 8, dummy, 1, 4, 4, dummy, dummy, dummy, None) == -3
    assert lib.mvp_prepare_labels_u16(dummy, 1, 8, 8, dummy, 1, 4, 8, None, None, None, None, 0, -100, dummy, None) == -1  # yi is needed
    assert lib.mvp_prepare_labels_u16(dummy, 1, 8, 8, dummy, 0, 8, 8, None, None, None, None, 0, -100, dummy, None) == -1


def test_ops_refuse_host_tensors():
    import mvpnet_amd.ops as ops
    with pytest.raises(RuntimeError):
        ops.resize_frames(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), (4, 4))
    with pytest.raises(RuntimeError):
        ops.prepare_labels(torch.zeros(2, 8, 8, dtype=torch.uint16), torch.zeros(1, dtype=torch.int64))


# ---- the label table ------------------------------------------------------------------------------------------------------------------
def test_label_mapping_equals_the_reference_table(golden):
    from mvpnet_amd import config as C
    table = C.scannet_label_mapping(os.path.join(GOLDEN, 'resize_labels.tsv'), os.path.join(GOLDEN, 'resize_labelids.txt'))
    assert table.dtype == torch.int64 and np.array_equal(table.numpy(), golden['label_table'])
    assert sorted(set(table.tolist())) == [-100] + list(range(20))
    with open(os.path.join(GOLDEN, 'resize_labels.tsv')) as f, open(os.path.join(GOLDEN, 'resize_labelids.txt')) as g:
        assert np.array_equal(RO.scannet_label_mapping(f.read(), g.read()), golden['label_table'])
    other = C.scannet_label_mapping(os.path.join(GOLDEN, 'resize_labels.tsv'), os.path.join(GOLDEN, 'resize_labelids.txt'), ignore_value=255)
    assert np.array_equal(other.numpy(), np.where(golden['label_table'] < 0, 255, golden['label_table']))


def test_oracle_labels_flip_and_mapping():
    labels = np.arange(2 * 3 * 4, dtype=np.uint16).reshape(2, 3, 4)
    mapping = np.arange(20, dtype=np.int64) * 10
    out = RO.prepare_labels(labels, [1, 0, 5], flip=[1, 0, 0], mapping=mapping)
    assert np.array_equal(out[1], labels[0].astype(np.int64) * 10)
    assert np.array_equal(out[0], np.where(labels[1] < 20, labels[1].astype(np.int64) * 10, -100)[:, ::-1])
    assert np.array_equal(out[2], np.where(labels[1] < 20, labels[1].astype(np.int64) * 10, -100))  # row 5 is clamped to the last frame


# ---- config and model --------------------------------------------------------------------------------------------------------------------
def _plain(node):
    if isinstance(node, dict):
        return {k: _plain(v) for k, v in node.items()}
    if isinstance(node, (tuple, list)):
        return [_plain(v) for v in node]
    return node


@pytest.fixture(scope='module')
def configs():
    with open(os.path.join(GOLDEN, 'configs_2d.json')) as f:
        return json.load(f)


def test_default_tree_equals_the_reference_module(configs):
    from mvpnet_amd import config as C
    assert _plain(C.get_cfg_sem_seg_2d()) == configs['defaults']


def test_the_yaml_loads(configs):
    """load_cfg on the YAML's text = the parsed YAML over the defaults, purged by TYPE"""
    from mvpnet_amd import config as C
    raw = configs['unet_resnet34']
    cfg = C.load_cfg(text=yaml.safe_dump(raw))
    assert cfg.TASK == 'sem_seg_2d' and cfg.MODEL.TYPE == 'UNetResNet34' and cfg.DATASET.TYPE == 'ScanNet2D'

    def check(node, want):  # every value of the YAML is in the tree (strings such as "(160, 120)" evaluated like yacs does)
        for k, v in want.items():
            if isinstance(v, dict):
                check(node[k], v)
            else:
                assert _plain(node[k]) == _plain(C.CfgNode._convert(v)), k
    check(cfg, raw)
    assert cfg.DATASET.ScanNet2D.resize == (160, 120) and cfg.DATASET.ScanNet2D.augmentation.color_jitter == (0.4, 0.4, 0.4)
    assert cfg.DATASET.ScanNet2D.normalizer == ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))  # (the default: the YAML does not set it)
    assert cfg.MODEL.UNetResNet34.p == 0.5 and cfg.TRAIN.BATCH_SIZE == 32 and cfg.OPTIMIZER.TYPE == 'SGD'
    assert 'StepLR' not in cfg.SCHEDULER and cfg.SCHEDULER.MultiStepLR.milestones == (60000, 70000)  # purged
    # the keys outside the YAML are the defaults
    rest = _plain(cfg)
    assert rest['VAL']['METRIC'] == 'seg_iou' and rest['VAL']['REPEATS'] == 1 and rest['DATALOADER']['DROP_LAST'] is True


def test_build_batch_2d(configs):
    import inspect
    from mvpnet_amd import config as C
    from mvpnet_amd import scene as SC
    cfg = C.load_cfg(text=yaml.safe_dump(configs['unet_resnet34']))
    train, val = C.build_batch_2d(cfg, training=True), C.build_batch_2d(cfg, training=False)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert train == {'resize': (160, 120), 'image_normalizer': norm, 'color_jitter': (0.4, 0.4, 0.4), 'flip': 0.5}
    assert val == {'resize': (160, 120), 'image_normalizer': norm, 'color_jitter': (), 'flip': 0.0}
    params = inspect.signature(SC.sample_train_batch_2d).parameters
    assert all(k in params and params[k].kind == inspect.Parameter.KEYWORD_ONLY for k in train)
    bare = C.load_cfg(text='TASK: sem_seg_2d\nDATASET:\n  TYPE: ScanNet2D\n')
    assert C.build_batch_2d(bare) == {'resize': None, 'image_normalizer': norm, 'color_jitter': (), 'flip': 0.0}
    with pytest.raises(ValueError):
        C.build_batch_2d(C.load_cfg(text='TASK: sem_seg_2d\nDATASET:\n  TYPE: Other\n'))


def test_build_model_and_loss_2d(configs, tmp_path):
    from mvpnet_amd import config as C
    from mvpnet_amd.mvpnet3d import SegLoss
    raw = json.loads(json.dumps(configs['unet_resnet34']))
    weights = tmp_path / 'weights.txt'
    weights.write_text('\n'.join('%.6f' % (1.0 + 0.1 * i) for i in range(20)) + '\n')
    raw['TRAIN']['LABEL_WEIGHTS_PATH'] = str(weights)
    cfg = C.load_cfg(text=yaml.safe_dump(raw))
    model = C.build_model_sem_seg_2d(cfg)
    assert type(model).__name__ == 'UNetResNet34' and model.num_classes == 20
    drops = [m.p for m in model.modules() if isinstance(m, torch.nn.Dropout)]
    assert drops and all(p == 0.5 for p in drops)
    loss = C.build_loss_2d(cfg)
    assert isinstance(loss, SegLoss) and loss.weight.dtype == torch.float32
    assert np.array_equal(loss.weight.cpu().numpy(), np.loadtxt(str(weights), dtype=np.float32))
    raw['TRAIN']['LABEL_WEIGHTS_PATH'] = ''
    assert C.build_loss_2d(C.load_cfg(text=yaml.safe_dump(raw))).weight is None
    assert C.build_optimizer(cfg, model).defaults['lr'] == 0.005


def test_rank_4_logits_are_viewed_not_copied():
    """(B,C,H,W) -> (B,C,H*W) shares the logits' memory in both layouts: what SegLoss and confusion_matrix hand to the kernels"""
    x = torch.randn(2, 20, 6, 8)
    for logit in (x, x.contiguous(memory_format=torch.channels_last)):
        flat = logit.flatten(2)
        assert flat.data_ptr() == logit.data_ptr() and tuple(flat.shape) == (2, 20, 48) and torch.equal(flat.reshape(2, 20, 6, 8), logit)
    assert x.contiguous(memory_format=torch.channels_last).flatten(2).stride() == (960, 1, 20)


def test_host_rank_4_loss_and_confusion():
    """host tensors take the torch path, rank 4 included (the reference's own arithmetic)"""
    from mvpnet_amd import metric as M
    from mvpnet_amd.mvpnet3d import SegLoss
    g = torch.Generator().manual_seed(3)
    logit = torch.randn(2, 20, 6, 8, generator=g)
    label = torch.randint(0, 20, (2, 6, 8), generator=g)
    label[0, :2] = -100
    loss = SegLoss()({'seg_logit': logit}, {'seg_label': label})['seg_loss']
    assert torch.allclose(loss, torch.nn.functional.cross_entropy(logit, label, ignore_index=-100))
    keep = label != -100
    ref = torch.bincount(20 * label[keep] + logit.argmax(1)[keep], minlength=400).reshape(20, 20)
    assert torch.equal(M.confusion_matrix(logit, label), ref)


def test_draw_frames_on_the_host():
    from mvpnet_amd import augment as A
    rows = A.draw_frames(1000, 7, 'cpu', generator=torch.Generator().manual_seed(1))
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (1000,) and int(rows.min()) == 0 and int(rows.max()) == 6
    assert 'replacement' in A.draw_frames.__doc__

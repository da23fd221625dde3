"""The 2D stage on the MI355X: ops.resize_frames (mvp_resize_frames_u8) and ops.prepare_labels (mvp_prepare_labels_u16) bit for bit
against Pillow's own results (tests/golden/resize.npz) and the NumPy restatement (tests/resize_oracle.py); scene.sample_train_batch_2d
against the oracle fed the same draws; SegLoss and metric.confusion_matrix on (B,C,H,W) logits."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resize_oracle as RO
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NORMALIZER = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
MEAN_STD = np.array(NORMALIZER[0] + NORMALIZER[1], np.float32)
PAIRS = ['13x17_5x7', '11x9_4x9', '7x10_7x4', '5x7_10x14', '96x128_24x32', '100x131_37x53']  # H x W -> h x w


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'resize.npz'))


def same_bits(got, exp):
    got = got.contiguous().cpu().numpy()
    return got.dtype == np.float32 and got.shape == exp.shape and np.array_equal(got.view(np.uint32), np.ascontiguousarray(exp).view(np.uint32))


def count_diff(got, exp):
    got = got.cpu().numpy()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    return int((got != exp).sum())


# ---- resize_frames ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIRS)
def test_resize_equals_pillow(golden, pair):
    """a golden group in one call: rows that repeat, out of order, one behind the store and one in front of it (clamped)"""
    import mvpnet_amd.ops as ops
    src, pil = golden['b' + pair + '_in'], golden['b' + pair + '_out']
    h, w = pil.shape[1:3]
    picked = np.array([3, 0, 0, 2, 1, 3, 9, -1], np.int64)
    out = ops.resize_frames(t(src), t(picked), (w, h))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (8, h, w, 3) and out.is_contiguous()
    diff = count_diff(out, pil[np.clip(picked, 0, 3)])
    print(pair, 'values that differ from Pillow:', diff)
    assert diff == 0
    grid = ops.resize_frames(t(src), t(picked.reshape(2, 4)), (w, h))  # picked of any shape
    assert tuple(grid.shape) == (2, 4, h, w, 3) and torch.equal(grid.view(8, h, w, 3), out)


@pytest.mark.parametrize('H,W,frames,picked', [(480, 640, 4, [2, 0, 3]), (240, 320, 2, [1, 0]), (968, 1296, 2, [1]), (120, 160, 3, [2, 2, 0])])
def test_resize_equals_the_oracle_at_the_production_sizes(H, W, frames, picked):
    """-> 120 x 160: the 8-tap path, the 4-tap one, the 17-tap one (up to 75 intermediate rows per tile) and the plain gather"""
    import mvpnet_amd.ops as ops
    rs = np.random.RandomState(H)
    src = rs.randint(0, 256, (frames, H, W, 3)).astype(np.uint8)
    src[0, : H // 2] = (np.arange(W)[None, :, None] * 255 // (W - 1)).astype(np.uint8)  # a smooth half
    out = ops.resize_frames(t(src), t(np.array(picked, np.int64)), (160, 120))
    diff = count_diff(out, RO.resize_frames(src, picked, (160, 120)))
    print('%dx%d -> 120x160: values that differ from the oracle: %d' % (H, W, diff))
    assert diff == 0


def test_resize_no_frames_and_refused_sizes():
    import mvpnet_amd.ops as ops
    frames = torch.zeros((2, 16, 20, 3), dtype=torch.uint8, device=DEV)
    none = ops.resize_frames(frames, torch.zeros((0,), dtype=torch.int64, device=DEV), (5, 4))
    assert tuple(none.shape) == (0, 4, 5, 3) and none.dtype == torch.uint8
    tall = torch.zeros((1, 2000, 8, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r'code -2'):  # 401 taps: refused by the entry point, nothing is launched
        ops.resize_frames(tall, torch.zeros(1, dtype=torch.int64, device=DEV), (4, 10))
    with pytest.raises(RuntimeError):
        ops.resize_frames(frames.float(), torch.zeros(1, dtype=torch.int64, device=DEV), (5, 4))
    with pytest.raises(RuntimeError):
        ops.resize_frames(frames, torch.zeros(1, dtype=torch.int32, device=DEV), (5, 4))
    with pytest.raises(RuntimeError):
        ops.resize_frames(frames, torch.zeros(1, dtype=torch.int64, device=DEV), (5, 0))
    torch.cuda.synchronize()


# ---- prepare_labels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIRS)
def test_labels_equal_pillow(golden, pair):
    """the golden groups: the raw resize is Pillow's; with a flip and a mapping it is the oracle's (which is held to Pillow)"""
    import mvpnet_amd.ops as ops
    src, pil = golden['n' + pair + '_in'], golden['n' + pair + '_out']
    h, w = pil.shape[1:3]
    picked = np.array([1, 0, 0, 1, 7, -2], np.int64)
    rows = np.clip(picked, 0, 1)
    labels = t(src)
    out = ops.prepare_labels(labels, t(picked), (w, h))
    assert out.dtype == torch.int64 and tuple(out.shape) == (6, h, w)
    assert count_diff(out, pil[rows].astype(np.int64)) == 0
    rs = np.random.RandomState(h)
    mapping = rs.randint(-100, 20, 40000).astype(np.int64)  # raw ids reach 65520: both sides of T are hit
    flip = np.array([1, 0, 1, 0, 1, 1], np.uint8)
    for fl in (None, flip):
        for mp in (None, mapping):
            got = ops.prepare_labels(labels, t(picked), (w, h), flip=None if fl is None else t(fl), mapping=None if mp is None else t(mp))
            assert count_diff(got, RO.prepare_labels(src, picked, (w, h), fl, mp)) == 0
    mirrored = ops.prepare_labels(labels, t(picked), (w, h), flip=t(flip))
    assert torch.equal(mirrored, torch.where(t(flip).bool().view(6, 1, 1), out.flip(-1), out))  # a flipped row is the mirror of the plain one
    as_bool = ops.prepare_labels(labels, t(picked), (w, h), flip=t(flip).bool())
    assert torch.equal(as_bool, mirrored)


@pytest.mark.parametrize('W', [7, 160])
def test_labels_at_the_store_size_and_the_end_of_the_table(W):
    """no resize (no tables); raw ids T - 1, T and T + 1: the last entry, then ignore_value"""
    import mvpnet_amd.ops as ops
    rs = np.random.RandomState(W)
    T = 41
    src = rs.randint(0, 60, (3, 5, W)).astype(np.uint16)
    src[0, 0, :3] = (T - 1, T, T + 1)
    src[2, 4, -1] = 65535
    mapping = rs.randint(0, 20, T).astype(np.int64)
    picked = np.array([2, 0, 1, 0], np.int64)
    flip = np.array([0, 1, 1, 0], np.uint8)
    got = ops.prepare_labels(t(src), t(picked), flip=t(flip), mapping=t(mapping), ignore_value=255)
    assert count_diff(got, RO.prepare_labels(src, picked, None, flip, mapping, 255)) == 0
    plain = ops.prepare_labels(t(src), t(picked), mapping=t(mapping)).cpu().numpy()
    assert plain[1, 0, 0] == mapping[T - 1] and plain[1, 0, 1] == -100 and plain[1, 0, 2] == -100 and plain[0, 4, -1] == -100
    raw = ops.prepare_labels(t(src), t(picked))
    assert count_diff(raw, src[picked].astype(np.int64)) == 0
    same = ops.prepare_labels(t(src), t(picked), (W, 5))  # the store's own size
    assert torch.equal(same, raw)
    assert tuple(ops.prepare_labels(t(src), torch.zeros((0, 2), dtype=torch.int64, device=DEV), (3, 2)).shape) == (0, 2, 2, 3)
    with pytest.raises(RuntimeError):
        ops.prepare_labels(t(src.astype(np.int16)), t(picked))
    with pytest.raises(RuntimeError):
        ops.prepare_labels(t(src), t(picked), mapping=t(mapping.astype(np.int32)))
    with pytest.raises(RuntimeError):
        ops.prepare_labels(t(src), t(picked), flip=t(flip[:3]))


# ---- sample_train_batch_2d -------------------------------------------------------------------------------------------------------------
def _store_2d():
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:48, 0:64]
    smooth = np.stack([(yy * 5 + xx * f) % 256 for f in (1, 2, 3)], axis=-1)
    images = np.clip(smooth[None] + rs.randint(-40, 41, (6, 48, 64, 3)), 0, 255).astype(np.uint8)
    labels = rs.randint(0, 45, (6, 48, 64)).astype(np.uint16)
    mapping = rs.randint(-1, 20, 41).astype(np.int64)
    mapping[mapping < 0] = -100
    return images, labels, mapping


@pytest.mark.parametrize('resize', [(16, 12), (64, 48), None])
@pytest.mark.parametrize('channels_last', [False, True])
def test_sample_train_batch_2d(resize, channels_last):
    """6 frames of 48 x 64 -> 12 x 16 (and at the store's own size), jitter, flip and normaliser on: image bits and labels are the
    oracle's for the same draws, and the call synchronises nothing"""
    from mvpnet_amd import augment as A
    from mvpnet_amd import scene as SC
    images, labels, mapping = _store_2d()
    store = {'images': t(images), 'labels': t(labels)}
    picked = t(np.array([4, 1, 1, 0, 5, 2, 3, 3], np.int64))
    gen = lambda: torch.Generator(device=DEV).manual_seed(23)
    kw = dict(resize=resize, color_jitter=(0.4, 0.4, 0.4), image_normalizer=NORMALIZER, flip=0.5, label_mapping=t(mapping), channels_last=channels_last)
    SC.sample_train_batch_2d(store, picked, generator=gen(), **kw)  # (the tables and the normaliser's 6 floats exist from here on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        batch = SC.sample_train_batch_2d(store, picked, generator=gen(), **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert sorted(batch) == ['image', 'seg_label']
    h, w = (12, 16) if resize == (16, 12) else (48, 64)
    image, label = batch['image'], batch['seg_label']
    assert tuple(image.shape) == (8, 3, h, w) and image.dtype == torch.float32 and tuple(label.shape) == (8, h, w) and label.dtype == torch.int64
    assert image.is_contiguous() != channels_last
    if channels_last:
        assert image.stride() == (h * w * 3, 1, w * 3, 3)
    g = gen()
    factor, order = A.draw_color_jitter(8, kw['color_jitter'], DEV, generator=g)
    flip = A.draw_flip(8, 0.5, DEV, generator=g)
    assert 0 < int(flip.sum()) < 8
    eimage, elabel = RO.sample_train_batch_2d(images, labels, picked.cpu().numpy(), resize, factor.cpu().numpy(), order.cpu().numpy(), flip.cpu().numpy(),
                                              MEAN_STD, mapping)
    assert same_bits(image, eimage)
    assert count_diff(label, elabel) == 0
    # a flipped row's label is the mirror of the unflipped one's (rows 1 and 2 and rows 6 and 7 are the same frame)
    quiet = SC.sample_train_batch_2d(store, picked, resize=resize, label_mapping=t(mapping), generator=gen())
    assert torch.equal(label, torch.where(flip.bool().view(8, 1, 1), quiet['seg_label'].flip(-1), quiet['seg_label']))
    assert torch.equal(quiet['seg_label'][1], quiet['seg_label'][2])
    plain = RO.sample_train_batch_2d(images, labels, picked.cpu().numpy(), resize)
    assert same_bits(quiet['image'], plain[0])  # no jitter, no normaliser: u / 255


def test_draw_frames_on_the_device():
    from mvpnet_amd import augment as A
    gen = torch.Generator(device=DEV).manual_seed(1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        rows = A.draw_frames(4096, 6, DEV, generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert rows.device.type == 'cuda' and rows.dtype == torch.int64
    counts = torch.bincount(rows, minlength=6).cpu().numpy()
    assert len(counts) == 6 and (np.abs(counts - 4096 / 6) < 150).all(), counts  # sd ~ 24


# ---- loss and confusion matrix on (B,C,H,W) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['contiguous', 'channels_last'])
def test_loss_and_confusion_on_rank_4_logits(layout):
    """(2,20,6,8) logits with weights and ignored pixels: the bars of tests/test_seg_gpu.py's rank-3 cases; the HIP path ran"""
    from mvpnet_amd import metric as M
    from mvpnet_amd.mvpnet3d import SegLoss, _SegLossFn
    g = torch.Generator(device=DEV).manual_seed(11)
    base = torch.randn(2, 20, 6, 8, device=DEV, generator=g) * 3
    if layout == 'channels_last':
        base = base.contiguous(memory_format=torch.channels_last)
        assert not base.is_contiguous()
    label = torch.randint(0, 20, (2, 6, 8), device=DEV, generator=g)
    label[torch.rand(2, 6, 8, device=DEV, generator=g) < 0.15] = -100
    weight = torch.rand(20, device=DEV, generator=g) + 0.5
    for w in (weight, None):
        a = base.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        b = base.detach().clone().contiguous().requires_grad_(True)
        crit = SegLoss(weight=w)
        _SegLossFn.last_acc = None
        la = crit({'seg_logit': a}, {'seg_label': label})['seg_loss']
        lb = F.cross_entropy(b, label, weight=w, ignore_index=-100)
        # the kernel's own accumulator: sum of w[label] over the valid pixels
        assert _SegLossFn.last_acc is not None and crit.last_weight_sum is not None  # set by the HIP path's forward, reset above
        valid = label != -100
        want = float(valid.sum()) if w is None else float(w[label[valid]].double().sum())
        np.testing.assert_allclose(float(_SegLossFn.last_acc[1]), want, rtol=1e-6)
        np.testing.assert_allclose(float(crit.last_weight_sum), want, rtol=1e-6)
        la.backward()
        lb.backward()
        np.testing.assert_allclose(la.item(), lb.item(), rtol=1e-5)
        assert a.grad.shape == a.shape and a.grad.stride() == a.stride()  # the gradient in the logits' own layout
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.cpu().numpy(), rtol=1e-4, atol=1e-10)
    mat = M.confusion_matrix(base, label)
    keep = label != -100
    ref = torch.bincount(20 * label[keep] + base.argmax(1)[keep], minlength=400).reshape(20, 20)
    assert torch.equal(mat, ref)
    M.confusion_matrix(base, label, out=mat)
    assert torch.equal(mat, 2 * ref)
    iou = M.SegIoU(20)
    iou.update_dict({'seg_logit': base}, {'seg_label': label})
    assert torch.equal(iou.mat, ref)

"""Stage one's test, validation and class weights on the MI355X: ops.frame_confusion (mvp_frame_confusion_f32) and ops.label_histogram
(mvp_label_histogram_u16 / _i64) against the NumPy oracle and the reference's results (tests/golden/frame_eval.npz), and the entry points
on top of them -- mvpnet2d.test_frames_2d / validate_2d, scene.label_weights_2d / _3d -- against the pieces the project had before them.
Every comparison is integer-exact (the weights and the loss: bit for bit)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml
from torch import nn

from tests import frame_eval_oracle as FO
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NORMALIZER = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
T = FO.FIX_T


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'frame_eval.npz'))


@pytest.fixture(scope='module')
def store():
    """(5,23,31) uint16 raw ids in [0,48); frame 3 holds ids past every mapping here (T = 41) only: entirely ignored"""
    labels = FO.fixture_inputs()['labels'].copy()
    labels[3] = 41 + labels[3] % 7
    return labels


def mapping_for(C):
    """(41,) int64: C = 20 -- the benchmark table, -100 elsewhere; else every value of [-1, C] (-1 and C count nowhere) and some -100"""
    if C == 20:
        return FO.fixture_inputs()['mapping']
    m = np.arange(T, dtype=np.int64) % (C + 2) - 1
    m[::9] = -100
    return m


def logits_for(Nf, C, h, w, seed):
    """random logits with planted exact ties: classes 0 and C-1 above the rest in column 1 of frame 0, a row of frame 1 all equal"""
    x = np.random.RandomState(seed).standard_normal((Nf, C, h, w)).astype(np.float32)
    x[0, 0, :, 1] = x[0, C - 1, :, 1] = 9.0
    x[1, :, 2, :] = 0.5
    if C > 2:
        x[Nf - 1, C - 1, 0, :] = x[Nf - 1, C - 2, 0, :] = 8.0
    return x


def laid_out(x, layout):
    """the (Nf,C,h,w) values of x on the device in the given memory: nchw, cl (channels-last), or either with a padded frame stride
    (pad 5: rows that are not 16-byte aligned; cl_pad8: aligned)"""
    Nf, C, h, w = x.shape
    n = C * h * w
    if layout == 'nchw':
        out = t(x)
    elif layout == 'cl':
        out = t(x).contiguous(memory_format=torch.channels_last)
    else:
        pad = 8 if layout.endswith('8') else 5
        buf = torch.zeros((Nf, n + pad), dtype=torch.float32, device=DEV)
        strides = (n + pad, h * w, w, 1) if layout.startswith('nchw') else (n + pad, 1, w * C, C)
        out = torch.as_strided(buf, (Nf, C, h, w), strides)
        out.copy_(t(x))
        assert out.stride() == strides
    assert torch.equal(out.cpu(), torch.from_numpy(x))
    return out


# ---- frame_confusion ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(7, 5), None])
@pytest.mark.parametrize('layout', ['nchw', 'cl', 'nchw_pad5', 'cl_pad5', 'cl_pad8'])
@pytest.mark.parametrize('C', [3, 20, 36, 70])
def test_frame_confusion_equals_the_oracle(store, C, layout, size):
    """picked out of order and repeated, 4 x 35 or 4 x 713 pixels (no multiple of the workgroup), a mapping shorter than the largest raw id
    that sends ids to -100, planted ties, want_pred, then a second call into the same matrix whose first frame is entirely ignored.
    C = 3: one dword per class; 20: 16-byte quads when the rows are aligned (cl, cl_pad8); 36: the loop over classes, LDS histogram;
    70: the loop, global atomics."""
    import mvpnet_amd.ops as ops
    h, w = (5, 7) if size else store.shape[1:]
    mapping = mapping_for(C)
    assert int(store.max()) >= T and (mapping == -100).any()
    x1, x2 = logits_for(4, C, h, w, C), logits_for(2, C, h, w, C + 1)
    p1, p2 = np.array([4, 0, 0, 2], np.int64), np.array([3, 1], np.int64)
    mat, pred = ops.frame_confusion(laid_out(x1, layout), t(store), t(p1), size=size, mapping=t(mapping), want_pred=True)
    emat, epred = FO.frame_confusion(x1, store, p1, size=size, mapping=mapping)
    assert mat.dtype == torch.int64 and tuple(mat.shape) == (C, C) and np.array_equal(mat.cpu().numpy(), emat) and int(emat.sum()) > 0
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), epred)
    assert (epred[0, :, 1] == 0).all() and (epred[1, 2, :] == 0).all() and (epred[3, 0, :] == C - 2).all()  # the first maximum
    again = ops.frame_confusion(laid_out(x2, layout), t(store), t(p2), size=size, mapping=t(mapping), out=mat)
    assert again is mat
    emat2, _ = FO.frame_confusion(x2, store, p2, size=size, mapping=mapping, out=emat)
    assert np.array_equal(mat.cpu().numpy(), emat2) and int(emat2.sum()) > int(emat.sum())
    ignored = ops.frame_confusion(laid_out(x2[:1], layout), t(store), t(p2[:1]), size=size, mapping=t(mapping))
    assert int(ignored.sum()) == 0


def test_frame_confusion_without_a_mapping_and_clamped_rows(store):
    """raw ids as classes (ids >= C count nowhere); rows outside the store are clamped; picked of another shape"""
    import mvpnet_amd.ops as ops
    x = logits_for(4, 44, 5, 7, 9)
    picked = np.array([[-3, 1], [9, 2]], np.int64)
    mat = ops.frame_confusion(t(x), t(store), t(picked), size=(7, 5))
    emat, _ = FO.frame_confusion(x, store, picked, size=(7, 5))
    assert np.array_equal(mat.cpu().numpy(), emat) and 0 < int(emat.sum()) < 4 * 35
    other = ops.frame_confusion(t(x), t(store), t(picked), size=(7, 5), mapping=t(np.full(T, 7, np.int64)), ignore_value=2)
    eother, _ = FO.frame_confusion(x, store, picked, size=(7, 5), mapping=np.full(T, 7, np.int64), ignore_value=2)
    assert np.array_equal(other.cpu().numpy(), eother) and int(eother[2].sum()) > 0  # (an ignore_value inside [0,C) is a class)


def test_frame_confusion_many_frames(store):
    """300 frames: one workgroup per frame walks its 713 pixels with a stride"""
    import mvpnet_amd.ops as ops
    picked = np.arange(300, dtype=np.int64) % 5
    x = np.random.RandomState(2).standard_normal((300, 3, 23, 31)).astype(np.float32)
    mapping = mapping_for(3)
    mat, pred = ops.frame_confusion(t(x), t(store), t(picked), mapping=t(mapping), want_pred=True)
    emat, epred = FO.frame_confusion(x, store, picked, mapping=mapping)
    assert np.array_equal(mat.cpu().numpy(), emat) and np.array_equal(pred.cpu().numpy(), epred)


@pytest.mark.parametrize('layout', ['nchw', 'cl'])
def test_predictions_only(layout):
    import mvpnet_amd.ops as ops
    x = logits_for(3, 20, 9, 31, 4)
    pred = ops.frame_confusion(laid_out(x, layout), None, None)
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), FO.first_argmax(x))
    assert torch.equal(pred, laid_out(x, layout).argmax(1))


@pytest.mark.parametrize('layout', ['nchw', 'cl'])
def test_frame_confusion_equals_the_reference_evaluator(golden, layout):
    import mvpnet_amd.ops as ops
    mat = ops.frame_confusion(laid_out(golden['logit'], layout), t(golden['labels']), t(golden['picked']), size=FO.FIX_SIZE, mapping=t(golden['mapping']))
    assert np.array_equal(mat.cpu().numpy(), golden['confusion'].astype(np.int64))


def test_frame_confusion_refuses():
    import mvpnet_amd.ops as ops
    labels, picked = torch.zeros((2, 8, 8), dtype=torch.uint16, device=DEV), torch.zeros((1,), dtype=torch.int64, device=DEV)
    logit = torch.zeros((1, 3, 8, 8), device=DEV)
    for bad in (lambda: ops.frame_confusion(logit, labels, picked, size=(4, 4)),                      # the logits are 8 x 8
                lambda: ops.frame_confusion(logit[:, :, :4], labels, picked),                        # ... or not the store's size
                lambda: ops.frame_confusion(logit, labels, torch.zeros((2,), dtype=torch.int64, device=DEV)),
                lambda: ops.frame_confusion(logit.double(), labels, picked),
                lambda: ops.frame_confusion(logit, labels, picked, out=torch.zeros((4, 4), dtype=torch.int64, device=DEV)),
                lambda: ops.label_histogram(labels, 0), lambda: ops.label_histogram(labels, 65537),
                lambda: ops.label_histogram(torch.zeros(4, dtype=torch.int64, device=DEV), 20, size=(4, 4))):
        with pytest.raises(RuntimeError):
            bad()


# ---- label_histogram -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(7, 5), None])
@pytest.mark.parametrize('mapped', [False, True])
@pytest.mark.parametrize('num_bins', [20, 41, 65536])
def test_label_histogram_of_frames(store, num_bins, mapped, size):
    """LDS counters (20, 41) and global atomics (65536: every raw id); all frames, then picked ones added to the same counts"""
    import mvpnet_amd.ops as ops
    labels = store.copy()
    labels[0, 0, :3] = (65535, 4096, 0)
    mapping = FO.fixture_inputs()['mapping'] if mapped else None
    hist = ops.label_histogram(t(labels), num_bins, size=size, mapping=None if mapping is None else t(mapping))
    ehist = FO.label_histogram(labels, num_bins, size=size, mapping=mapping)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (num_bins,) and np.array_equal(hist.cpu().numpy(), ehist) and int(ehist.sum()) > 0
    picked = np.array([4, 0, 0, 2, 7], np.int64)
    again = ops.label_histogram(t(labels), num_bins, picked=t(picked), size=size, mapping=None if mapping is None else t(mapping), out=hist)
    assert again is hist
    assert np.array_equal(hist.cpu().numpy(), FO.label_histogram(labels, num_bins, picked=picked, size=size, mapping=mapping, out=ehist))
    if num_bins == 65536 and not mapped and size is None:
        assert int(ehist[65535]) == 1 and int(ehist[4096]) == 1


def test_label_histogram_many_frames(store):
    """2000 frames: one workgroup per frame, a strided walk"""
    import mvpnet_amd.ops as ops
    picked = np.arange(2000, dtype=np.int64) % 5
    hist = ops.label_histogram(t(store), 41, picked=t(picked))
    assert np.array_equal(hist.cpu().numpy(), 400 * FO.label_histogram(store, 41))


@pytest.mark.parametrize('num_bins', [41, 5000])
def test_label_histogram_of_int64_labels(num_bins):
    """negatives and values >= num_bins count nowhere; two calls accumulate; n = 0 launches nothing; more than one workgroup's worth"""
    import mvpnet_amd.ops as ops
    rs = np.random.RandomState(num_bins)
    a, b = rs.randint(-5, num_bins + 7, 100003).astype(np.int64), rs.randint(0, num_bins, (3, 11)).astype(np.int64)
    a[::5] = -100
    hist = ops.label_histogram(t(a), num_bins)
    assert np.array_equal(hist.cpu().numpy(), FO.label_histogram(a, num_bins))
    ops.label_histogram(t(b), num_bins, out=hist)
    ops.label_histogram(torch.zeros((0,), dtype=torch.int64, device=DEV), num_bins, out=hist)
    assert np.array_equal(hist.cpu().numpy(), FO.label_histogram(b, num_bins, out=FO.label_histogram(a, num_bins)))


# ---- the class weights ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    assert a.dtype == np.float32
    return a.view(np.uint32)


def test_label_weights_equal_the_fixture(golden):
    from mvpnet_amd import scene as SC
    labels, mapping = t(golden['labels']), t(golden['mapping'])
    w2 = SC.label_weights_2d({'labels': labels}, resize=FO.FIX_SIZE, label_mapping=mapping)
    assert isinstance(w2, np.ndarray) and np.array_equal(bits(w2), bits(golden['weights_2d']))
    every = SC.label_weights_2d({'labels': labels}, torch.arange(0, 5, 1, device=DEV), resize=FO.FIX_SIZE, label_mapping=mapping, num_classes=20)
    assert np.array_equal(bits(every), bits(golden['weights_2d']))
    some = SC.label_weights_2d({'labels': labels}, torch.arange(0, 5, 2, device=DEV), resize=FO.FIX_SIZE, label_mapping=mapping)
    esome = FO.label_log_weights(FO.label_histogram(golden['labels'], 20, picked=[0, 2, 4], size=FO.FIX_SIZE, mapping=golden['mapping']))
    assert np.array_equal(bits(some), bits(esome)) and not np.array_equal(bits(some), bits(w2))
    flat, off = golden['seg_label_3d'], golden['scene_offsets_3d']
    w3 = SC.label_weights_3d(t(flat))
    assert np.array_equal(bits(w3), bits(golden['weights_3d']))
    per_scene = SC.label_weights_3d([t(flat[a:b]) for a, b in zip(off[:-1], off[1:])], num_labels=41, class_ids=FO.EVAL_CLASS_IDS)
    assert np.array_equal(bits(per_scene), bits(golden['weights_3d']))


# ---- test_frames_2d and validate_2d --------------------------------------------------------------------------------------------------------
class PointwiseNet(nn.Module):
    """a stand-in 2D network behind the {'image'} -> {'seg_logit'} interface"""

    def __init__(self, C):
        super().__init__()
        torch.manual_seed(3)
        self.conv = nn.Conv2d(3, C, 1)

    def forward(self, batch):
        return {'seg_logit': self.conv(batch['image'])}


def frames_store(frames=7, H=48, W=64):
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = np.stack([(yy * 5 + xx * f) % 256 for f in (1, 2, 3)], axis=-1)
    images = np.clip(smooth[None] + rs.randint(-40, 41, (frames, H, W, 3)), 0, 255).astype(np.uint8)
    labels = rs.randint(0, 45, (frames, H, W)).astype(np.uint16)
    return {'images': t(images), 'labels': t(labels)}, t(FO.fixture_inputs()['mapping'])


def host_pieces(model, store, batches, **kw):
    """what the project offered before: sample_train_batch_2d without an augmentation -> model -> argmax(1) -> metric.Evaluator on the host"""
    from mvpnet_amd import metric as M
    from mvpnet_amd import scene as SC
    ev, preds = M.Evaluator(M.CLASS_NAMES), []
    model.eval()
    with torch.no_grad():
        for picked in batches:
            batch = SC.sample_train_batch_2d(store, picked, **kw)
            pred = model(batch)['seg_logit'].argmax(1)
            ev.batch_update(pred.cpu().numpy(), batch['seg_label'].cpu().numpy())
            preds.append(pred)
    return ev, torch.cat(preds)


@pytest.mark.parametrize('resize', [(16, 12), None])
@pytest.mark.parametrize('channels_last', [False, True])
def test_test_frames_2d(resize, channels_last):
    """7 frames of 48 x 64 in batches of 3 (the last one partial): the matrix is metric.Evaluator's over the same batches, the predictions
    are argmax(1)'s, and the loop synchronises nothing"""
    from mvpnet_amd import metric as M
    from mvpnet_amd import mvpnet2d as M2
    store, mapping = frames_store()
    model = PointwiseNet(20).to(DEV)
    kw = dict(resize=resize, image_normalizer=NORMALIZER, label_mapping=mapping, channels_last=channels_last)
    M2.test_frames_2d(model, store, batch_size=3, **kw)  # (the tables and the normaliser's 6 floats exist from here on)
    frames = torch.arange(7, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ev, pred = M2.test_frames_2d(model, store, frames, batch_size=3, want_pred=True, **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert isinstance(ev, M.DeviceEvaluator) and ev.class_names == tuple(M.CLASS_NAMES)
    eev, epred = host_pieces(model, store, [frames[0:3], frames[3:6], frames[6:7]], **kw)
    assert np.array_equal(ev.confusion_matrix, eev.confusion_matrix) and eev.confusion_matrix.sum() > 300  # (20 of 45 ids are classes: ~600 of 1344)
    assert torch.equal(pred, epred) and tuple(pred.shape) == ((7, 12, 16) if resize else (7, 48, 64))
    assert ev.overall_acc == eev.overall_acc and ev.overall_iou == eev.overall_iou
    # frames=None is every frame; an evaluator that is passed in is added to
    same = M2.test_frames_2d(model, store, batch_size=3, evaluator=ev, **kw)
    assert same is ev and np.array_equal(ev.confusion_matrix, 2 * eev.confusion_matrix)
    # an unlabelled split: predictions only
    none, only = M2.test_frames_2d(model, {'images': store['images']}, frames, batch_size=3, resize=resize, image_normalizer=NORMALIZER,
                                   channels_last=channels_last)
    assert none is None and torch.equal(only, epred)
    # an evaluator of raw ids, or of another class count, is refused
    with pytest.raises(ValueError):
        M2.test_frames_2d(model, store, batch_size=3, evaluator=M.DeviceEvaluator(M.CLASS_NAMES, M.EVAL_CLASS_IDS), **kw)
    with pytest.raises(ValueError):
        M2.test_frames_2d(PointwiseNet(5).to(DEV), store, batch_size=3, **kw)


def test_test_frames_2d_with_the_real_network():
    """config.build_model_sem_seg_2d at 2 frames of 64 x 64, channels-last: the network's own output layout goes through"""
    from mvpnet_amd import config as C
    from mvpnet_amd import mvpnet2d as M2
    with open(os.path.join(GOLDEN, 'configs_2d.json')) as f:
        cfg = C.load_cfg(text=yaml.safe_dump(json.load(f)['unet_resnet34']))
    torch.manual_seed(11)
    model = C.build_model_sem_seg_2d(cfg).to(DEV).to(memory_format=torch.channels_last)
    store, mapping = frames_store(2, 64, 64)
    kw = dict(image_normalizer=NORMALIZER, label_mapping=mapping, channels_last=True)
    ev, pred = M2.test_frames_2d(model, store, batch_size=2, want_pred=True, **kw)
    assert model.training  # (the mode is restored)
    eev, epred = host_pieces(model, store, [torch.arange(2, dtype=torch.int64, device=DEV)], **kw)
    assert torch.equal(pred, epred) and np.array_equal(ev.confusion_matrix, eev.confusion_matrix) and eev.confusion_matrix.sum() > 1000


@pytest.mark.parametrize('resize', [(16, 12), None])
def test_validate_2d(resize):
    """the loss is the mean of SegLoss over the same batches, bit for bit; the summary is what SegAccuracy and SegIoU report"""
    from mvpnet_amd import metric as M
    from mvpnet_amd import mvpnet2d as M2
    from mvpnet_amd import scene as SC
    from mvpnet_amd.mvpnet3d import SegLoss
    store, mapping = frames_store()
    model = PointwiseNet(20).to(DEV)
    loss_fn = SegLoss(weight=t(M.label_log_weights(np.arange(1, 21))))
    frames = t(np.array([6, 0, 1, 5, 5, 2, 3], np.int64))
    kw = dict(resize=resize, image_normalizer=NORMALIZER, label_mapping=mapping)
    model.train()
    M2.validate_2d(model, loss_fn, store, frames, batch_size=3, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = M2.validate_2d(model, loss_fn, store, frames, batch_size=3, **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert model.training and sorted(out) == ['confusion', 'loss']
    assert out['loss'].is_cuda and out['loss'].dim() == 0 and out['confusion'].is_cuda and out['confusion'].dtype == torch.int64
    acc, iou, losses = M.SegAccuracy(), M.SegIoU(20), []
    model.eval()
    with torch.no_grad():
        for part in (frames[0:3], frames[3:6], frames[6:7]):
            batch = SC.sample_train_batch_2d(store, part, **kw)
            preds = model(batch)
            losses.append(loss_fn(preds, batch)['seg_loss'])
            acc.update_dict(preds, batch)
            iou.update_dict(preds, batch)
    eloss = torch.stack(losses).mean()
    assert torch.equal(out['loss'].view(1).view(torch.int32), eloss.view(1).view(torch.int32)) and bool(torch.isfinite(eloss))
    assert torch.equal(out['confusion'], iou.mat) and int(iou.mat.sum()) > 300
    summary = M.summary_from_confusion(out['confusion'])
    assert summary == {'seg_acc': acc.global_avg, 'seg_iou': iou.global_avg}
    # the fused kernel counts what the validation's two launches count
    ev = M2.test_frames_2d(model, store, frames, batch_size=3, **kw)
    assert np.array_equal(ev.confusion_matrix, out['confusion'].cpu().numpy().astype(np.float64))

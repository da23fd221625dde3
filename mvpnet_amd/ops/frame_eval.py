"""What surrounds stage one, on the device (new: mvpnet/test_2d.py:103-118 and the validation pass of mvpnet/train_2d.py:240-312 copy
labels and predictions to the host per batch; mvpnet/data/preprocess/compute_label_weights.py counts labels in a host loop): the raw
16-bit label frames go through Pillow's NEAREST indices and the label mapping straight into integer counts."""
import torch

from .. import _lib as L
from .resize import _nearest_on, _size

MAX_BINS = L.LIMITS['MVP_HISTOGRAM_MAX_BINS']

_ALL = {}  # (device, Ftot) -> arange(Ftot) int64 on the device, for picked=None


def _check_store(who, labels, picked, mapping):
    if labels.dim() != 3 or labels.dtype != torch.uint16 or labels.size(0) < 1 or labels.size(1) < 1 or labels.size(2) < 1:
        raise RuntimeError(who + ': labels must be (Ftot,H,W) uint16 with Ftot, H, W >= 1')
    dev = labels.device
    if picked.dtype != torch.int64 or picked.device != dev:
        raise RuntimeError(who + ': picked must be int64 on the labels\' device')
    if mapping is not None and (mapping.dtype != torch.int64 or mapping.dim() != 1 or mapping.device != dev):
        raise RuntimeError(who + ': mapping must be (T,) int64 on the labels\' device')


def frame_confusion(logit, labels, picked, *, size=None, mapping=None, ignore_value=-100, out=None, want_pred=False):
    """(C,C) int64 matrix [label][argmax logit] of a batch of frames against the store's label images, one launch, no label tensor and no
    host synchronisation: what ops.prepare_labels + metric.confusion_matrix give in two launches with an (Nf,h,w) int64 tensor between.
    logit (Nf,C,h,w) float32 on the device in ANY strides (contiguous, channels-last, a view with a padded batch stride: no copy).
    labels (Ftot,H,W) uint16, picked (any shape, Nf elements) int64, mapping (T,) int64 or None, ignore_value: as ops.prepare_labels.
    size: PIL's (w, h), which must be the logits' -- None says the logits have the store's size.  A pixel counts when its mapped label
    lies in [0,C); the first maximum wins (torch.argmax's rule; NaN logits are outside the contract).
    out: a running (C,C) int64 matrix that is added to.  -> the matrix, or (matrix, pred) with want_pred: pred (Nf,h,w) int64, the argmax
    of every pixel.  labels=None (an unlabelled split): -> pred alone; picked, size and mapping are not used.
    Definition: include/mvp_hip.h, mvp_frame_confusion_f32."""
    L.require_gpu(labels, picked, mapping, out)
    if not torch.is_tensor(logit) or not logit.is_cuda:
        raise RuntimeError('frame_confusion: logit must be a tensor on the GPU; there is no CPU fallback')
    if logit.dim() != 4 or logit.dtype != torch.float32 or min(logit.shape) < 1:
        raise RuntimeError('frame_confusion: logit must be (Nf,C,h,w) float32, every size >= 1')
    Nf, C, h, w = logit.shape
    dev = logit.device
    if C >= 2 ** 16 or h * w >= 2 ** 31:
        raise RuntimeError('frame_confusion: needs C < 2^16 and h*w < 2^31')
    pred = torch.empty((Nf, h, w), dtype=torch.int64, device=dev) if (want_pred or labels is None) else None
    strides = tuple(logit.stride())
    if labels is None:
        L.call('mvp_frame_confusion_f32', logit, L.ptr(logit), Nf, C, h, w, *strides, None, 1, h, w, None, None, None, None, 0, int(ignore_value),
               None, L.ptr(pred))
        return pred
    _check_store('frame_confusion', labels, picked, mapping)
    if labels.device != dev or picked.numel() != Nf:
        raise RuntimeError('frame_confusion: labels must be on the logits\' device and picked must name one frame per logit frame')
    Ftot, H, W = labels.shape
    if _size('frame_confusion', size, H, W) != (h, w):
        raise RuntimeError('frame_confusion: the logits are {}x{} (h x w) but size asks for {}x{}'.format(h, w, *_size('frame_confusion', size, H, W)))
    if H * W >= 2 ** 31:
        raise RuntimeError('frame_confusion: a label image must stay below 2^31 pixels')
    if out is None:
        out = torch.zeros((C, C), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or tuple(out.shape) != (C, C) or out.device != dev:
        raise RuntimeError('frame_confusion: out must be (C,C) int64 on the logits\' device')
    L.call('mvp_frame_confusion_f32', logit, L.ptr(logit), Nf, C, h, w, *strides, L.ptr(labels), Ftot, H, W, L.ptr(picked),
           L.ptr(_nearest_on(dev, H, h)), L.ptr(_nearest_on(dev, W, w)), L.ptr(mapping), 0 if mapping is None else mapping.numel(),
           int(ignore_value), L.ptr(out), L.ptr(pred))
    return (out, pred) if want_pred else out


def label_histogram(labels, num_bins, *, picked=None, size=None, mapping=None, out=None):
    """(num_bins,) int64 counts of label values, one launch, no host synchronisation (torch.bincount reads its maximum back): the
    np.bincount of compute_label_weights.py, added to `out` when given.  Values outside [0,num_bins) -- -100, a raw id past the mapping --
    count nowhere.  1 <= num_bins <= 65536.
    labels (Ftot,H,W) uint16 on the device, a store of raw label frames: picked (any shape) int64 rows or None for all frames, size =
    PIL's (w, h) or None, mapping (T,) int64 or None for the raw ids, as ops.prepare_labels -- the frames are read through Pillow's
    NEAREST indices and the mapping and counted; no label tensor is made.
    labels int64 of any shape, contiguous, on the device (the 3D store's seg_label): counted as they are; picked, size, mapping must be None.
    Definition: include/mvp_hip.h, mvp_label_histogram_u16 / mvp_label_histogram_i64."""
    L.require_gpu(labels, picked, mapping, out)
    num_bins = int(num_bins)
    if not 1 <= num_bins <= MAX_BINS:
        raise RuntimeError('label_histogram: needs 1 <= num_bins <= {}'.format(MAX_BINS))
    dev = labels.device
    if out is None:
        out = torch.zeros((num_bins,), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or tuple(out.shape) != (num_bins,) or out.device != dev:
        raise RuntimeError('label_histogram: out must be (num_bins,) int64 on the labels\' device')
    if labels.dtype == torch.int64:
        if picked is not None or size is not None or mapping is not None:
            raise RuntimeError('label_histogram: picked, size and mapping go with a uint16 frame store, not with int64 labels')
        if labels.numel():
            L.call('mvp_label_histogram_i64', labels, L.ptr(labels), labels.numel(), num_bins, L.ptr(out))
        return out
    if picked is None:
        if labels.dim() != 3 or labels.size(0) < 1:
            raise RuntimeError('label_histogram: labels must be (Ftot,H,W) uint16 with Ftot, H, W >= 1, or int64')
        picked = _ALL.get((dev, labels.size(0)))
        if picked is None:
            picked = _ALL[(dev, labels.size(0))] = torch.arange(labels.size(0), dtype=torch.int64, device=dev)
    _check_store('label_histogram', labels, picked, mapping)
    Ftot, H, W = labels.shape
    h, w = _size('label_histogram', size, H, W)
    if H * W >= 2 ** 31 or h * w >= 2 ** 31:
        raise RuntimeError('label_histogram: a label image must stay below 2^31 pixels')
    if picked.numel():
        L.call('mvp_label_histogram_u16', labels, L.ptr(labels), Ftot, H, W, L.ptr(picked), picked.numel(), h, w, L.ptr(_nearest_on(dev, H, h)),
               L.ptr(_nearest_on(dev, W, w)), L.ptr(mapping), 0 if mapping is None else mapping.numel(), num_bins, L.ptr(out))
    return out

"""What the reference's test scripts do behind a scene's logits, on the device (new: mvpnet/ensemble.py:45-49 sums scipy softmaxes of
four models' saved logits on the host; mvpnet/evaluate_3d.py:25-40 calls sklearn's confusion_matrix on host label arrays)."""
import ctypes

import torch

from .. import _lib as L

MAX_MODELS = L.LIMITS['MVP_ENSEMBLE_MAX_MODELS']
MAX_CLASSES = 64
MAX_CONFUSION_CLASSES = L.LIMITS['MVP_CONFUSION_MAX_CLASSES']


def ensemble_softmax(logits, want_prob=True):
    """sum over models of softmax(logits[m], dim=1), and its argmax, one launch.  logits: a list of 1..8 float32 tensors of one shape (n,C),
    C <= 64, on one device, in ANY strides -- (n,C) rows, the transposed view of a (C,n) network output, rows with a padded stride --; the
    kernel reads all of them with the first one's strides, a tensor whose strides differ is copied into them first (only then).
    -> (prob (n,C) float32 or None when not want_prob, label (n,) int64: the first maximum, 0 for a row with a NaN).
    Definition (pinned): include/mvp_hip.h, mvp_ensemble_softmax_f32."""
    logits = list(logits)
    if not 1 <= len(logits) <= MAX_MODELS:
        raise RuntimeError('ensemble_softmax: needs 1 to {} models, got {}'.format(MAX_MODELS, len(logits)))
    first = logits[0]
    for t in logits:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError('ensemble_softmax: logits must be tensors on the GPU; there is no CPU fallback')
        if t.dim() != 2 or t.dtype != torch.float32 or t.shape != first.shape or t.device != first.device:
            raise RuntimeError('ensemble_softmax: logits must be float32 tensors of one shape (n,C) on one device')
    n, C = first.shape
    if not 1 <= C <= MAX_CLASSES or n >= 2 ** 31:
        raise RuntimeError('ensemble_softmax: needs 1 <= C <= {} and n < 2^31'.format(MAX_CLASSES))
    same = []
    for t in logits:
        if t.stride() != first.stride():
            t = torch.empty_strided(first.shape, first.stride(), dtype=torch.float32, device=first.device).copy_(t)
        same.append(t)
    prob = torch.empty((n, C), dtype=torch.float32, device=first.device) if want_prob else None
    label = torch.empty((n,), dtype=torch.int64, device=first.device)
    if n:
        table = (ctypes.c_void_p * len(same))(*[t.data_ptr() for t in same])  # on the host: the kernel takes the pointers by value
        L.call('mvp_ensemble_softmax_f32', first, table, len(same), n, C, first.stride(0), first.stride(1), L.ptr(prob), L.ptr(label))
    return prob, label


def label_confusion(pred, gt, mat, pred_lut=None, gt_lut=None):
    """mat (C,C) int64 += 1 at [position(gt)][position(pred)] over the points where both are labels, one launch.  pred, gt (n,) int64 on
    mat's device; pred_lut, gt_lut: int32 tables value -> position (-1: not a label) or None (the value is the position when it lies in
    [0,C)).  -> mat.  Definition (pinned): include/mvp_hip.h, mvp_label_confusion_i64."""
    L.require_gpu(pred, gt, mat, pred_lut, gt_lut)
    if pred.dtype != torch.int64 or gt.dtype != torch.int64 or pred.dim() != 1 or gt.shape != pred.shape:
        raise RuntimeError('label_confusion: pred and gt must be (n,) int64')
    if mat.dtype != torch.int64 or mat.dim() != 2 or mat.size(0) != mat.size(1) or not 1 <= mat.size(0) <= MAX_CONFUSION_CLASSES:
        raise RuntimeError('label_confusion: mat must be (C,C) int64, 1 <= C <= {}'.format(MAX_CONFUSION_CLASSES))
    for lut in (pred_lut, gt_lut):
        if lut is not None and (lut.dtype != torch.int32 or lut.dim() != 1 or lut.numel() < 1):
            raise RuntimeError('label_confusion: a table must be (L,) int32, L >= 1')
    if any(t is not None and t.device != mat.device for t in (pred, gt, pred_lut, gt_lut)):
        raise RuntimeError('label_confusion: all tensors must be on one device')
    L.call('mvp_label_confusion_i64', mat, L.ptr(pred), L.ptr(gt), pred.numel(), mat.size(0), L.ptr(pred_lut),
           0 if pred_lut is None else pred_lut.numel(), L.ptr(gt_lut), 0 if gt_lut is None else gt_lut.numel(), L.ptr(mat))
    return mat

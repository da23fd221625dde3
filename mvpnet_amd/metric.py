"""Segmentation meters and the whole-scene evaluator matrices.

  SegAccuracy, SegIoU           mvpnet/models/metric.py:5-73   (same names, `update_dict` contract, strings)
  Evaluator, CLASS_NAMES, ...   mvpnet/evaluate_3d.py:4-92     (confusion matrix + accuracy / IoU numbers only)
  DeviceEvaluator               the same for label tensors on the device (mvp_label_confusion_i64; nothing is read back until a number is)
                                + update_frames: the 2D network's logits against raw label frames (mvp_frame_confusion_f32), mvpnet/test_2d.py
  DeviceMeters, MeterSnapshot   SegAccuracy + SegIoU + the loss meter of a loop with their state on the device, updated by the loss launch
                                (mvp_seg_loss_meter_f32 through SegLoss(meters=)); no read-back until a number is wanted
  label_log_weights             mvpnet/data/preprocess/compute_label_weights.py (the arithmetic behind the class weights)

MI355X side: for fp32 logits on the GPU both meters get `argmax -> mask by ignore_index -> bincount` from ONE pass of
`mvp_seg_confusion_f32` over the logits where the network left them ((B,C,N) or channels-last rows); the reference runs
argmax, two boolean-mask compactions, `eq`, `bincount` and a reshape as separate ATen kernels, twice.  The running
confusion matrix of SegIoU stays on the device; nothing is synchronised until a value is read.  Host tensors take the
torch path (the reference's own arithmetic).

The generic host utilities of the reference (`common/utils/metric_logger.py`: AverageMeter, MetricLogger; the evaluator's
table printing) are OUT OF SCOPE and not re-implemented: the reference's own `MetricLogger.add_meter(s)` accepts the two
meters below as they are (they expose `name`, `update_dict`, `__str__`, `summary_str`, `reset`, `avg`, `global_avg`).
Pinned against the imported reference classes by tests/golden/metrics.npz."""
import weakref

import numpy as np
import torch

from . import _lib as L


def confusion_matrix(seg_logit, seg_label, num_classes=None, ignore_index=-100, out=None):
    """(C,C) int64 matrix [label][argmax logit] over the points whose label is not ignore_index, added to `out` if given.
    seg_logit (B,C,N) in any strides that keep (b,c,n) addressable (e.g. the transposed view of channels-last rows), or the 2D stage's
    (B,C,H,W) with seg_label (B,H,W): viewed as (B,C,H*W), without a copy for contiguous and channels-last memory."""
    if seg_logit.dim() == 4:
        seg_logit, seg_label = seg_logit.flatten(2), seg_label.reshape(seg_label.size(0), -1)
    B, C, N = seg_logit.shape
    n = C if num_classes is None else num_classes
    mat = out if out is not None else torch.zeros((n, n), dtype=torch.int64, device=seg_logit.device)
    if seg_logit.is_cuda and seg_logit.dtype == torch.float32 and n == C:
        label = seg_label.contiguous()
        sb, sc, sn = seg_logit.stride()
        L.call('mvp_seg_confusion_f32', seg_logit, L.ptr(seg_logit), B, C, N, sb, sc, sn, L.ptr(label), int(ignore_index), L.ptr(mat))
        return mat
    pred = seg_logit.argmax(1)
    keep = seg_label != ignore_index
    mat += torch.bincount(n * seg_label[keep] + pred[keep], minlength=n * n).reshape(n, n)
    return mat


class SegAccuracy(object):
    """Fraction of non-ignored points whose argmax equals the label (metric.py:5-24): printed as
    `<mean over the last 20 updates> (<mean over all updates>)`, both weighted by the number of valid points."""
    name = 'seg_acc'
    WINDOW = 20

    def __init__(self, ignore_index=-100):
        self.ignore_index = ignore_index
        self.reset()

    def reset(self):
        self.recent = []          # (correct, valid) of the last WINDOW updates
        self.sum, self.count = 0.0, 0

    def update_dict(self, preds, labels):
        with torch.no_grad():
            mat = confusion_matrix(preds['seg_logit'], labels['seg_label'], ignore_index=self.ignore_index)
            correct, valid = torch.stack([mat.diagonal().sum(), mat.sum()]).tolist()  # ONE device->host copy
        self.recent = (self.recent + [(correct, valid)])[-self.WINDOW:]
        self.sum += correct
        self.count += valid

    @property
    def avg(self):
        hit = sum(c for c, _ in self.recent)
        tot = sum(v for _, v in self.recent)
        return hit / tot if tot else float('nan')

    @property
    def global_avg(self):
        return self.sum / self.count if self.count else float('nan')

    def __str__(self):
        return '{:.4f} ({:.4f})'.format(self.avg, self.global_avg)

    @property
    def summary_str(self):
        return '{:.4f}'.format(self.global_avg)


class SegIoU(object):
    """Running confusion matrix and per-class IoU = tp / (gt + pred - tp) (metric.py:26-73)."""
    name = 'seg_iou'

    def __init__(self, num_classes, ignore_index=-100):
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.mat = None

    def update_dict(self, preds, labels):
        with torch.no_grad():
            if self.mat is None:
                self.mat = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=preds['seg_logit'].device)
            confusion_matrix(preds['seg_logit'], labels['seg_label'], self.num_classes, self.ignore_index, out=self.mat)

    def reset(self):
        self.mat = None

    @property
    def iou(self):
        h = self.mat.float()
        tp = torch.diag(h)
        return tp / (h.sum(1) + h.sum(0) - tp)

    @property
    def global_avg(self):
        return self.iou.mean().item()

    def __str__(self):
        return '{iou:.4f}'.format(iou=self.iou.mean().item())

    @property
    def summary_str(self):
        return str(self)


# ScanNet v2 benchmark classes (evaluate_3d.py:4-9)
CLASS_NAMES = ['wall', 'floor', 'cabinet', 'bed', 'chair', 'sofa', 'table', 'door',
               'window', 'bookshelf', 'picture', 'counter', 'desk', 'curtain',
               'refridgerator', 'showercurtain', 'toilet', 'sink', 'bathtub', 'otherfurniture']
EVAL_CLASS_IDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]


class Evaluator(object):
    """Whole-scene confusion matrix on host label arrays and the numbers derived from it (evaluate_3d.py:11-92).
    A (gt, pred) pair counts when BOTH sides are one of `labels` -- what sklearn's confusion_matrix(gt, pred, labels=...)
    keeps: ignored ground truth and the "unlabelled" prediction (num_classes) drop out.  The caller's arrays are not
    modified.  The reference's table printing (tabulate) is host formatting and is not part of this build."""

    def __init__(self, class_names, labels=None):
        self.class_names = tuple(class_names)
        self.num_classes = n = len(self.class_names)
        self.labels = np.arange(n) if labels is None else np.asarray(labels)
        if self.labels.shape != (n,):
            raise ValueError('one label id per class expected')
        self._order = np.argsort(self.labels, kind='stable')
        self._sorted = self.labels[self._order]
        self.confusion_matrix = np.zeros((n, n))

    def _position(self, values):
        """index into `labels` of every value, -1 where the value is not a label"""
        v = np.asarray(values).reshape(-1)
        at = np.clip(np.searchsorted(self._sorted, v), 0, self.num_classes - 1)
        return np.where(self._sorted[at] == v, self._order[at], -1)

    def update(self, pred_label, gt_label):
        gt = np.asarray(gt_label).reshape(-1)
        if not (gt >= 0).any():
            print('Invalid label.')
            return
        row, col = self._position(gt), self._position(pred_label)
        both = (row >= 0) & (col >= 0)
        n = self.num_classes
        self.confusion_matrix += np.bincount(row[both] * n + col[both], minlength=n * n).reshape(n, n)

    def batch_update(self, pred_labels, gt_labels):
        if len(pred_labels) != len(gt_labels):
            raise ValueError('one prediction array per ground-truth array expected')
        for p, g in zip(pred_labels, gt_labels):
            self.update(p, g)

    @property
    def overall_acc(self):
        cm = self.confusion_matrix
        return np.trace(cm) / cm.sum()

    @property
    def class_seg_acc(self):
        cm = self.confusion_matrix
        with np.errstate(invalid='ignore', divide='ignore'):
            return list(np.diag(cm) / cm.sum(1))

    @property
    def class_iou(self):
        cm = self.confusion_matrix
        tp = np.diag(cm)
        union = cm.sum(0) + cm.sum(1) - tp
        with np.errstate(invalid='ignore', divide='ignore'):
            return list(np.where(union == 0, np.nan, tp / union))

    @property
    def overall_iou(self):
        return np.nanmean(self.class_iou)


class DeviceEvaluator(object):
    """Evaluator for label tensors that are on the device already (the four whole-scene test paths of mvpnet_amd.scene and
    scene.ensemble_scene end there): the same interface and numbers, with the confusion matrix kept on the device.  `update` only
    launches (ops.label_confusion: mvp_label_confusion_i64 through two value -> position tables built once here); nothing is copied or
    synchronised until a number -- or `confusion_matrix` -- is read, and that read is the only synchronisation.
    `labels` must be non-negative integers (raw ids index the tables), one per class.  For such labels the reference's early return on
    a scene whose ground truth is all negative (evaluate_3d.py:29-31) adds nothing to the matrix -- a negative value is no label -- and
    neither does the kernel: there is no such test here, and no 'Invalid label.' print.  Ignored ground truth (-100), raw ids that are
    no evaluation class and the "no prediction" label (num_classes, when it is not itself one of `labels`) drop out, as in Evaluator.
    Host arrays are refused: Evaluator exists for them."""

    def __init__(self, class_names, labels=None):
        self.class_names = tuple(class_names)
        self.num_classes = n = len(self.class_names)
        labels = np.arange(n) if labels is None else np.asarray(labels)
        if labels.shape != (n,):
            raise ValueError('one label id per class expected')
        if not np.issubdtype(labels.dtype, np.integer) or (labels < 0).any():
            raise ValueError('DeviceEvaluator: labels must be non-negative integers')
        self.labels = labels
        lut = np.full(int(labels.max()) + 1 if n else 1, -1, np.int32)
        for pos in range(n - 1, -1, -1):  # (a repeated id keeps its first position, as Evaluator's stable sort does)
            lut[labels[pos]] = pos
        self._host_lut = torch.from_numpy(lut)
        self._lut = self._mat = None

    def update(self, pred_label, gt_label):
        from . import ops
        for t in (pred_label, gt_label):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError('DeviceEvaluator.update takes tensors on the GPU; use metric.Evaluator for host arrays')
        if self._lut is None:
            self._lut = self._host_lut.to(pred_label.device)
        if self._mat is None:
            self._mat = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=pred_label.device)
        pred, gt = pred_label.reshape(-1).long().contiguous(), gt_label.reshape(-1).long().contiguous()
        ops.label_confusion(pred, gt, self._mat, pred_lut=self._lut, gt_lut=self._lut)

    def batch_update(self, pred_labels, gt_labels):
        if len(pred_labels) != len(gt_labels):
            raise ValueError('one prediction array per ground-truth array expected')
        for p, g in zip(pred_labels, gt_labels):
            self.update(p, g)

    def update_frames(self, seg_logit, labels, picked, *, size=None, mapping=None, want_pred=False):
        """A batch of the 2D network's logits (Nf,C,h,w) against the frame store's raw label images, added to the running matrix: what
        mvpnet/test_2d.py:113-118 does with `argmax(1).cpu().numpy()` and `batch_update` on host arrays.  Only launches
        ops.frame_confusion (mvp_frame_confusion_f32: label read, mapping, argmax and count in one kernel); labels (Ftot,H,W) uint16,
        picked, size, mapping as there.  Allowed when this evaluator's labels are arange(C), the `Evaluator(class_names)` of test_2d.py,
        with C the logits' channel count: the class index is the position, so no table is needed; ValueError otherwise.
        want_pred: -> the (Nf,h,w) int64 argmax of every pixel, written by the same launch."""
        from . import ops
        n = self.num_classes
        if not np.array_equal(self.labels, np.arange(n)) or seg_logit.size(1) != n:
            raise ValueError('DeviceEvaluator.update_frames: needs labels == arange(C) and C == seg_logit.size(1)')
        if self._mat is None:  # (no table here: nothing is copied to the device)
            self._mat = torch.zeros((n, n), dtype=torch.int64, device=seg_logit.device)
        out = ops.frame_confusion(seg_logit, labels, picked, size=size, mapping=mapping, out=self._mat, want_pred=want_pred)
        return out[1] if want_pred else None

    @property
    def confusion_matrix(self):
        """(C,C) float64 NumPy array, as Evaluator's (the read: one device-to-host copy)."""
        n = self.num_classes
        return np.zeros((n, n)) if self._mat is None else self._mat.cpu().numpy().astype(np.float64)

    overall_acc = Evaluator.overall_acc
    class_seg_acc = Evaluator.class_seg_acc
    class_iou = Evaluator.class_iou
    overall_iou = Evaluator.overall_iou


MAX_WINDOW = L.LIMITS['MVP_SEG_METER_MAX_WINDOW']


def meter_state_sizes(num_classes, window):
    """(int64 words, float64 words) of the meter state of mvp_seg_loss_meter_f32 (MVP_SEG_METER_I64 / _F64 of include/mvp_hip.h)."""
    return 4 + 2 * (window + 1) + num_classes * num_classes, 1 + window


class MeterSnapshot(object):
    """The meter state of mvp_seg_loss_meter_f32 on the host, and every number the three meters report, as plain Python values: the
    arithmetic behind DeviceMeters.read().  state_i64 / state_f64: the two state arrays (NumPy, the layout of include/mvp_hip.h).
      updates                        u
      correct, valid                 cumulative counts       window_correct, window_valid   of the last min(u, window) updates
      mat                            (C,C) int64 [label][argmax]
      loss_sum                       sum of the per-update losses, added in update order (AverageMeter.sum)
      window_losses                  the last min(u, window) losses, oldest first (AverageMeter.values)"""

    def __init__(self, state_i64, state_f64, num_classes, window):
        si, sf = np.asarray(state_i64), np.asarray(state_f64)
        C, W = int(num_classes), int(window)
        if si.shape != (meter_state_sizes(C, W)[0],) or sf.shape != (meter_state_sizes(C, W)[1],):
            raise ValueError('MeterSnapshot: the state arrays do not have the sizes of {} classes and a window of {}'.format(C, W))
        self.num_classes, self.window = C, W
        self.updates = u = int(si[0])
        self.correct, self.valid = int(si[1]), int(si[2])
        k = min(u, W)
        before = 4 + 2 * ((u - k) % (W + 1))  # the cumulative pair as it stood k updates ago
        self.window_correct, self.window_valid = self.correct - int(si[before]), self.valid - int(si[before + 1])
        self.mat = si[4 + 2 * (W + 1):].reshape(C, C).copy()
        self.loss_sum = float(sf[0])
        self.window_losses = [float(sf[1 + j % W]) for j in range(u - k + 1, u + 1)]

    # SegAccuracy's numbers
    @property
    def acc_avg(self):
        return self.window_correct / self.window_valid if self.window_valid else float('nan')

    @property
    def acc_global_avg(self):
        return (0.0 + self.correct) / self.valid if self.valid else float('nan')

    # SegIoU's: float32 torch arithmetic on the matrix, expression by expression
    @property
    def iou(self):
        h = torch.from_numpy(self.mat).float()
        tp = torch.diag(h)
        return tp / (h.sum(1) + h.sum(0) - tp)

    @property
    def iou_mean(self):
        return self.iou.mean().item()

    # the loss meter's (common/utils/metric_logger.py:26-38 with count = 1 per update)
    @property
    def loss_avg(self):
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.sum(self.window_losses) / np.sum([1] * len(self.window_losses))

    @property
    def loss_global_avg(self):
        return self.loss_sum / self.updates if self.updates != 0 else float('nan')

    # the three meter views over THIS snapshot (strings and numbers only: a snapshot takes no update)
    def snapshot(self):
        return self

    def meters(self):
        return _AccView(self), _IoUView(self), _LossView(self)

    def reset(self):
        raise RuntimeError('a MeterSnapshot is a host copy: reset the DeviceMeters it was read from')

    _update_once = lambda self, preds, labels: self.reset()


class _MeterView(object):
    """One meter of a DeviceMeters, as MetricLogger.add_meters takes it.  Reads go through the owner's host snapshot (one read serves all
    three views); `reset` resets the owner -- all three meters share one state."""

    def __init__(self, owner):
        self._owner = owner

    def reset(self):
        self._owner.reset()

    def update_dict(self, preds, labels):
        """The reference loop calls this on every meter of its list (train_mvpnet_3d.py:172-173): the first call with a given logit
        tensor updates the shared state, a repeat with the SAME tensor object -- the second view, or logits that SegLoss(meters=) has
        just counted -- does nothing."""
        self._owner._update_once(preds, labels)

    def __str__(self):
        return '{:.4f} ({:.4f})'.format(self.avg, self.global_avg)

    @property
    def summary_str(self):
        return '{:.4f}'.format(self.global_avg)


class _AccView(_MeterView):
    name = 'seg_acc'
    avg = property(lambda self: self._owner.snapshot().acc_avg)
    global_avg = property(lambda self: self._owner.snapshot().acc_global_avg)


class _IoUView(_MeterView):
    name = 'seg_iou'
    iou = property(lambda self: self._owner.snapshot().iou)
    mat = property(lambda self: self._owner.snapshot().mat)
    avg = global_avg = property(lambda self: self._owner.snapshot().iou_mean)

    def __str__(self):
        return '{iou:.4f}'.format(iou=self.global_avg)

    @property
    def summary_str(self):
        return str(self)


class _LossView(_MeterView):
    name = 'loss'
    avg = property(lambda self: self._owner.snapshot().loss_avg)
    global_avg = property(lambda self: self._owner.snapshot().loss_global_avg)

    def update_dict(self, preds, labels):
        pass  # (the loss reaches the state through SegLoss(meters=))


class DeviceMeters(object):
    """SegAccuracy, SegIoU and the loss meter of a training or validation loop (mvpnet/train_mvpnet_3d.py:170-173, :237-239) with their
    state on the device: ONE launch per iteration (mvp_seg_loss_meter_f32) and no device-to-host copy until a number is wanted.
    Attached to the loss -- SegLoss(meters=m), or `loss_fn.meters = m` -- the launch IS the loss launch: the argmax and the confusion
    count come from the logit rows the loss holds anyway, and the launch's last workgroup moves the window cursor, so the arguments
    are the same every step and the launch may sit in a captured graph.  `update_dict` is the same launch without a loss.

    The state is two tensors on the logits' device, made at the first update (state layout: include/mvp_hip.h): `state_i64` -- update
    count, cumulative (correct, valid), ticket, a ring of window + 1 cumulative pairs, the (C,C) matrix -- and `state_f64` -- loss sum,
    the last `window` losses.  Updates that share a DeviceMeters must be ordered on one stream.
    `read()` is the only synchronisation; `meters()`, `summary()` compute from its host snapshot.  The views re-read on their own when
    this object has launched an update since the last read; after graph replays, which it does not see, call read().
    An update without a loss (update_dict) puts NaN where its loss would be: the `loss` view says nan rather than average over fewer
    updates than it claims."""

    def __init__(self, num_classes, ignore_index=-100, window=20):
        if not 1 <= int(window) <= MAX_WINDOW or int(num_classes) < 1:
            raise ValueError('DeviceMeters: 1 <= window <= {} and num_classes >= 1 expected'.format(MAX_WINDOW))
        self.num_classes, self.ignore_index, self.window = int(num_classes), int(ignore_index), int(window)
        self._state = self.state_i64 = self.state_f64 = None
        self._snap, self._stale, self._last = None, True, None
        self._views = (_AccView(self), _IoUView(self), _LossView(self))

    # ---- the state -------------------------------------------------------------------------------------------------------------
    def _ensure(self, device):
        if self._state is None:
            ni, nf = meter_state_sizes(self.num_classes, self.window)
            self._state = torch.zeros(ni + nf, dtype=torch.int64, device=device)  # one allocation: reset() is one fill
            self.state_i64, self.state_f64 = self._state[:ni], self._state[ni:].view(torch.float64)
        elif self._state.device != device:
            raise RuntimeError('DeviceMeters: the state is on {}, the logits on {}'.format(self._state.device, device))

    def reset(self):
        if self._state is not None:
            self._state.zero_()
        self._snap, self._stale, self._last = None, True, None

    def state_dict(self):
        if self._state is None:
            return {'state_i64': None, 'state_f64': None}
        return {'state_i64': self.state_i64.clone(), 'state_f64': self.state_f64.clone()}

    def load_state_dict(self, state):
        si, sf = state['state_i64'], state['state_f64']
        if si is None:
            self._state = self.state_i64 = self.state_f64 = None
        else:
            ni, nf = meter_state_sizes(self.num_classes, self.window)
            if tuple(si.shape) != (ni,) or tuple(sf.shape) != (nf,) or si.dtype != torch.int64 or sf.dtype != torch.float64:
                raise ValueError('DeviceMeters.load_state_dict: not the state of {} classes and a window of {}'.format(self.num_classes, self.window))
            if self._state is None:
                if not si.is_cuda:
                    raise RuntimeError('DeviceMeters.load_state_dict: move the state to the GPU first (the state lives on the device)')
                self._ensure(si.device)
            self.state_i64.copy_(si)
            self.state_f64.copy_(sf)
        self._snap, self._stale, self._last = None, True, None

    # ---- updates ---------------------------------------------------------------------------------------------------------------
    def _operands(self, logit, label):
        """(B,C,N) logits and contiguous (B,N) labels as the kernel reads them, after the checks; ValueError outside its domain."""
        for t in (logit, label):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError('DeviceMeters takes tensors on the GPU; metric.SegAccuracy / metric.SegIoU exist for host tensors')
        if logit.dim() == 4 and label.dim() == 3:
            logit, label = logit.flatten(2), label.reshape(label.size(0), -1)
        if logit.dtype != torch.float32 or label.dtype != torch.int64 or logit.dim() != 3 or label.dim() != 2:
            raise ValueError('DeviceMeters: float32 (B,C,N) logits with int64 (B,N) labels, or (B,C,H,W) with (B,H,W), expected; got {} {} and {} {}'
                             .format(logit.dtype, tuple(logit.shape), label.dtype, tuple(label.shape)))
        if logit.size(1) != self.num_classes or (logit.size(0), logit.size(2)) != tuple(label.shape):
            raise ValueError('DeviceMeters: {} classes and labels {} do not fit the logits {}'.format(self.num_classes, tuple(label.shape), tuple(logit.shape)))
        return logit, label.contiguous()

    def _launch(self, logit, label, weight, acc, loss):
        """One mvp_seg_loss_meter_f32 on (B,C,N) `logit` / contiguous `label` (checked by the caller through _operands)."""
        self._ensure(logit.device)
        B, C, N = logit.shape
        sb, sc, sn = logit.stride()
        L.call('mvp_seg_loss_meter_f32', logit, L.ptr(logit), B, C, N, sb, sc, sn, L.ptr(label), L.ptr(weight), self.ignore_index, L.ptr(acc),
               L.ptr(loss), L.ptr(self.state_i64), L.ptr(self.state_f64), self.window)
        self._stale, self._last = True, None

    def _counted(self, source):
        """`source` (the caller's logit tensor object) is in the state: a view's update_dict with the same object adds nothing."""
        self._last = (weakref.ref(source), source._version)

    def update_dict(self, preds, labels):
        """The meters-only launch: accuracy counts and matrix of preds['seg_logit'] against labels['seg_label']."""
        source = preds['seg_logit']
        with torch.no_grad():
            logit, label = self._operands(source, labels['seg_label'])
            self._launch(logit, label, None, None, None)
        self._counted(source)

    def _update_once(self, preds, labels):
        source = preds['seg_logit']
        if self._last is not None and self._last[0]() is source and self._last[1] == source._version:
            return
        self.update_dict(preds, labels)

    # ---- reads -----------------------------------------------------------------------------------------------------------------
    def read(self):
        """-> MeterSnapshot of the state as it is now: one device-to-host copy, the only synchronisation."""
        ni, nf = meter_state_sizes(self.num_classes, self.window)
        host = np.zeros(ni + nf, np.int64) if self._state is None else self._state.cpu().numpy()
        self._snap, self._stale = MeterSnapshot(host[:ni], host[ni:].view(np.float64), self.num_classes, self.window), False
        return self._snap

    def snapshot(self):
        """The last read(), refreshed when this object has launched an update since."""
        return self.read() if self._stale or self._snap is None else self._snap

    def meters(self):
        """(seg_acc, seg_iou, loss): three light views with `name`, `avg`, `global_avg`, `__str__`, `summary_str`, `reset`, `update_dict`
        -- what MetricLogger.add_meters takes, and after the same updates the strings and numbers of SegAccuracy, SegIoU and the
        reference's AverageMeter of the loss."""
        return self._views

    def summary(self):
        """{'loss', 'seg_acc', 'seg_iou'}: the global averages, after one read()."""
        s = self.read()
        return {'loss': s.loss_global_avg, 'seg_acc': s.acc_global_avg, 'seg_iou': s.iou_mean}


def summary_from_confusion(mat):
    """{'seg_acc', 'seg_iou'} of a (C,C) int64 confusion matrix on the device (mvpnet2d.validate_2d's): the expressions of
    SegAccuracy.global_avg and SegIoU.global_avg, so the numbers are the ones the two meters report after the same batches.  The read is
    the only synchronisation."""
    correct, valid = torch.stack([mat.diagonal().sum(), mat.sum()]).tolist()
    h = mat.float()
    tp = torch.diag(h)
    return {'seg_acc': (0.0 + correct) / valid if valid else float('nan'), 'seg_iou': (tp / (h.sum(1) + h.sum(0) - tp)).mean().item()}


def label_log_weights(hist, class_ids=None):
    """The class weights `1 / log(1.2 + frequency)` that SegLoss is built with, from label counts (ops.label_histogram's, a tensor on the
    device -- reading it is the only synchronisation -- or an array): the arithmetic of
    mvpnet/data/preprocess/compute_label_weights.py:27-29 and :45-47, operation by operation.  The counts, taken at class_ids when given
    (compute_3d_weights' VALID_CLASS_IDS = EVAL_CLASS_IDS), are cast to float32, divided by their float32 sum, and 1 / np.log(1.2 + w)
    stays float32.  -> (len,) float32 NumPy array: what np.savetxt writes there and what SegLoss / config.build_loss_2d take as weights."""
    counts = hist.cpu().numpy() if torch.is_tensor(hist) else np.asarray(hist)
    label_weights = counts.astype(np.float64).astype(np.float32)
    if class_ids is not None:
        label_weights = label_weights[list(class_ids)]
    label_weights = label_weights / np.sum(label_weights)
    return 1 / np.log(1.2 + label_weights)

"""NumPy restatement of the meter state that mvp_seg_loss_meter_f32 keeps on the device (plain helper module, layout of include/mvp_hip.h),
and a deque-based loss meter: the semantics of the reference's SegAccuracy / SegIoU (mvpnet/models/metric.py) and AverageMeter
(common/utils/metric_logger.py) written out for the tests of metric.DeviceMeters.

  state_i64: [0] u  [1] correct  [2] valid  [3] ticket (0 between launches)  [4 + 2 s, 5 + 2 s] ring of W + 1 cumulative pairs
             [4 + 2 (W + 1) ...] the (C,C) matrix [label][argmax]
  state_f64: [0] sum of the losses  [1 + j % W] the float32 loss of update j"""
import collections

import numpy as np


def sizes(C, W):
    return 4 + 2 * (W + 1) + C * C, 1 + W


def new_state(C, W):
    ni, nf = sizes(C, W)
    return np.zeros(ni, np.int64), np.zeros(nf, np.float64)


def confusion(logit, label, ignore_index=-100):
    """(C,C) int64 [label][argmax] of (B,C,N) logits against (B,N) labels: first maximum (np.argmax), points whose label is ignore_index
    or outside [0, C) skipped."""
    C = logit.shape[1]
    pred = np.argmax(logit, axis=1)
    keep = (label != ignore_index) & (label >= 0) & (label < C)
    return np.bincount(C * label[keep] + pred[keep], minlength=C * C).reshape(C, C).astype(np.int64)


def update(si, sf, C, W, mat, loss=None):
    """One update, in place: `mat` the (C,C) counts of this update's points, `loss` its float32 loss (None: an update without a loss)."""
    si[1] += int(np.trace(mat))
    si[2] += int(mat.sum())
    si[4 + 2 * (W + 1):] += mat.reshape(-1)
    u = int(si[0]) + 1
    si[0] = u
    si[4 + 2 * (u % (W + 1)):6 + 2 * (u % (W + 1))] = si[1:3]
    value = float('nan') if loss is None else float(np.float32(loss))
    sf[1 + u % W] = value
    sf[0] += value


class LossMeter(object):
    """The loss meter of the training loop: window mean over the last `window` values, global mean over all, one count per update."""

    def __init__(self, window=20):
        self.values = collections.deque(maxlen=window)
        self.counts = collections.deque(maxlen=window)
        self.sum, self.count = 0.0, 0

    def update(self, value):
        self.values.append(value)
        self.counts.append(1)
        self.sum += value
        self.count += 1

    @property
    def avg(self):
        return np.sum(self.values) / np.sum(self.counts)

    @property
    def global_avg(self):
        return self.sum / self.count if self.count != 0 else float('nan')

    def __str__(self):
        return '{:.4f} ({:.4f})'.format(self.avg, self.global_avg)

    @property
    def summary_str(self):
        return '{:.4f}'.format(self.global_avg)

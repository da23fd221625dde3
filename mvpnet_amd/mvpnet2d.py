"""MVPNet2D: the 2D-only baseline that lifts per-pixel class logits to the points (mvpnet/models/mvpnet_2d.py:7-34).

Same class name, constructor, data-dict keys (`images`, `knn_indices` -> `seg_logit` (B, classes, N)).  The reference
re-lays the logits out as (B, classes, nv*h*w) (a transposed copy), gathers with `group_points` (channel-major: classes x
N*k scattered 4-byte reads) and averages over k.  Here the 2D network's (B*nv, classes, h, w) output is viewed
channels-last -- free when it already runs in torch.channels_last --, the k-NN rows are gathered by the lifting gather
kernel (mvp_lift_gather_f32: one 80-byte row per neighbour) and averaged.  As in MVPNet3D, the k-NN indices may be computed
on the device from depth / intrinsics / pose when the loader does not supply them."""
import torch
from torch import nn

from . import ops
from . import optim
from .nn import eval_mode
from .scene import _resize_target, _sized_frames


class MVPNet2D(nn.Module):
    def __init__(self, net_2d):
        super(MVPNet2D, self).__init__()
        self.net_2d = net_2d

    def forward(self, data_batch):
        images = data_batch['images']  # (B,nv,3,h,w)
        b, nv, _, h, w = images.shape
        seg_logit_2d = self.net_2d({'image': images.reshape(b * nv, *images.shape[2:])})['seg_logit']  # (B*nv,classes,h,w)
        nc = seg_logit_2d.size(1)
        logit_cl = seg_logit_2d.permute(0, 2, 3, 1).contiguous().view(b, nv, h, w, nc)  # channels-last rows
        knn = data_batch.get('knn_indices')
        if knn is None:
            # device lifting from depth / intrinsics / pose.  The fused kernel gathers rows whose 16-byte chunks divide a 256-lane
            # workgroup (C/4 | 256); 20 class logits do not, so the indices come from the un-project + projective k-NN entry
            # points and the rows from the generic gather below.
            cam = data_batch['cam_matrix']
            kinv = data_batch['kinv'] if 'kinv' in data_batch else torch.linalg.inv(cam)
            xyz, mask = ops.unproject(data_batch['depth'], kinv, data_batch['pose'], data_batch.get('pixel_box'))
            knn = ops.pixel_knn(xyz, mask, data_batch['points'].transpose(1, 2).contiguous(), int(data_batch.get('k', 3)), cam=cam,
                                pose=data_batch['pose'])
        gathered, _ = ops.lift_gather(logit_cl, None, knn)  # (B,N,k,classes)
        return {'seg_logit': gathered.mean(2).transpose(1, 2).contiguous()}


def train_step_2d(model, loss_fn, optimizer, data_batch, scheduler=None, max_grad_norm=0.0):
    """One iteration of the reference's 2D-stage loop (mvpnet/train_2d.py:158-185):
    zero_grad -> forward -> loss_fn(preds, batch)['seg_loss'] -> backward -> [clip] -> step -> scheduler; -> (loss.detach(), preds).
    With max_grad_norm > 0 and an optim.FusedSGD the clip is deferred: optim.total_grad_norm leaves its coefficient on the device and
    the step multiplies the gradients by it as it reads them -- they are read once for the norm, once in the step and never rewritten
    (so p.grad holds the UNclipped gradients afterwards).  Any other optimizer gets optim.clip_grad_norm_, the in-place clip.
    The iteration's meters (train_2d.py:174-177) ride on loss_fn: SegLoss(meters=metric.DeviceMeters(...)) updates them in the loss launch."""
    optimizer.zero_grad()
    preds = model(data_batch)
    loss = loss_fn(preds, data_batch)['seg_loss']
    loss.backward()
    if max_grad_norm > 0 and isinstance(optimizer, optim.FusedSGD):
        _, coef = optim.total_grad_norm(model.parameters(), max_grad_norm)
        optimizer.step(grad_scale=coef if coef.is_cuda else None)  # (no gradient at all: nothing to scale)
    else:
        if max_grad_norm > 0:
            optim.clip_grad_norm_(model.parameters(), max_grad_norm)
        optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return loss.detach(), preds


def _eval_batches(who, store, frames, batch_size, resize):
    """-> (frames (n,) int64 on the device, size = (w, h) or None when the store's size is kept, the batches as slices)"""
    images = store['images']
    labels = store.get('labels')
    if images.dim() != 4 or (labels is not None and (labels.dim() != 3 or tuple(labels.shape) != tuple(images.shape[:3]))):
        raise RuntimeError(who + ': images (Ftot,H,W,3) uint8 and labels (Ftot,H,W) uint16 must describe the same frames')
    if int(batch_size) < 1:
        raise RuntimeError(who + ': batch_size must be >= 1')
    if frames is None:
        frames = torch.arange(images.size(0), dtype=torch.int64, device=images.device)
    if frames.dim() != 1:
        raise RuntimeError(who + ': frames must be (n,)')
    if frames.numel() < 1:
        raise RuntimeError(who + ': no frames')
    return frames, _resize_target(resize, images.size(2), images.size(1)), [slice(i, min(i + int(batch_size), frames.numel())) for i in range(0, frames.numel(), int(batch_size))]


def test_frames_2d(model, store, frames=None, *, batch_size, resize=None, image_normalizer=None, label_mapping=None, channels_last=False,
                   evaluator=None, want_pred=False):
    """The loop of the reference's stage-one test (mvpnet/test_2d.py:103-118) from frames resident on the device, under torch.no_grad():
    batches of `frames` in order, the last one partial (drop_last=False); per batch the images as scene.sample_train_batch_2d makes them
    without an augmentation (resize -> `/ 255.` -> normalise), model({'image': ...})['seg_logit'], evaluator.update_frames -- the argmax,
    the labels through Pillow's NEAREST indices and label_mapping, and the count in one launch.  No label tensor is made and nothing is
    synchronised in the loop; the first number read from the evaluator is the synchronisation.  The model runs in eval mode (its mode is
    restored afterwards).
    store: images (Ftot,H,W,3) uint8 [, labels (Ftot,H,W) uint16]; frames (n,) int64 on the device or None for all; resize,
    image_normalizer, label_mapping, channels_last: as scene.sample_train_batch_2d (config.build_batch_2d(cfg, training=False)).
    evaluator: a metric.DeviceEvaluator to add to, a fresh `DeviceEvaluator(metric.CLASS_NAMES)` otherwise -- the network's class count
    must be its.  -> the evaluator, or (evaluator, pred (n,h,w) int64) with want_pred.  A store without 'labels' (an unlabelled split)
    gives (None, pred).  The command line, the logging and the table printing of the script are out of scope."""
    from . import metric
    frames, size, batches = _eval_batches('test_frames_2d', store, frames, batch_size, resize)
    labels = store.get('labels')
    if labels is not None and evaluator is None:
        evaluator = metric.DeviceEvaluator(metric.CLASS_NAMES)
    preds = []
    with eval_mode(model):
        for part in batches:
            picked = frames[part]
            image = _sized_frames(store['images'], picked, size, normalizer=image_normalizer, channels_last=channels_last)
            logit = model({'image': image})['seg_logit']
            if labels is None:
                preds.append(ops.frame_confusion(logit, None, None))
            else:
                pred = evaluator.update_frames(logit, labels, picked, size=size, mapping=label_mapping, want_pred=want_pred)
                if want_pred:
                    preds.append(pred)
    if labels is None:
        return None, torch.cat(preds)
    return (evaluator, torch.cat(preds)) if want_pred else evaluator


def validate_2d(model, loss_fn, store, frames, *, batch_size, resize=None, image_normalizer=None, label_mapping=None, channels_last=False):
    """The validation pass of the reference's stage-one training (mvpnet/train_2d.py:240-312) from frames resident on the device: the
    model in eval mode (its mode is restored afterwards) under torch.no_grad(), batches of `frames` in order with the last one partial,
    per batch loss_fn(preds, batch)['seg_loss'] and the confusion matrix.  SegLoss reads a label tensor, so the batch's labels are made
    once with ops.prepare_labels and the matrix is taken from the same tensor (metric.confusion_matrix); nothing is synchronised.
    -> {'loss': the mean of the per-batch losses (what the reference's loss meter reports as global_avg), a device scalar,
        'confusion': (C,C) int64 on the device}; metric.summary_from_confusion turns the matrix into the seg_acc / seg_iou that
    SegAccuracy and SegIoU report for the same batches.  Batch arguments: as test_frames_2d."""
    from . import metric
    frames, size, batches = _eval_batches('validate_2d', store, frames, batch_size, resize)
    losses, mat = [], None
    with eval_mode(model):
        for part in batches:
            picked = frames[part]
            batch = {'image': _sized_frames(store['images'], picked, size, normalizer=image_normalizer, channels_last=channels_last),
                     'seg_label': ops.prepare_labels(store['labels'], picked, size=size, mapping=label_mapping)}
            preds = model(batch)
            losses.append(loss_fn(preds, batch)['seg_loss'])
            mat = metric.confusion_matrix(preds['seg_logit'], batch['seg_label'], out=mat)
    return {'loss': torch.stack(losses).mean(), 'confusion': mat}

"""MVPNet 2D->3D lifting + aggregation in front of PN2SSG: mirror of
`mvpnet.models.mvpnet_3d` (reference: mvpnet/models/mvpnet_3d.py:9-118) and of
`mvpnet.models.loss.SegLoss` (loss.py:5-21).

Differences from the reference that do not change results:
  * the 2D feature map is consumed channels-last ((B*nv, C, h, w) in torch.channels_last memory
    format IS (B,nv,h,w,C) physically), so each gathered neighbour is one contiguous row and the
    `transpose(1,2).contiguous()` full copy of mvpnet_3d.py:101 disappears;
  * `knn_indices` / `image_xyz` may be omitted from the data dict when `depth`, `cam_matrix`,
    `pose` (and optionally `pixel_box`) are given: they are then computed on the device with the
    lifting kernels instead of by dataloader workers (scannet_2d3d.py:254-313).
"""
import os

import torch
from torch import nn
import torch.nn.functional as F

from .nn import SharedMLP, xavier_uniform
from . import ops
from . import _lib as L
from . import rows as R


REL_EPILOGUE = os.environ.get('MVP_REL_EPILOGUE', '1') != '0'  # A/B switch: relation columns in the first layer's epilogue


class FeatureAggregation(nn.Module):
    """cat[feature, src - tgt, |src - tgt|^2] -> SharedMLP -> reduce over k (mvpnet_3d.py:9-67)."""

    def __init__(self, in_channels, mlp_channels=(64, 64, 64), reduction='sum', use_relation=True):
        super().__init__()
        self.in_channels, self.use_relation = in_channels, use_relation
        if mlp_channels:
            self.out_channels = mlp_channels[-1]
            self.mlp = SharedMLP(in_channels + (4 if use_relation else 0), mlp_channels, ndim=2, bn=True)
        else:
            self.out_channels, self.mlp = in_channels, None
        if reduction not in ('sum', 'max'):
            raise ValueError('reduction must be sum or max')
        self.reduction_name = reduction
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Linear)):
                xavier_uniform(m)

    def reduction(self, x, dim):
        return torch.sum(x, dim) if self.reduction_name == 'sum' else torch.max(x, dim)[0]

    def forward_rows(self, gxyz, points, gfeat):
        """gxyz (B,N,k,3), points (B,N,3), gfeat (B,N,k,C) channels-last -> (B,N,C_out) rows."""
        B, N, k, C = gfeat.shape
        if self.mlp is None:
            return gfeat.sum(2) if self.reduction_name == 'sum' else gfeat.max(2)[0]
        x = gfeat
        if self.use_relation and REL_EPILOGUE and gfeat.is_cuda and gfeat.dtype == torch.float32 and C % 4 == 0 and R.mlp_chain_is_fused(self.mlp) \
                and self.mlp[0].conv.weight.size(1) == C + 4:
            # [feature | src - tgt | squared length] (:55-56) is never built: the first conv reads the gathered feature rows as they are,
            # the four relation columns meet their weight columns in that kernel's epilogue (the 68-wide operand cost a 214 MB tensor and
            # 2.3x the layer's time: csrc/mlp.hip, EpiBwd::rel)
            rel = R.relation4_rows(gxyz, points)
            return R.shared_mlp_rows(gfeat.reshape(B * N * k, C), self.mlp, K=k, reduce=self.reduction_name, rel=rel.view(B * N * k, 4)).view(B, N, -1)
        if self.use_relation and gfeat.is_cuda and gfeat.dtype == torch.float32 and C % 4 == 0:
            x = R.relation_rows(gfeat, gxyz, points)  # feature, diff, dist (:55-56) written in one pass
        elif self.use_relation:
            diff = gxyz - points.unsqueeze(2)
            x = torch.cat([gfeat, diff, torch.sum(diff ** 2, dim=3, keepdim=True)], dim=3)
        if x.size(3) % 4:
            x = torch.nn.functional.pad(x, (0, 4 - x.size(3) % 4))
        # the reduction over the k neighbours (max or sum, :40-41,59) is folded into the last layer's BatchNorm + ReLU kernel
        return R.shared_mlp_rows(x.reshape(B * N * k, -1), self.mlp, K=k, reduce=self.reduction_name).view(B, N, -1)

    def forward(self, src_xyz, tgt_xyz, feature, rows=False):
        """src_xyz (B,3,N,k), tgt_xyz (B,3,N), feature (B,C,N,k) -> (B,C_out,N).
        rows=True: channels-last (B,N,k,3), (B,N,3), (B,N,k,C) -> (B,N,C_out)."""
        if rows:
            return self.forward_rows(src_xyz, tgt_xyz, feature)
        if self.mlp is None:
            return self.reduction(feature, 3)
        x = feature
        if self.use_relation:
            diff = src_xyz - tgt_xyz.unsqueeze(-1)
            x = torch.cat([feature, diff, torch.sum(diff ** 2, dim=1, keepdim=True)], dim=1)
        return self.reduction(self.mlp(x), 3)


def points_rows(data_batch, points=None):
    """(B,N,3) rows of the batch's (B,3,N) `points` (or of another (B,3,N) tensor of the batch, e.g. the rotated points), transposed ONCE
    per batch: lifting, aggregation, the geometry plan and the 3D network all read the same copy (four transposing launches per training
    step before).  Cached in the batch dict under a private key, per source tensor and its version counter (an in-place refill of a
    loader's static buffer gives a new copy)."""
    points = data_batch['points'] if points is None else points
    cache = data_batch.get('_points_rows')
    if cache is None:
        cache = data_batch['_points_rows'] = {}
    hit = cache.get(id(points))
    if hit is not None and hit[0] is points and hit[1] == points._version:
        return hit[2]
    rows = points.transpose(1, 2).contiguous()
    if len(cache) >= 2:  # a batch has at most two sources (the loader's points, the rotated ones): a dict that is REUSED with new
        cache.clear()    # point tensors must not collect their copies
    cache[id(points)] = (points, points._version, rows)
    return rows


def net3d_points(data_batch):
    """(B,3,N) points as the 3D network sees them: the loader's points, or -- when the batch carries a device-side z rotation
    ('z_rot' (B,3,3) float64 from mvpnet_amd.augment, lifting still to be done on the device) -- those points rotated
    (scannet_2d3d.py:400-409; the pixel k-NN runs on the UN-rotated points, everything after it on the rotated ones)."""
    points = data_batch['points']
    if 'z_rot' not in data_batch or 'knn_indices' in data_batch:
        return points
    if '_points_rot' not in data_batch:
        data_batch['_points_rot'] = ops.rotate_rows(points_rows(data_batch), data_batch['z_rot']).transpose(1, 2).contiguous()
    return data_batch['_points_rot']


class MVPNet3D(nn.Module):
    def __init__(self, net_2d, net_2d_ckpt_path, net_3d, **feat_aggr_kwargs):
        super().__init__()
        self.net_2d = net_2d
        if net_2d_ckpt_path:
            checkpoint = torch.load(net_2d_ckpt_path, map_location=torch.device('cpu'))
            self.net_2d.load_state_dict(checkpoint['model'])
        self.feat_aggreg = FeatureAggregation(**feat_aggr_kwargs)
        self.net_3d = net_3d

    @staticmethod
    def lift(feature_cl, data_batch):
        """Device lifting from depth (B,nv,h,w), cam_matrix (B,nv,3,3 forward intrinsics already scaled to
        (h,w)), pose (B,nv,4,4) [, kinv, pixel_box (B,4), k]: gathered feature, gathered xyz, knn_indices."""
        cam = data_batch['cam_matrix']
        kinv = data_batch['kinv'] if 'kinv' in data_batch else torch.linalg.inv(cam)
        points_nc = points_rows(data_batch)  # (B,N,3), un-rotated: the search precedes the rotation
        return ops.lift(feature_cl, data_batch['depth'], kinv, cam, data_batch['pose'], points_nc,
                        k=int(data_batch.get('k', 3)), box=data_batch.get('pixel_box'), flip=data_batch.get('flip'),
                        rot=data_batch.get('z_rot'))

    @staticmethod
    def lift_store(data_batch):
        """`lift` for a batch that carries feature_store (U,h,w,C) and view_slot (B,nv) int32 in place of `images`: the rows of the
        shared store are read through view_slot.  Test path: no flip, no z rotation."""
        if 'flip' in data_batch or 'z_rot' in data_batch:
            raise RuntimeError('MVPNet3D: a batch with feature_store / view_slot takes no flip / z_rot (the un-augmented test path)')
        cam = data_batch['cam_matrix']
        kinv = data_batch['kinv'] if 'kinv' in data_batch else torch.linalg.inv(cam)
        return ops.lift_store(data_batch['feature_store'], data_batch['view_slot'], data_batch['depth'], kinv, cam, data_batch['pose'],
                              points_rows(data_batch), k=int(data_batch.get('k', 3)), box=data_batch.get('pixel_box'))

    def _side_stream(self, device):
        if getattr(self, '_geo_stream', None) is None or self._geo_stream.device != device:
            self._geo_stream = torch.cuda.Stream(device=device)
        return self._geo_stream

    def forward(self, data_batch):
        with R.zero_pool.step(data_batch['points'].device), R.eval_invstd.scope(self):  # rows.ZeroPool / rows.EvalInvStd
            return self._forward(data_batch)

    def _forward(self, data_batch):
        # coordinate-only work of the 3D network (FPS chain, ball queries, 3-NN) starts on a side stream
        # now and overlaps the 2D network, the lifting and the aggregation MLP below.
        plan = data_batch.get('geometry_plan')
        points = net3d_points(data_batch)  # what the 3D network sees (rotated when the batch carries a device-side z rotation)
        if plan is None and hasattr(self.net_3d, 'plan_geometry') and points.is_cuda:
            pts_rows = points_rows(data_batch, points)
            plan = self.net_3d.plan_geometry(pts_rows, stream=self._side_stream(pts_rows.device))
        if 'feature_store' in data_batch and 'view_slot' in data_batch:
            # whole-scene test (scene.infer_scene_shared): the 2D network already ran ONCE per distinct frame into a store shared by all
            # chunks; no `images`, no net_2d call, no (B,nv,h,w,C) copy -- the rows are read through view_slot (mvp_lift_store_f32)
            gfeat, gxyz = self.lift_store(data_batch)[:2]  # (B,N,k,C), (B,N,k,3)
            return self._after_lift(data_batch, points, plan, gfeat, gxyz)
        images = data_batch['images']  # (B,nv,3,h,w)
        b, nv, _, h, w = images.shape
        # consumed exactly once (a batch dict that is reused must not feed a stale map to a later step, nor keep the tensor pinned), and only
        # while the branch is still what it was when the map was made: frozen (an unfrozen branch must run in-line to get its gradient)
        pre = data_batch.pop('_feature_2d', None) if isinstance(data_batch, dict) else None
        if pre is not None and net_2d_is_frozen(self) and pre[0].size(0) == b * nv:
            feature_2d, ev = pre  # the frozen 2D network already ran for this batch on its own stream (prefetch_features_2d)
            torch.cuda.current_stream(feature_2d.device).wait_event(ev)
        else:
            feature_2d = self.net_2d({'image': images.reshape(b * nv, *images.shape[2:])})['feature']  # (B*nv,C,h,w)
        c = feature_2d.size(1)
        # a bfloat16 / float16 map (frozen_inference(feature_dtype=...)) goes to the lift as it is: the gather widens its rows, no float32
        # copy.  One that needs a gradient is widened here: the scatter-add backward is float32 only
        if feature_2d.dtype in (torch.bfloat16, torch.float16) and feature_2d.requires_grad and torch.is_grad_enabled():
            feature_2d = feature_2d.float()
        # channels-last view (B,nv,h,w,C); free when the 2D net already runs in torch.channels_last
        feature_cl = feature_2d.permute(0, 2, 3, 1).contiguous().view(b, nv, h, w, c)
        if 'knn_indices' in data_batch and 'image_xyz' in data_batch:  # loader-supplied, as in the reference
            gfeat, gxyz = ops.lift_gather(feature_cl, data_batch['image_xyz'], data_batch['knn_indices'])
        else:  # device lifting: un-project + pixel k-NN + gather fused (mvp_lift_f32)
            gfeat, gxyz = self.lift(feature_cl, data_batch)[:2]  # (B,N,k,C), (B,N,k,3)
        return self._after_lift(data_batch, points, plan, gfeat, gxyz)

    def _after_lift(self, data_batch, points, plan, gfeat, gxyz):
        """Everything behind the lifting: the next batch's geometry, the aggregation and the 3D network."""
        nxt = data_batch.get('prefetch_next')
        if nxt is not None:  # start the NEXT batch's FPS / ball query / 3-NN now: runs under this batch's MLPs
            prefetch_geometry(self, nxt)
        rows = points_rows(data_batch, points)
        feature_2d3d = self.feat_aggreg(gxyz, rows, gfeat, rows=True)  # (B,N,C) rows
        return self.net_3d({'points': points, 'points_rows': rows, 'feature_rows': feature_2d3d, 'geometry_plan': plan})


class _SegLossFn(torch.autograd.Function):
    """F.cross_entropy(logit (B,C,N), label (B,N), weight, ignore_index) in one forward and one backward kernel
    (mvp_seg_loss_f32 / mvp_seg_loss_backward_f32): no (B,C,N) log-probability tensor, no nll_loss fill + scatter."""

    last_acc = None

    @staticmethod
    def forward(ctx, logit, label, weight, ignore_index):
        L.require_gpu(label, weight)
        B, C, N = logit.shape
        acc = R.zero_pool.zeros(3, torch.float64, logit.device)  # [sum w*nll, sum w, ticket]
        loss = torch.empty((), dtype=torch.float32, device=logit.device)
        sb, sc, sn = logit.stride()
        L.call('mvp_seg_loss_f32', logit, L.ptr(logit), B, C, N, sb, sc, sn, L.ptr(label), L.ptr(weight), int(ignore_index), L.ptr(acc),
               L.ptr(loss))
        ctx.save_for_backward(logit, label, weight, acc)
        ctx.ignore_index = int(ignore_index)
        _SegLossFn.last_acc = acc  # [sum w*nll, sum w, ticket] of the latest call (SegLoss.last_weight_sum reads [1])
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        logit, label, weight, acc = ctx.saved_tensors
        B, C, N = logit.shape
        g = grad_out.contiguous().to(torch.float32)
        sb, sc, sn = logit.stride()
        # the gradient in the logits' own layout: PN2SSG hands out a transposed VIEW of its (B,N,classes) rows, and a gradient with the
        # same strides flows back into the row kernels without a transposing copy (a (B,C,N)-contiguous logit gets a contiguous gradient)
        dense = sorted((sb, sc, sn), reverse=True) in ([C * N, N, 1], [N * C, C, 1])
        grad = torch.empty_strided((B, C, N), (sb, sc, sn) if dense else (C * N, N, 1), dtype=torch.float32, device=logit.device)
        gb, gc, gn = grad.stride()
        L.call('mvp_seg_loss_backward_f32', logit, L.ptr(logit), B, C, N, sb, sc, sn, L.ptr(label), L.ptr(weight), ctx.ignore_index,
               L.ptr(acc), L.ptr(g), L.ptr(grad), gb, gc, gn)
        return grad, None, None, None


class _SegLossMeterFn(torch.autograd.Function):
    """_SegLossFn with the meters of the iteration updated by the same launch (mvp_seg_loss_meter_f32: the loss sums, acc and the loss
    scalar are mvp_seg_loss_f32's; metric.DeviceMeters holds the meter state).  The backward is _SegLossFn's, on the same acc."""

    @staticmethod
    def forward(ctx, logit, label, weight, ignore_index, meters):
        L.require_gpu(label, weight)
        acc = R.zero_pool.zeros(3, torch.float64, logit.device)  # [sum w*nll, sum w, ticket]
        loss = torch.empty((), dtype=torch.float32, device=logit.device)
        meters._launch(logit, label, weight, acc, loss)
        ctx.save_for_backward(logit, label, weight, acc)
        ctx.ignore_index = int(ignore_index)
        _SegLossFn.last_acc = acc
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        return _SegLossFn.backward(ctx, grad_out) + (None,)


class SegLoss(nn.Module):
    """Weighted cross entropy with ignore_index (loss.py:5-21).  fp32 (B,C,N) logits on the GPU go through the fused HIP
    kernels (logits in any strides), and so do the 2D stage's (B,C,H,W) logits with (B,H,W) labels, contiguous or channels-last: they
    are VIEWED as (B,C,H*W) -- both layouts merge H and W without a copy -- and the gradient comes back in the logits' own layout;
    everything else (host tensors, other dtypes / ranks) through F.cross_entropy, which is what the reference calls.
    meters: a metric.DeviceMeters (given here or set later as the attribute `meters`) -- on the fused path the forward is then ONE launch
    that also updates the iteration's meters (SegAccuracy, SegIoU, the loss meter: train_mvpnet_3d.py:170-173) on the device, in training
    and under no_grad alike, with nothing read back; the backward is unchanged.  On the F.cross_entropy path `meters.update_dict` follows
    the loss (it refuses what its kernel cannot take).  The meters' class count and ignore_index must be this loss's.  None: no meters."""

    def __init__(self, weight=None, ignore_index=-100, meters=None):
        super().__init__()
        self.weight, self.ignore_index = weight, ignore_index
        self.last_weight_sum = None  # sum of w[label] over the valid points of the last call (0-dim tensor): dist.GradSync(weight_sum=)
        self.meters = meters

    def forward(self, preds, labels):
        if self.meters is not None:
            return self._forward_meters(preds, labels, self.meters)
        logit, label = preds['seg_logit'], labels['seg_label']
        if logit.is_cuda and logit.dtype == torch.float32 and logit.dim() == 4 and label.dim() == 3 and label.dtype == torch.int64:
            # (B,C,H,W) -> (B,C,H*W): a view for contiguous and channels-last memory alike (stride(H) == W * stride(W))
            logit, label = logit.flatten(2), label.reshape(label.size(0), -1)
        if logit.is_cuda and logit.dtype == torch.float32 and logit.dim() == 3 and label.dtype == torch.int64:
            weight = None if self.weight is None else self.weight.to(device=logit.device, dtype=torch.float32).contiguous()
            loss = _SegLossFn.apply(logit, label.contiguous(), weight, self.ignore_index)
            self.last_weight_sum = _SegLossFn.last_acc[1] if _SegLossFn.last_acc is not None else None
        else:
            loss = F.cross_entropy(logit, label, weight=self.weight, ignore_index=self.ignore_index)
            with torch.no_grad():
                valid = label != self.ignore_index
                self.last_weight_sum = (valid.sum().to(logit.dtype) if self.weight is None
                                        else self.weight.to(logit.device)[label[valid]].sum())
        return {'seg_loss': loss}

    def _forward_meters(self, preds, labels, meters):
        source, label = preds['seg_logit'], labels['seg_label']
        if meters.ignore_index != self.ignore_index:
            raise ValueError('SegLoss: the meters ignore {}, the loss ignores {}'.format(meters.ignore_index, self.ignore_index))
        fused = source.is_cuda and source.dtype == torch.float32 and label.dtype == torch.int64 and \
            ((source.dim() == 4 and label.dim() == 3) or source.dim() == 3)
        if not fused:
            self.meters = None
            try:
                out = self.forward(preds, labels)
            finally:
                self.meters = meters
            meters.update_dict(preds, labels)
            return out
        logit, label = meters._operands(source, label)  # the (B,C,N) view and contiguous labels; ValueError before any launch
        weight = None if self.weight is None else self.weight.to(device=logit.device, dtype=torch.float32).contiguous()
        loss = _SegLossMeterFn.apply(logit, label, weight, self.ignore_index, meters)
        meters._counted(source)
        self.last_weight_sum = _SegLossFn.last_acc[1] if _SegLossFn.last_acc is not None else None
        return {'seg_loss': loss}


def prefetch_geometry(model, data_batch):
    """Start the coordinate-only work (FPS chain, ball queries, 3-NN) of `data_batch` on the model's side
    stream and store the plan in the batch.  Called for batch i+1 before the forward of batch i, the ~3 ms
    FPS dependency chain (which can only use B of the 256 CUs) runs under batch i's forward + backward --
    the device-side counterpart of the reference's dataloader workers running ahead of the training loop.
    A LIST of batches (inference) is planned in one call: see prefetch_geometry_many."""
    if isinstance(data_batch, (list, tuple)):
        return prefetch_geometry_many(model, data_batch)
    net = model.module if hasattr(model, 'module') else model
    if 'geometry_plan' not in data_batch and hasattr(net, 'net_3d') and data_batch['points'].is_cuda:
        pts_rows = points_rows(data_batch, net3d_points(data_batch))
        data_batch['geometry_plan'] = net.net_3d.plan_geometry(pts_rows, stream=net._side_stream(pts_rows.device))
    return data_batch


def net_2d_is_frozen(net):
    """True when the 2D branch of `net` takes no gradient and runs with fixed statistics: every parameter has requires_grad False and
    no BatchNorm is in training mode -- the reference's Freezer state (mvpnet/train_mvpnet_3d.py:142-143, common/nn/freezer.py)."""
    n2 = getattr(net, 'net_2d', None)
    if n2 is None:
        return False
    ps = list(n2.parameters())
    return bool(ps) and not any(p.requires_grad for p in ps) and not any(m.training for m in n2.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm))


def prefetch_features_2d(model, data_batch):
    """Run the FROZEN 2D network (mvpnet/models/unet_resnet34.py:9-125 behind mvpnet_3d.py:99) of `data_batch` now, on its own stream, and
    keep the feature map in the batch: called for batch i+1 while batch i trains, the image branch -- which depends on nothing of the
    3D network or of the previous step once it is frozen -- runs under the 3D network's backward pass instead of in front of its forward
    (VERDICT r3 next #9).  No-op when the branch trains, has no parameters (a supplied feature map), or the batch already carries one."""
    net = model.module if hasattr(model, 'module') else model
    if '_feature_2d' in data_batch or 'images' not in data_batch or not data_batch['images'].is_cuda or not net_2d_is_frozen(net):
        return data_batch
    images = data_batch['images']
    dev = images.device
    st = getattr(net, '_feat_stream', None)
    if st is None or st.device != dev:
        st = net._feat_stream = torch.cuda.Stream(device=dev)
    cur = torch.cuda.current_stream(dev)
    st.wait_stream(cur)
    b, nv = images.shape[:2]
    with torch.cuda.stream(st), torch.no_grad():
        feature_2d = net.net_2d({'image': images.reshape(b * nv, *images.shape[2:])})['feature']
        ev = torch.cuda.Event()
        ev.record(st)
    if not torch.cuda.is_current_stream_capturing():
        images.record_stream(st)
        feature_2d.record_stream(cur)
    data_batch['_feature_2d'] = (feature_2d, ev)
    return data_batch


def prefetch_geometry_many(model, batches):
    """The coordinate-only work of SEVERAL upcoming batches in one call (inference: no transposed indices).  Farthest point sampling
    is a serial chain that occupies one CU per cloud for ~2.9 ms whatever the batch size, longer than the eval-mode forward of a
    batch of 32 chunks (2.5 ms): planned one batch at a time it bounds a forward-only loop, planned for two batches at once it takes
    64 of the 256 CUs for the same 2.9 ms and the loop is bound by the forward itself.  Same idea as scene.infer_scene (all chunks of
    a scene in one plan).  Each batch gets its slice of the plan; batches that already carry one, or with another point count, are
    planned on their own."""
    net = model.module if hasattr(model, 'module') else model
    todo = [b for b in batches if 'geometry_plan' not in b and b['points'].is_cuda]
    same = len({(b['points'].size(2), b['points'].device) for b in todo}) == 1
    training = net.training and torch.is_grad_enabled()
    if len(todo) < 2 or not same or training or not hasattr(net, 'net_3d') or sum(b['points'].size(0) for b in todo) > 256:
        for b in batches:
            prefetch_geometry(model, b)
        return batches
    pts = torch.cat([net3d_points(b) for b in todo]).transpose(1, 2).contiguous()
    plan = net.net_3d.plan_geometry(pts, stream=net._side_stream(pts.device), with_csr=False)
    lo = 0
    for b in todo:
        hi = lo + b['points'].size(0)
        b['geometry_plan'] = net.net_3d.slice_plan(plan, lo, hi)
        lo = hi
    return batches


PREFETCH_AT = os.environ.get('MVP_PREFETCH_AT', 'backward')  # where train_step starts the next batch's geometry: 'backward' | 'forward'


def train_step(model, loss_fn, optimizer, data_batch, scheduler=None, max_grad_norm=0.0, grad_sync=None, next_batch=None, marks=None):
    """One iteration of the reference loop (mvpnet/train_mvpnet_3d.py:158-180,287-288):
    zero_grad -> forward -> SegLoss -> backward -> [grad all-reduce] -> [clip] -> step -> scheduler.
    next_batch: the batch of the NEXT iteration (already on the device); its geometry is prefetched.
    marks: a callable(name) invoked at 'begin', 'fwd_end' (loss enqueued), 'bwd_begin' (just before loss.backward()), 'bwd_first' (from a
    hook on the logits' gradient: the first backward kernel is enqueued), 'bwd_end', 'end' -- a measurement aid (bench.py records HIP
    events on the training stream there: where the stream waits for the host shows up as time between two marks).
    The iteration's meters (:170-173) need nothing here: they ride on loss_fn -- SegLoss(meters=metric.DeviceMeters(...)) updates them
    in the loss launch, without a host synchronisation."""
    if marks is not None:
        marks('begin')
    optimizer.zero_grad()
    if next_batch is not None and PREFETCH_AT == 'forward':
        data_batch = dict(data_batch, prefetch_next=next_batch)  # launched right after this batch's lifting
    preds = model(data_batch)
    loss = loss_fn(preds, data_batch)['seg_loss']
    if marks is not None:
        marks('fwd_end')
        if preds['seg_logit'].requires_grad:
            preds['seg_logit'].register_hook(lambda g: marks('bwd_first'))
    if next_batch is not None and PREFETCH_AT == 'backward':
        # The next batch's coordinate-only work (FPS chain, ball queries, 3-NN, transposed indices: ~3 ms of side-stream kernels) starts
        # HERE, beside the backward pass, not beside the forward: the forward's deep levels are chains of 10-40 us kernels that the
        # geometry kernels delay badly (measured with HIP events: SA3 + SA4 forward 0.45 -> 1.20 ms beside them, the whole step
        # 7.6 -> 8.9 ms), the backward is dominated by 100-350 us kernels that share the chip gracefully.
        prefetch_geometry(model, next_batch)
        prefetch_features_2d(model, next_batch)  # (a frozen 2D branch only: its forward of the NEXT batch runs beside this backward pass)
    if marks is not None:
        marks('bwd_begin')
    loss.backward()
    if marks is not None:
        marks('bwd_end')
    if grad_sync is not None:
        grad_sync(weight_sum=getattr(loss_fn, 'last_weight_sum', None))  # == the gradient of ONE loss over the gathered batch
    if max_grad_norm > 0:
        nn.utils.clip_grad_norm_(model.parameters(), max_norm=max_grad_norm)
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    if marks is not None:
        marks('end')
    return loss.detach(), preds


def validate(model, loss_fn, batches, meters=None):
    """The validation pass of stage two and of the 3D baselines (mvpnet/train_mvpnet_3d.py:221-284, train_3d.py) over batches that are
    on the device already: model and loss_fn in eval mode under torch.no_grad() -- every module's training flag is put back afterwards,
    also when the body raises --, per batch the forward and loss_fn with `meters` attached (whatever loss_fn.meters was is re-attached
    afterwards), so the loss, the accuracy counts and the confusion matrix of a batch are ONE launch and nothing is synchronised in the
    loop.  The geometry of the batch after the current one is started (prefetch_geometry) before the current forward.
    batches: any iterable of batch dicts -- MVPNet3D's (scene.sample_train_batch) or the baselines' (scene.sample_train_batch_3d), e.g.
    a generator over scene.val_batches.  meters: a metric.DeviceMeters to continue; None makes a fresh one for the logits' class count
    and loss_fn.ignore_index.  -> the DeviceMeters (None when `batches` is empty and none was given): summary() reads the numbers the
    reference logs, meters()[i].global_avg is what VAL.METRIC selects (is_better)."""
    from . import metric
    flags = [(m, m.training) for m in list(model.modules()) + list(loss_fn.modules())]
    had = getattr(loss_fn, 'meters', None)
    model.eval()
    loss_fn.eval()
    try:
        with torch.no_grad():
            it = iter(batches)
            cur = next(it, None)
            while cur is not None:
                nxt = next(it, None)
                if nxt is not None:
                    prefetch_geometry(model, nxt)  # (a model without a 3D geometry plan, or a batch that carries one: nothing to do)
                preds = model(cur)
                if meters is None:
                    meters = metric.DeviceMeters(preds['seg_logit'].size(1), ignore_index=getattr(loss_fn, 'ignore_index', -100))
                loss_fn.meters = meters
                loss_fn(preds, cur)
                cur = nxt
    finally:
        loss_fn.meters = had
        for m, flag in flags:
            m.training = flag
    return meters


def is_better(metric_name, cur, best):
    """The best-checkpoint rule of train_mvpnet_3d.py:275-277: is the validation value `cur` of VAL.METRIC better than `best`?  None always
    loses (no best yet: anything is better; no current value: nothing is); a name that contains 'loss' is better when lower, everything
    else when higher."""
    if cur is None:
        return False
    if best is None:
        return True
    return cur < best if 'loss' in metric_name else cur > best


def _plan_tensors(plan):
    """The tensors of a geometry plan (PN2SSG.plan_geometry) in a fixed order."""
    return [t for g in plan['sa'] + plan['fp'] if g is not None for t in g]


class GraphedForward:
    """The eval-mode forward of one batch shape (geometry plan on the side stream + 2D network + lifting + aggregation + PN2SSG) replayed
    from ONE HIP graph.  A single chunk issued eagerly sits behind ~100 launches and the serial FPS chain (2.33 ms, of which the chain is
    1.55); replayed, the host submits one graph and the levels' kernels follow their per-level events at dispatch speed: 2.25 ms on an idle
    host (bench field `latency_ms_B1_graph`) -- the chain, not the launches, is what bounds one chunk; under host load the replay is immune.
    `batch`: a data dict as MVPNet3D.forward takes it (its tensors become the static inputs; keys starting with '_' are ignored);
    calling the object with another batch of the same shapes copies its tensors in and replays; returns the model's output dict (static
    tensors: clone what must outlive the next call).  The reference has no counterpart (test_mvpnet_3d.py:142-174 feeds chunk by chunk)."""

    COPY_KEYS = ('images', 'points', 'depth', 'cam_matrix', 'kinv', 'pose', 'pixel_box', 'image_xyz', 'knn_indices', 'flip', 'z_rot', 'feature')

    def __init__(self, model, batch, warmup=2):
        self.model = model
        net = model.module if hasattr(model, 'module') else model
        assert not net.training, 'GraphedForward captures the eval-mode forward (model.eval() first)'
        self.static = {k: (v.clone() if torch.is_tensor(v) and k in self.COPY_KEYS else v) for k, v in batch.items()
                       if k not in ('geometry_plan', 'prefetch_next') and not k.startswith('_')}
        dev = self.static['points'].device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():  # eager warm-up off the default stream (allocator, lazy module state, kernel attributes)
            for _ in range(warmup):
                model(dict(self.static))
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        R.weight_slices.refresh(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.preds = model(dict(self.static))

    def __call__(self, batch=None):
        if batch is not None:
            for k, v in batch.items():
                if k in self.COPY_KEYS and torch.is_tensor(v) and v.data_ptr() != self.static[k].data_ptr():
                    self.static[k].copy_(v)
        self.graph.replay()
        return self.preds


class GraphedTrainStep:
    """The training iteration of `train_step` with forward + loss + backward captured ONCE in a HIP graph
    (torch.cuda.CUDAGraph): ~400 kernel launches per step become one graph launch, so the step no longer depends on the
    host keeping up (8 ranks per node share the CPU) and the launch gaps between the many small kernels disappear.

    The graph holds, for fixed shapes: lifting of batch i -> FORK: FPS / ball query / 3-NN of batch i+1 on the side stream ->
    aggregation + PointNet++ of batch i with the geometry computed by the PREVIOUS replay -> loss -> backward -> JOIN -> copy
    of the new geometry into the static plan.  Gradient all-reduce, clipping, optimizer and scheduler stay eager after the
    replay (they are a handful of multi-tensor launches, and RCCL stays out of the capture) -- unless solver='captured'.

    solver='captured' (opt-in; needs optim.FusedAdam(capturable=True), scheduler None or an optim.DeviceMultiStepLR, and no grad_sync):
    the clip coefficient (optim.total_grad_norm, only when max_grad_norm > 0), optimizer.step(grad_scale=coef) and scheduler.step() are
    nodes of the graph behind the plan copy -- the step number and the learning rate live on the device, so every replay takes the next
    update --, and step() is the input copies and one replay.  The gradients are left UNSCALED: the coefficient is applied while the
    step kernel reads them (the deferred scale of FusedSGD.step(grad_scale=)), so `.grad` after a step holds the unclipped gradient.

    step(batch, next_batch) copies the two batches into the static input tensors (keys of the reference's data dict; the 2D
    feature map is produced inside the graph by model.net_2d) and replays.  Batches must arrive in sequence: `batch` of call
    i is `next_batch` of call i-1, as with train_step(..., next_batch=...).

    The iteration's meters ride on loss_fn (SegLoss(meters=metric.DeviceMeters(...))): their update is part of the captured loss launch --
    the window cursor lives on the device, so every replay advances it -- and nothing here changes for them.  The eager warm-up
    iterations of the constructor update them too: reset() the meters after building the step, and read() them after replays."""

    COPY_KEYS = ('images', 'points', 'seg_label', 'depth', 'cam_matrix', 'kinv', 'pose', 'pixel_box', 'image_xyz', 'knn_indices', 'flip', 'z_rot')

    def __init__(self, model, loss_fn, optimizer, batch, next_batch, scheduler=None, max_grad_norm=0.0, grad_sync=None, warmup=3,
                 geometry='captured', plan=None, solver='eager'):
        """plan: the static geometry plan of ANOTHER GraphedTrainStep of the same model and shapes (PipelinedTrainStep: several captured copies
        of the step replayed in turn hand the next batch's geometry to each other through one set of plan tensors).
        geometry='captured' (default): the fork / join of the next batch's coordinate-only work lives inside the graph (no per-step
        host work besides the replay: 3.8 ms of host time per step).  geometry='eager': only the training stream is captured; the
        FPS chain, ball queries, 3-NN and transposed indices of the NEXT batch (~40 launches) are issued eagerly on the side stream next
        to the replay and copied into the static plan afterwards.  Measured on an idle host (B = 32): 9.82 ms either way against
        9.43 ms for the plain eager step on the same box -- the replay itself, not the fork, is what trails the eager stream by 4 %."""
        assert geometry in ('eager', 'captured')
        self.geometry = geometry
        if solver not in ('eager', 'captured'):
            raise ValueError("GraphedTrainStep: solver is 'eager' or 'captured', not {!r}".format(solver))
        if solver == 'captured':
            from . import optim
            if not (isinstance(optimizer, optim.FusedAdam) and optimizer.capturable):
                raise ValueError("GraphedTrainStep(solver='captured') needs an optim.FusedAdam(capturable=True)")
            if scheduler is not None and not isinstance(scheduler, optim.DeviceMultiStepLR):
                raise ValueError("GraphedTrainStep(solver='captured') takes no scheduler or an optim.DeviceMultiStepLR (others write host floats)")
            if grad_sync is not None:
                raise ValueError("GraphedTrainStep(solver='captured') takes no grad_sync: the all-reduce stays out of the capture")
        self.solver = solver
        self.model, self.loss_fn, self.optimizer = model, loss_fn, optimizer
        self.scheduler, self.max_grad_norm, self.grad_sync = scheduler, max_grad_norm, grad_sync
        net = model.module if hasattr(model, 'module') else model
        self.static = {k: (v.clone() if torch.is_tensor(v) and k in self.COPY_KEYS else v) for k, v in batch.items()
                       if k not in ('geometry_plan', 'prefetch_next') and not k.startswith('_')}
        self.static_next = {k: next_batch[k].clone() for k in ('points', 'z_rot') if k in next_batch}  # what the geometry reads
        dev = self.static['points'].device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # eager warm-up off the default stream (allocator, lazy module state)
            for _ in range(warmup):
                optimizer.zero_grad(set_to_none=True)
                loss = loss_fn(model(dict(self.static)), self.static)['seg_loss']
                loss.backward()
            if plan is None:
                plan = net.net_3d.plan_geometry(self.static['points'].transpose(1, 2).contiguous())
                plan = {'sa': plan['sa'], 'fp': plan['fp'], 'event': None, 'stream': None}
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.plan = plan  # static geometry of the CURRENT batch
        if solver == 'captured':
            optimizer.materialize()  # moments, counts and device learning rates exist before the capture (the warm-up's gradients say which)
        optimizer.zero_grad(set_to_none=True)
        R.weight_slices.refresh(dev)  # the slice table exists before the capture: the refresh launch becomes a node of the graph
        self.graph = torch.cuda.CUDAGraph()
        # the weight gradients stay on the captured stream: inside a graph the extra fork / join edges cost more than the overlap
        # returns (measured B = 32: 9.25 ms captured without them, 9.72 ms with -- MVP_GRAPH_DW_SIDE=1 --; the eager step gains 0.2 ms from them)
        aside = R.DW_SIDE_STREAM
        R.DW_SIDE_STREAM = aside and os.environ.get('MVP_GRAPH_DW_SIDE', '0') == '1'
        try:
            self._capture(model, loss_fn, dev, geometry)
        finally:
            R.DW_SIDE_STREAM = aside
        # the gradients the replay writes (tensors of this graph's pool); `rebind`: another captured copy of the step shares the parameters, so
        # before the eager tail (all-reduce, clipping, optimizer) reads `.grad` it must point at THIS copy's tensors again
        self.grads = [(p, p.grad) for p in model.parameters() if p.grad is not None]
        self.rebind = False

    def _capture(self, model, loss_fn, dev, geometry):
        with torch.cuda.graph(self.graph):
            if geometry == 'captured':
                nxt = dict(self.static_next)
                preds = model(dict(self.static, geometry_plan=self.plan, prefetch_next=nxt))
            else:
                preds = model(dict(self.static, geometry_plan=self.plan))
            self.loss = loss_fn(preds, self.static)['seg_loss']
            self.loss.backward()
            if geometry == 'captured':
                new_plan = nxt['geometry_plan']
                torch.cuda.current_stream(dev).wait_event(new_plan['event'])  # join the side stream
                for dst, src in zip(_plan_tensors(self.plan), _plan_tensors(new_plan)):
                    dst.copy_(src)
            self.preds = preds
            if self.solver == 'captured':
                from . import optim
                coef = None
                if self.max_grad_norm > 0:
                    self.grad_norm, coef = optim.total_grad_norm(list(model.parameters()), self.max_grad_norm)
                self.optimizer.step(grad_scale=coef)
                if self.scheduler is not None:
                    self.scheduler.step()

    def step(self, batch=None, next_batch=None):
        if batch is not None:
            for k, v in batch.items():
                if k in self.COPY_KEYS and torch.is_tensor(v) and v.data_ptr() != self.static[k].data_ptr():
                    self.static[k].copy_(v)
        if next_batch is not None:
            for k, dst in self.static_next.items():
                if next_batch[k].data_ptr() != dst.data_ptr():
                    dst.copy_(next_batch[k])
        if self.geometry == 'eager':
            # geometry of the next batch on the side stream, eagerly, next to the replay; handed over after it
            net = self.model.module if hasattr(self.model, 'module') else self.model
            new_plan = prefetch_geometry(self.model, dict(self.static_next))['geometry_plan']
            self.graph.replay()
            cur = torch.cuda.current_stream(self.static['points'].device)
            cur.wait_event(new_plan['event'])
            dst, src = _plan_tensors(self.plan), _plan_tensors(new_plan)
            for dt in {t.dtype for t in dst}:
                torch._foreach_copy_([d for d in dst if d.dtype == dt], [x for d, x in zip(dst, src) if d.dtype == dt])
            del net
        else:
            self.graph.replay()
        if self.solver == 'captured':
            return self.loss.detach(), self.preds
        if self.rebind:
            for p, g in self.grads:
                p.grad = g
        if self.grad_sync is not None:
            self.grad_sync(weight_sum=getattr(self.loss_fn, 'last_weight_sum', None))
        if self.max_grad_norm > 0:
            nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=self.max_grad_norm)
        self.optimizer.step()
        if self.scheduler is not None:
            self.scheduler.step()
        return self.loss.detach(), self.preds


class PipelinedTrainStep:
    """`depth` captured copies of the training step (GraphedTrainStep) replayed in turn: the host can enqueue step i + 1 (input copies, the
    graph launch of ~190 nodes, the optimizer launch) while copy A's replay of step i still runs, whatever the runtime does with a second
    launch of one executable graph.  Everything stays in order on ONE stream (inputs of copy B are copied behind copy A's replay and optimizer
    launch); the copies share the parameters, the optimizer state and the static geometry plan (copy A's replay writes the plan of batch
    i + 1 that copy B's replay reads); each has its own static inputs and gradient tensors (`rebind`).
    Measured (bench field per_gpu_batch, `graph_x2`): at 4 chunks per GPU -- the reference's partition of its batch of 32
    over 8 GPUs, train_mvpnet_3d.py:68-70 -- 2.73 ms against 2.71 for one copy: the replay is GPU-bound there (2.09 ms of kernels on the
    training stream), the host needs 0.7 ms per step and runs ahead either way.  Kept as the measurement it is and for hosts slower than the
    replay.  step(batch, next_batch) as GraphedTrainStep.step: batches arrive in sequence."""

    def __init__(self, model, loss_fn, optimizer, batch, next_batch, depth=2, **kw):
        first = GraphedTrainStep(model, loss_fn, optimizer, batch, next_batch, **kw)
        kw = dict(kw, warmup=0)
        self.copies = [first] + [GraphedTrainStep(model, loss_fn, optimizer, batch, next_batch, plan=first.plan, **kw) for _ in range(depth - 1)]
        for c in self.copies:
            c.rebind = len(self.copies) > 1
        self.turn = 0

    def step(self, batch=None, next_batch=None):
        c = self.copies[self.turn]
        self.turn = (self.turn + 1) % len(self.copies)
        return c.step(batch, next_batch)

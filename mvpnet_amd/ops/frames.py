"""The picked frames of a raw uint8 store as the 2D network reads them, on the device (new: the reference prepares every frame in a
data-loader worker -- T.ColorJitter on the PIL image, `/ 255.`, `(image - mean) / std`, np.fliplr: mvpnet/data/scannet_2d3d.py:241-252,
:293-296, mvpnet/data/scannet_2d.py:158-171)."""
import torch

from .. import _lib as L

_MEAN_STD = {}  # (device, mean, std) -> the 6 floats on the device: uploaded once, so a call makes no host-to-device copy


def _mean_std(normalizer, dev):
    if normalizer is None:
        return None
    mean, std = normalizer
    key = (dev, tuple(float(v) for v in mean), tuple(float(v) for v in std))
    if len(key[1]) != 3 or len(key[2]) != 3:
        raise RuntimeError('prepare_frames: normalizer must be (mean, std) with three numbers each')
    t = _MEAN_STD.get(key)
    if t is None:
        t = _MEAN_STD[key] = torch.tensor(key[1] + key[2], dtype=torch.float32).to(dev)
    return t


def prepare_frames(frames, picked, factor=None, order=None, flip=None, normalizer=None, channels_last=False):
    """frames (Ftot,H,W,3) uint8 RGB as a PNG decodes and picked (any shape) int64 global rows, on the device -> float32
    picked.shape + (3,H,W): the picked frames after the colour jitter, `/ 255.`, the normalisation and the horizontal flip, two launches
    (one without a jitter), no host synchronisation.
    factor picked.shape + (3,) float32 (brightness, contrast, saturation) and order picked.shape + (3,) uint8 -- the op applied i-th, 0 / 1
    / 2 in that numbering, any other value = no step --, both or neither (augment.draw_color_jitter draws them); flip picked.shape uint8 /
    bool or None; normalizer: the YAML's (mean, std) or None; channels_last: the same logical shape with
    (...,H,W,3) memory, as a channels-last 2D network reads it.  Rows outside [0, Ftot) are clamped.
    The first call with a given normalizer on a device uploads its six floats (a host-to-device copy) and keeps them: make one call
    before capturing the op in a graph.
    Definition (pinned; for given factors and order bit-identical to PIL's ImageEnhance chain): include/mvp_hip.h, mvp_prepare_frames_u8."""
    L.require_gpu(frames, picked, factor, order, flip)
    if frames.dim() != 4 or frames.size(3) != 3 or frames.dtype != torch.uint8 or frames.size(0) < 1 or frames.size(1) < 1 or frames.size(2) < 1:
        raise RuntimeError('prepare_frames: frames must be (Ftot,H,W,3) uint8 with Ftot, H, W >= 1')
    dev = frames.device
    if picked.dtype != torch.int64 or picked.device != dev:
        raise RuntimeError('prepare_frames: picked must be int64 on the frames\' device')
    if (factor is None) != (order is None):
        raise RuntimeError('prepare_frames: factor and order go together')
    shape = tuple(picked.shape)
    if factor is not None:
        if factor.dtype != torch.float32 or tuple(factor.shape) != shape + (3,) or factor.device != dev:
            raise RuntimeError('prepare_frames: factor must be picked.shape + (3,) float32 on the frames\' device')
        if order.dtype != torch.uint8 or tuple(order.shape) != shape + (3,) or order.device != dev:
            raise RuntimeError('prepare_frames: order must be picked.shape + (3,) uint8 on the frames\' device')
    if flip is not None and (flip.dtype not in (torch.uint8, torch.bool) or tuple(flip.shape) != shape or flip.device != dev):
        raise RuntimeError('prepare_frames: flip must be picked.shape uint8 or bool on the frames\' device')
    Ftot, H, W = frames.size(0), frames.size(1), frames.size(2)
    if H * W * 3 >= 2 ** 31:
        raise RuntimeError('prepare_frames: a frame must stay below 2^31 bytes')
    ms = _mean_std(normalizer, dev)
    Nf = picked.numel()
    out = torch.empty((Nf, H, W, 3) if channels_last else (Nf, 3, H, W), dtype=torch.float32, device=dev)
    if Nf:
        ws = torch.empty(L.lib().mvp_prepare_frames_workspace(Nf) // 8, dtype=torch.int64, device=dev) if order is not None else None
        L.call('mvp_prepare_frames_u8', frames, L.ptr(frames), Ftot, H, W, L.ptr(picked), Nf, L.ptr(factor), L.ptr(order), L.ptr(flip), L.ptr(ms),
               int(bool(channels_last)), L.ptr(out), L.ptr(ws))
    if channels_last:
        return out.view(shape + (H, W, 3)).permute(*range(len(shape)), len(shape) + 2, len(shape), len(shape) + 1)
    return out.view(shape + (3, H, W))

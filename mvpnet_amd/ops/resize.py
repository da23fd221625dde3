"""The loader steps of the 2D stage that change an image's size, on the device (new: the reference calls Pillow per frame in a
data-loader worker -- `image.resize(size, Image.BILINEAR)`, `label.resize(size, Image.NEAREST)`, `label_mapping[label]`, F.hflip:
mvpnet/data/scannet_2d.py:153-168, mvpnet/data/scannet_2d3d.py:234-239)."""
import ctypes

import numpy as np
import torch

from .. import _lib as L

_BILINEAR = {}  # (device, inS, outS) -> the axis' int32 table on the device [xmin | count | coef]: uploaded once, a later call copies nothing
_NEAREST = {}   # (device, inS, outS) -> the axis' int32 source indices on the device


def _int32_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bilinear_table(inS, outS):
    """Pillow's coefficient table of one axis for the triangle filter, from the library's host function (no GPU): xmin (outS,), count
    (outS,), coef (outS, ksize) int32 and ksize.  Definition: include/mvp_hip.h, mvp_resize_bilinear_table."""
    fn = L.lib().mvp_resize_bilinear_table
    ksize = ctypes.c_int32(0)
    L.check(fn(int(inS), int(outS), None, None, None, ctypes.byref(ksize)), 'mvp_resize_bilinear_table')
    xmin, count = np.zeros(outS, np.int32), np.zeros(outS, np.int32)
    coef = np.zeros((outS, ksize.value), np.int32)
    L.check(fn(int(inS), int(outS), _int32_ptr(xmin), _int32_ptr(count), _int32_ptr(coef), ctypes.byref(ksize)), 'mvp_resize_bilinear_table')
    return xmin, count, coef, int(ksize.value)


def nearest_table(inS, outS):
    """The source index of every output index of one axis, Pillow's NEAREST on a 16-bit image (host, no GPU): (outS,) int32."""
    index = np.zeros(outS, np.int32)
    L.check(L.lib().mvp_resize_nearest_table(int(inS), int(outS), _int32_ptr(index)), 'mvp_resize_nearest_table')
    return index


def _bilinear_on(dev, inS, outS):
    if inS == outS:
        return None
    t = _BILINEAR.get((dev, inS, outS))
    if t is None:
        xmin, count, coef, _ = bilinear_table(inS, outS)
        t = _BILINEAR[(dev, inS, outS)] = torch.from_numpy(np.concatenate([xmin, count, coef.ravel()])).to(dev)
    return t


def _nearest_on(dev, inS, outS):
    if inS == outS:
        return None
    t = _NEAREST.get((dev, inS, outS))
    if t is None:
        t = _NEAREST[(dev, inS, outS)] = torch.from_numpy(nearest_table(inS, outS)).to(dev)
    return t


def _size(who, size, H, W):
    if size is None:
        return H, W
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise RuntimeError(who + ': size must be PIL\'s (w, h), both >= 1')
    return int(size[1]), int(size[0])


def resize_frames(frames, picked, size):
    """frames (Ftot,H,W,3) uint8 RGB and picked (any shape) int64 global rows, on the device; size = PIL's (w, h), as in the YAML -> uint8
    picked.shape + (h,w,3): `Image.fromarray(frame).resize(size, Image.BILINEAR)` of the picked frames, bit for bit, in one launch and
    without a host synchronisation.  Pillow's two passes, horizontal then vertical, the intermediate rounded to uint8 (kept in LDS); with
    one axis unchanged only the other pass runs, with both unchanged the frames are copied.  Rows outside [0, Ftot) are clamped.
    The first call with a given size pair on a device builds the two coefficient tables on the host and uploads them (a host-to-device
    copy), later calls copy nothing: make one call before capturing the op in a graph.
    Accepted sizes and the definition: include/mvp_hip.h, mvp_resize_frames_u8 (a reduction beyond ~21x raises)."""
    L.require_gpu(frames, picked)
    if frames.dim() != 4 or frames.size(3) != 3 or frames.dtype != torch.uint8 or frames.size(0) < 1 or frames.size(1) < 1 or frames.size(2) < 1:
        raise RuntimeError('resize_frames: frames must be (Ftot,H,W,3) uint8 with Ftot, H, W >= 1')
    dev = frames.device
    if picked.dtype != torch.int64 or picked.device != dev:
        raise RuntimeError('resize_frames: picked must be int64 on the frames\' device')
    Ftot, H, W = frames.size(0), frames.size(1), frames.size(2)
    h, w = _size('resize_frames', size, H, W)
    if max(H, h) * max(W, w) * 3 >= 2 ** 31:
        raise RuntimeError('resize_frames: a frame must stay below 2^31 bytes')
    shape, Nf = tuple(picked.shape), picked.numel()
    out = torch.empty((Nf, h, w, 3), dtype=torch.uint8, device=dev)
    if Nf:
        xtab, ytab = _bilinear_on(dev, W, w), _bilinear_on(dev, H, h)
        L.call('mvp_resize_frames_u8', frames, L.ptr(frames), Ftot, H, W, L.ptr(picked), Nf, h, w, L.ptr(xtab), L.ptr(ytab), L.ptr(out))
    return out.view(shape + (h, w, 3))


def prepare_labels(labels, picked, size=None, flip=None, mapping=None, ignore_value=-100):
    """labels (Ftot,H,W) uint16 raw ids as the label PNGs decode and picked (any shape) int64 global rows, on the device -> int64
    picked.shape + (h,w): `label.resize(size, Image.NEAREST)` (Pillow's rule for 16-bit images), the horizontal flip and
    `label_mapping[label]` of the picked label images in one launch, no host synchronisation.
    size: PIL's (w, h) or None (the store's size); flip picked.shape uint8 / bool or None -- the SAME draw the image got; mapping (T,)
    int64 on the device (config.scannet_label_mapping) or None for the raw ids; a raw id >= T gives ignore_value.  Rows outside [0, Ftot)
    are clamped.  The first call with a given size pair on a device uploads its two index tables and keeps them.
    Definition: include/mvp_hip.h, mvp_prepare_labels_u16."""
    L.require_gpu(labels, picked, flip, mapping)
    if labels.dim() != 3 or labels.dtype != torch.uint16 or labels.size(0) < 1 or labels.size(1) < 1 or labels.size(2) < 1:
        raise RuntimeError('prepare_labels: labels must be (Ftot,H,W) uint16 with Ftot, H, W >= 1')
    dev = labels.device
    if picked.dtype != torch.int64 or picked.device != dev:
        raise RuntimeError('prepare_labels: picked must be int64 on the labels\' device')
    shape = tuple(picked.shape)
    if flip is not None and (flip.dtype not in (torch.uint8, torch.bool) or tuple(flip.shape) != shape or flip.device != dev):
        raise RuntimeError('prepare_labels: flip must be picked.shape uint8 or bool on the labels\' device')
    if mapping is not None and (mapping.dtype != torch.int64 or mapping.dim() != 1 or mapping.device != dev):
        raise RuntimeError('prepare_labels: mapping must be (T,) int64 on the labels\' device')
    Ftot, H, W = labels.size(0), labels.size(1), labels.size(2)
    h, w = _size('prepare_labels', size, H, W)
    if H * W >= 2 ** 31 or h * w >= 2 ** 31:
        raise RuntimeError('prepare_labels: a label image must stay below 2^31 pixels')
    Nf = picked.numel()
    out = torch.empty((Nf, h, w), dtype=torch.int64, device=dev)
    if Nf:
        L.call('mvp_prepare_labels_u16', labels, L.ptr(labels), Ftot, H, W, L.ptr(picked), Nf, h, w, L.ptr(_nearest_on(dev, H, h)),
               L.ptr(_nearest_on(dev, W, w)), L.ptr(flip), L.ptr(mapping), 0 if mapping is None else mapping.numel(), int(ignore_value), L.ptr(out))
    return out.view(shape + (h, w))

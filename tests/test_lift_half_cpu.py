"""16-bit feature maps and stores, the host side (no GPU): the `_h16` entry points refuse a null feature, an unknown feature_type and a
misaligned feature before any HIP call; scene._frame_store builds a bfloat16 store; UNetResNet34.frozen_inference hands out the bfloat16
feature map it computed."""
import ctypes

import pytest
import torch

ENULL, EINVAL = -3, -1


def _entries():
    """name -> call(feature pointer, feature_type): every other operand a dummy address that no check objects to.  A precondition failure
    returns before any HIP call, so nothing here is ever dereferenced."""
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    B, nv, h, w, N, C, k = 2, 3, 30, 40, 300, 64, 3
    return {
        'mvp_lift_h16': lambda f, ft: lib.mvp_lift_h16(d, 1, d, d, d, None, d, f, ft, B, nv, h, w, N, C, k, d, d, d, d, None, None, None),
        'mvp_lift_aug_h16': lambda f, ft: lib.mvp_lift_aug_h16(d, 1, d, d, d, None, d, f, ft, B, nv, h, w, N, C, k, d, d, d, d, None, None, d, d, d,
                                                               None),
        'mvp_lift_store_h16': lambda f, ft: lib.mvp_lift_store_h16(d, 1, d, d, d, None, d, f, ft, d, 4, B, nv, h, w, N, C, k, d, d, d, d, None),
        'mvp_lift_gather_h16': lambda f, ft: lib.mvp_lift_gather_h16(f, ft, d, d, B, nv * h * w, C, N, k, d, d, None),
    }


@pytest.mark.parametrize('name', ['mvp_lift_h16', 'mvp_lift_aug_h16', 'mvp_lift_store_h16', 'mvp_lift_gather_h16'])
def test_argument_errors_do_not_launch(name):
    from mvpnet_amd import _lib
    assert (_lib.LIMITS['MVP_FEATURE_BF16'], _lib.LIMITS['MVP_FEATURE_F16']) == (1, 2)
    assert name in _lib.EXPORTS
    call = _entries()[name]
    aligned = ctypes.c_void_p(32)
    for feature_type in (1, 2):
        assert call(None, feature_type) == ENULL
        for misaligned in (ctypes.c_void_p(32 + 8), ctypes.c_void_p(32 + 2)):
            assert call(misaligned, feature_type) == EINVAL
    for feature_type in (0, 3):
        assert call(aligned, feature_type) == EINVAL
        assert call(None, feature_type) == ENULL   # a null pointer outranks an invalid argument, as everywhere in the library


def test_the_fused_entries_refuse_a_channel_count_that_is_no_multiple_of_four():
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    B, nv, h, w, N, k = 2, 3, 30, 40, 300, 3
    for C in (6, 2, 63):
        assert lib.mvp_lift_h16(d, 1, d, d, d, None, d, d, 1, B, nv, h, w, N, C, k, d, d, d, d, None, None, None) == EINVAL
        assert lib.mvp_lift_aug_h16(d, 1, d, d, d, None, d, d, 2, B, nv, h, w, N, C, k, d, d, d, d, None, None, d, d, d, None) == EINVAL
        assert lib.mvp_lift_store_h16(d, 1, d, d, d, None, d, d, 1, d, 4, B, nv, h, w, N, C, k, d, d, d, d, None) == EINVAL


def test_the_derived_signatures_carry_the_feature_type():
    from ctypes import c_int, c_int64, c_void_p
    from mvpnet_amd import _lib as L
    p, i64 = c_void_p, c_int64
    assert L._SIGNATURES['mvp_lift_h16'] == [p, c_int] + [p] * 6 + [c_int] + [i64] * 7 + [p] * 7
    assert L._SIGNATURES['mvp_lift_aug_h16'] == [p, c_int] + [p] * 6 + [c_int] + [i64] * 7 + [p] * 10
    assert L._SIGNATURES['mvp_lift_store_h16'] == [p, c_int] + [p] * 6 + [c_int, p] + [i64] * 8 + [p] * 5
    assert L._SIGNATURES['mvp_lift_gather_h16'] == [p, c_int, p, p] + [i64] * 5 + [p] * 3
    for name in ('mvp_lift_f32', 'mvp_lift_aug_f32', 'mvp_lift_store_f32', 'mvp_lift_gather_f32'):   # the siblings: one c_int fewer
        assert len(L._SIGNATURES[name]) + 1 == len(L._SIGNATURES[name[:-4] + '_h16'])


def test_ops_refuse_a_half_feature_that_needs_a_gradient_before_anything_else():
    """(CPU tensors: the forward-only refusal comes first and names the way out.)"""
    import mvpnet_amd.ops as ops
    feat = torch.zeros(1, 2, 4, 4, 8, dtype=torch.bfloat16, requires_grad=True)
    depth, cam, pose, pts = torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 4, 4), torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match=r'forward only.*feature\.float\(\)'):
        ops.lift(feat, depth, cam, cam, pose, pts)
    with pytest.raises(RuntimeError, match=r'forward only.*feature\.float\(\)'):
        ops.lift_gather(feat, None, torch.zeros(1, 5, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError):   # without a gradient it is a CPU tensor like any other: no fallback
        ops.lift(feat.detach(), depth, cam, cam, pose, pts)


# ---- scene._frame_store -------------------------------------------------------------------------------------------------------------
F, H, W, C, FRAMES = 6, 4, 5, 8, [0, 2, 3, 5]


class _Net(torch.nn.Module):
    def __init__(self, dtype=None):
        super().__init__()
        self.dtype = dtype

    def forward(self, data):
        x = data['image']
        out = torch.stack([x[:, 0] * (c + 1) + x[:, 1] * 0.37 - x[:, 2] for c in range(C)], 1)
        return {'out': out if self.dtype is None else out.to(self.dtype)}


def _store(net, dtype):
    from mvpnet_amd import scene as S
    images = torch.randn(F, 3, H, W, generator=torch.Generator().manual_seed(4))
    run = S._frames_through(net, 'out', images, None, False)
    store, slot_of = S._frame_store(FRAMES, F, H, W, 3, run, 'test', torch.device('cpu'), None, dtype=dtype)
    return store, slot_of, net({'image': images[FRAMES]})['out']


def test_a_bfloat16_frame_store():
    store, slot_of, out = _store(_Net(), torch.bfloat16)
    assert out.dtype == torch.float32
    assert store.dtype == torch.bfloat16 and tuple(store.shape) == (len(FRAMES), H, W, C) and store.is_contiguous()
    want = out.to(torch.bfloat16).permute(0, 2, 3, 1)   # one rounding to nearest even
    assert torch.equal(store.view(torch.int16), want.contiguous().view(torch.int16))
    assert not torch.equal(store.float(), out.permute(0, 2, 3, 1)), 'the float32 outputs are no bfloat16 values: the store is a lossy opt-in'
    assert slot_of.tolist() == [FRAMES.index(f) if f in FRAMES else -1 for f in range(F)]
    # a network that already returns bfloat16: copied as it is
    store2, _, out2 = _store(_Net(torch.bfloat16), torch.bfloat16)
    assert out2.dtype == torch.bfloat16 and store2.dtype == torch.bfloat16
    assert torch.equal(store2.view(torch.int16), out2.permute(0, 2, 3, 1).contiguous().view(torch.int16))
    # ... and one that returns the other 16-bit type is refused, as is any 16-bit output by default
    with pytest.raises(RuntimeError, match='test: net_2d must return a float32'):
        _store(_Net(torch.float16), torch.bfloat16)
    with pytest.raises(RuntimeError, match='test: net_2d must return a float32'):
        _store(_Net(torch.bfloat16), None)
    with pytest.raises(RuntimeError):
        _store(_Net(), torch.float64)
    assert _store(_Net(), None)[0].dtype == torch.float32


# ---- UNetResNet34.frozen_inference --------------------------------------------------------------------------------------------------
def test_frozen_inference_hands_out_the_bfloat16_feature_map():
    from mvpnet_amd.unet_resnet34 import UNetResNet34
    torch.manual_seed(0)
    net = UNetResNet34(20)
    image = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        wide = net.frozen_inference(compute_dtype=torch.bfloat16)({'image': image})
        assert '_feature_dtype' not in net.__dict__
        half = net.frozen_inference(compute_dtype=torch.bfloat16, feature_dtype=torch.bfloat16)({'image': image})
    assert wide['feature'].dtype == torch.float32 and wide['seg_logit'].dtype == torch.float32
    assert half['feature'].dtype == torch.bfloat16 and half['seg_logit'].dtype == torch.float32
    assert tuple(half['feature'].shape) == (2, 64, 32, 48) and half['feature'].permute(0, 2, 3, 1).is_contiguous(), 'channels-last'
    assert torch.equal(half['feature'].float().view(torch.int32), wide['feature'].view(torch.int32))
    assert torch.equal(half['seg_logit'].view(torch.int32), wide['seg_logit'].view(torch.int32))
    for compute, feature in ((None, torch.bfloat16), (torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16),
                             (torch.float32, torch.float32), (torch.bfloat16, torch.float32)):
        with pytest.raises(ValueError):
            net.frozen_inference(compute_dtype=compute, feature_dtype=feature)
    # whoever sets the private compute type alone (the benchmark does) keeps getting float32 features
    net.frozen_inference()
    net.__dict__['_fast_dtype'] = torch.bfloat16
    with torch.no_grad():
        assert net({'image': image})['feature'].dtype == torch.float32
    net.frozen_inference(compute_dtype=torch.bfloat16, feature_dtype=torch.bfloat16).unfreeze()
    assert '_feature_dtype' not in net.__dict__ and '_fast_dtype' not in net.__dict__

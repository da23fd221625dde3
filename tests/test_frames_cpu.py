"""Frames on the device, the parts that need no GPU: the NumPy oracle of mvp_prepare_frames_u8 (tests/frames_oracle.py) against vectors
made by PIL's ImageEnhance (tests/golden/frames.npz, tests/golden/make_frames_golden.py), its normalisation against the reference's
NumPy expression, the law of augment.draw_color_jitter on the CPU, config.build_color_jitter and the entry's argument errors."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from tests import frames_oracle as FO
from tests.conftest import ROOT

GROUPS = ('s5x7', 's6x8', 's120x160')
NORMALIZER = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))  # mvpnet/config/mvpnet_3d.py:26


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'frames.npz'))


def test_the_golden_file_holds_the_cases_it_should(golden):
    assert golden['s5x7_images'].shape[1:] == (5, 7, 3) and golden['s6x8_images'].shape[1:] == (6, 8, 3)
    assert golden['s120x160_images'].shape == (1, 120, 160, 3)
    for g in ('s5x7', 's6x8'):
        orders = {tuple(o) for o in golden[g + '_order']}
        assert set(itertools.permutations((0, 1, 2))) <= orders                                       # all six
        assert {(0, 3, 3), (1, 3, 3), (2, 3, 3)} <= orders and any(o.count(3) == 1 for o in orders)     # single-op and two-op
        f = golden[g + '_factor']
        assert (f < 1).any() and (f > 1).any() and (f == 1).all(1).any()
        assert (golden[g + '_out'] == 255).any()                                                        # the clip is hit
    half = golden['s6x8_images'][4]                                                                     # mean grey exactly k + 0.5
    assert FO.gray(half).sum() * 2 == (2 * 101 + 1) * 48 and FO.mean_gray(half) == 102
    unchanged = (golden['s6x8_factor'] == 1).all(1)
    assert np.array_equal(golden['s6x8_out'][unchanged], golden['s6x8_images'][golden['s6x8_case_image'][unchanged]])


@pytest.mark.parametrize('g', GROUPS)
def test_oracle_equals_pil_bit_for_bit(golden, g):
    images, idx, factor, order, out = (golden[g + '_' + k] for k in ('images', 'case_image', 'factor', 'order', 'out'))
    assert len(out) >= 3
    for i in range(len(out)):
        got = FO.jitter(images[idx[i]], factor[i], order[i])
        assert np.array_equal(got, out[i]), (g, i, factor[i], order[i], int((got != out[i]).sum()))


def test_integer_mean_equals_pils_double_rounding():
    """m = (2S + n) / (2n) against int(S / n + 0.5) in double, at sums on and around every half step"""
    for n in (35, 48, 19200, 640 * 480):
        for k in (0, 1, 100, 101, 254):
            for d in (-1, 0, 1):
                s = (2 * k + 1) * n // 2 + d
                if 0 <= s <= 255 * n:
                    assert (2 * s + n) // (2 * n) == int(s / n + 0.5), (n, s)


def test_normalisation_equals_the_reference_expression_for_every_byte():
    """mvpnet/data/scannet_2d3d.py:246-251 on all 3 x 256 (channel, byte) pairs"""
    image = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)  # (256,1,3): byte u in every channel
    ref = np.asarray(image, dtype=np.float32) / 255.
    assert ref.dtype == np.float32
    assert np.array_equal(FO.value_table(None).T, ref[:, 0])
    mean, std = NORMALIZER
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    ref = (ref - mean) / std
    assert ref.dtype == np.float32
    assert np.array_equal(FO.value_table(mean.tolist() + std.tolist()).T, ref[:, 0])
    got = FO.prepare_frames(image[None], [0], mean_std=np.concatenate([mean, std]))
    assert np.array_equal(got[0], ref.transpose(2, 0, 1))


def test_oracle_flip_and_layouts(golden):
    frames = golden['s5x7_images']
    a = FO.prepare_frames(frames, [1, 0], flip=[1, 0])
    b = FO.prepare_frames(frames, [1, 0])
    assert np.array_equal(a[0], b[0][:, :, ::-1]) and np.array_equal(a[1], b[1])
    c = FO.prepare_frames(frames, [1, 0], flip=[1, 0], channels_last=True)
    assert np.array_equal(c.transpose(0, 3, 1, 2), a)
    assert np.array_equal(FO.prepare_frames(frames, [99, -4]), FO.prepare_frames(frames, [len(frames) - 1, 0]))  # clamped


def test_draws_on_the_cpu():
    from mvpnet_amd.augment import draw_color_jitter, draw_flip
    gen = torch.Generator().manual_seed(5)
    factor, order = draw_color_jitter(600, (0.4, 0.4, 0.4), 'cpu', generator=gen)
    assert factor.shape == (600, 3) and factor.dtype == torch.float32 and order.shape == (600, 3) and order.dtype == torch.uint8
    assert float(factor.min()) >= np.float32(0.6) and float(factor.max()) <= np.float32(1.4)
    assert (order.sort(dim=1).values == torch.tensor([0, 1, 2], dtype=torch.uint8)).all()
    assert len({tuple(o) for o in order.tolist()}) == 6
    factor, order = draw_color_jitter((4, 3), (0.4, 0.0, 1.5), 'cpu', generator=gen)
    assert factor.shape == (4, 3, 3) and order.shape == (4, 3, 3)
    assert (factor[..., 1] == 1).all() and float(factor[..., 2].min()) >= 0 and float(factor[..., 2].max()) <= 2.5
    assert (order[..., 2] == 3).all() and (order[..., :2].sort(dim=-1).values == torch.tensor([0, 2], dtype=torch.uint8)).all()
    factor, order = draw_color_jitter(3, (0, 0, 0, 0), 'cpu')
    assert (factor == 1).all() and (order == 3).all()
    with pytest.raises(ValueError):
        draw_color_jitter(3, (0.4, 0.4, 0.4, 0.1), 'cpu')
    with pytest.raises(ValueError):
        draw_color_jitter(3, (0.4, 0.4), 'cpu')
    flags = draw_flip((50, 3), 0.5, 'cpu', generator=gen)
    assert flags.shape == (50, 3) and flags.dtype == torch.uint8 and 0 < int(flags.sum()) < 150
    assert int(draw_flip(10, 0.0, 'cpu').sum()) == 0


def test_build_color_jitter():
    from mvpnet_amd.config import build_color_jitter

    class Node(dict):
        __getattr__ = dict.__getitem__
    cfg = Node(DATASET=Node(ScanNet2D3DChunks=Node(augmentation=Node(color_jitter=(0.4, 0.4, 0.4), flip=0.5))))
    assert build_color_jitter(cfg, True) == (0.4, 0.4, 0.4) and build_color_jitter(cfg, False) == ()
    assert build_color_jitter(Node(DATASET=Node(ScanNet2D3DChunks=Node(augmentation=Node(color_jitter=())))), True) == ()
    assert build_color_jitter(Node(DATASET=Node()), True) == ()


def test_prepare_frames_refuses_cpu_tensors_and_bad_arguments():
    import mvpnet_amd.ops as ops
    from mvpnet_amd import _lib
    with pytest.raises(RuntimeError):
        ops.prepare_frames(torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))
    lib = _lib.lib()
    d = ctypes.c_void_p(16)
    call = lambda *a: lib.mvp_prepare_frames_u8(*a)
    assert call(d, 4, 0, 8, d, 1, None, None, None, None, 0, d, None, None) == -1      # H < 1
    assert call(d, 4, 8, 0, d, 1, None, None, None, None, 0, d, None, None) == -1      # W < 1
    assert call(d, 4, 8, 8, d, 0, None, None, None, None, 0, d, None, None) == -1      # Nf < 1
    assert call(d, 4, 8, 8, d, 1, d, None, None, None, 0, d, d, None) == -1            # factor without order
    assert call(d, 4, 8, 8, d, 1, None, d, None, None, 0, d, d, None) == -1            # order without factor
    assert call(d, 4, 1 << 15, 1 << 15, d, 1, None, None, None, None, 0, d, None, None) == -2   # H*W*3 >= 2^31
    assert call(None, 4, 8, 8, d, 1, None, None, None, None, 0, d, None, None) == -3
    assert lib.mvp_prepare_frames_workspace(96) >= 96 * 4 and lib.mvp_prepare_frames_workspace(0) == 0

"""Frames on the MI355X: ops.prepare_frames (mvp_prepare_frames_u8) bit for bit against PIL's own results (tests/golden/frames.npz) and
the NumPy restatement (tests/frames_oracle.py); the device draws of the jitter; scene.sample_train_batch and prepare_scene on a raw uint8
store."""
import os

import numpy as np
import pytest
import torch

from tests import frames_oracle as FO
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NORMALIZER = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))  # mvpnet/config/mvpnet_3d.py:26
MEAN_STD = np.array(NORMALIZER[0] + NORMALIZER[1], np.float32)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'frames.npz'))


def same_bits(got, exp):
    got = got.contiguous().cpu().numpy()
    return got.dtype == np.float32 and got.shape == exp.shape and np.array_equal(got.view(np.uint32), np.ascontiguousarray(exp).view(np.uint32))


def both(frames, picked, factor=None, order=None, flip=None, normalizer=None, channels_last=False):
    """the op and the oracle on the same arguments, all bytes equal -> the op's result"""
    import mvpnet_amd.ops as ops
    picked = np.asarray(picked, np.int64)
    out = ops.prepare_frames(t(frames), t(picked), factor=None if factor is None else t(np.asarray(factor, np.float32)),
                             order=None if order is None else t(np.asarray(order, np.uint8)), flip=None if flip is None else t(np.asarray(flip, np.uint8)),
                             normalizer=normalizer, channels_last=channels_last)
    H, W = frames.shape[1:3]
    assert tuple(out.shape) == picked.shape + (3, H, W) and out.dtype == torch.float32
    assert out.is_contiguous() != bool(channels_last) or out.numel() == 0
    exp = FO.prepare_frames(frames, picked, factor, order, flip, None if normalizer is None else MEAN_STD)  # (Nf,3,H,W)
    assert same_bits(out, exp.reshape(out.shape))
    if channels_last:  # the memory is (..., H, W, 3)
        assert out.stride()[-3:] == (1, W * 3, 3)
    return out


# ---- PIL's own results ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g', ['s5x7', 's6x8', 's120x160'])  # width 7: one pixel per lane; 8 and 160: four; 120x160: 5 workgroups per frame, the last partial
def test_golden_cases(golden, g):
    """every case of the golden file in one call: the case's image is its picked row (rows repeat), PIL's uint8 result through the
    byte table is the expected value"""
    import mvpnet_amd.ops as ops
    images, idx, factor, order, pil = (golden[g + '_' + k] for k in ('images', 'case_image', 'factor', 'order', 'out'))
    out = ops.prepare_frames(t(images), t(idx), factor=t(factor), order=t(order))
    table = FO.value_table(None)
    exp = np.stack([table[c][pil[..., c]] for c in range(3)], axis=1)  # (K,3,H,W)
    assert same_bits(out, exp)
    out = ops.prepare_frames(t(images), t(idx), factor=t(factor), order=t(order), normalizer=NORMALIZER, channels_last=True)
    table = FO.value_table(MEAN_STD)
    assert same_bits(out, np.stack([table[c][pil[..., c]] for c in range(3)], axis=1))


# ---- the oracle: layouts, normaliser, flip, picks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('normalizer', [None, NORMALIZER])
@pytest.mark.parametrize('g', ['s5x7', 's6x8'])
def test_against_the_oracle(golden, g, normalizer, channels_last):
    frames = golden[g + '_images']
    rs = np.random.RandomState(len(frames) + 2 * channels_last)
    picked = np.array([3, 0, 0, 2, 1, 3, len(frames) + 5, 1, 0], np.int64)  # repeats, out of order, one row past the store (clamped)
    n = len(picked)
    factor = rs.uniform(0.6, 1.4, (n, 3)).astype(np.float32)
    order = np.stack([rs.permutation(3) for _ in range(n)]).astype(np.uint8)
    order[4] = (3, 3, 3)
    order[5] = (2, 7, 0)
    order[7] = (1, 0, 1)  # a second contrast code is no step: one mean per frame
    order[8] = (0, 1, 1)
    for flip in (None, np.zeros(n, np.uint8), np.ones(n, np.uint8), (np.arange(n) % 2).astype(np.uint8)):
        both(frames, picked, factor, order, flip, normalizer, channels_last)
        both(frames, picked, None, None, flip, normalizer, channels_last)
    clamped = both(frames, picked[6:7], factor[6:7], order[6:7], None, normalizer, channels_last)
    assert torch.equal(clamped, both(frames, [len(frames) - 1], factor[6:7], order[6:7], None, normalizer, channels_last))
    assert torch.equal(both(frames, [-3]), both(frames, [0]))


def test_a_store_that_is_not_aligned(golden):
    """frames at an odd byte address (a view into a larger buffer): the entry takes one pixel per lane, the same bits"""
    import mvpnet_amd.ops as ops
    frames = golden['s6x8_images']
    buf = torch.zeros(frames.size + 1, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(frames.shape)
    view.copy_(t(frames))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    picked, factor = t(np.array([4, 1, 1, 0], np.int64)), t(np.array([[1.3, 0.7, 1.2]] * 4, np.float32))
    order, flip = t(np.array([[1, 0, 2], [2, 1, 0], [0, 2, 1], [3, 1, 3]], np.uint8)), t(np.array([1, 0, 1, 0], np.uint8))
    for channels_last in (False, True):
        kw = dict(factor=factor, order=order, flip=flip, normalizer=NORMALIZER, channels_last=channels_last)
        assert torch.equal(ops.prepare_frames(view, picked, **kw), ops.prepare_frames(t(frames), picked, **kw))


@pytest.mark.parametrize('h,w', [(30, 43), (36, 128)])  # 1290 pixels, one per lane; 1152 groups of four: both past a workgroup's 1024
def test_several_workgroups_per_frame(h, w):
    rs = np.random.RandomState(h)
    frames = rs.randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    factor = rs.uniform(0.6, 1.4, (4, 3)).astype(np.float32)
    order = np.array([[1, 0, 2], [2, 1, 0], [0, 2, 1], [3, 1, 3]], np.uint8)
    for channels_last in (False, True):
        both(frames, [2, 0, 1, 1], factor, order, [1, 0, 1, 0], NORMALIZER, channels_last)


def test_normalise_only_one_frame_and_shapes(golden):
    import mvpnet_amd.ops as ops
    frames = golden['s6x8_images']
    one = both(frames, [2], normalizer=NORMALIZER)                                             # Nf = 1, factor=None
    assert tuple(one.shape) == (1, 3, 6, 8)
    assert same_bits(one[0], ((frames[2].astype(np.float32) / 255. - MEAN_STD[:3]) / MEAN_STD[3:]).transpose(2, 0, 1))  # the loader's lines
    both(frames, [1], np.array([[1.3, 0.7, 1.2]], np.float32), np.array([[1, 0, 2]], np.uint8), [1], NORMALIZER)
    grid = both(frames, [[0, 1, 2], [3, 3, 0]], flip=[[0, 1, 0], [1, 0, 1]], channels_last=True)  # picked of any shape
    assert tuple(grid.shape) == (2, 3, 3, 6, 8)
    assert tuple(ops.prepare_frames(t(frames), torch.zeros((0, 3), dtype=torch.int64, device=DEV)).shape) == (0, 3, 3, 6, 8)
    with pytest.raises(RuntimeError):
        ops.prepare_frames(t(frames), t(np.zeros(2, np.int64)), factor=torch.ones((2, 3), device=DEV))  # factor without order
    with pytest.raises(RuntimeError):
        ops.prepare_frames(t(frames).float(), t(np.zeros(2, np.int64)))
    with pytest.raises(RuntimeError):
        ops.prepare_frames(t(frames), t(np.zeros(2, np.int32)))


def test_a_frame_behind_four_gib(golden):
    """a row whose byte offset exceeds 2^32: 80000 frames of 120x160 (4.3 GiB, never written but for the picked rows) against the same
    frames in a store of four"""
    import mvpnet_amd.ops as ops
    rs = np.random.RandomState(3)
    small = np.concatenate([golden['s120x160_images'], rs.randint(0, 256, (3, 120, 160, 3)).astype(np.uint8)])
    rows = [75000, 3, 79999, 74565]
    assert rows[0] * 57600 > 2 ** 32 and rows[3] * 57600 < 2 ** 32 < rows[3] * 57600 + 57600  # one frame straddles 2^32
    big = torch.empty((80000, 120, 160, 3), dtype=torch.uint8, device=DEV)
    small_t = t(small)
    for i, r in enumerate(rows):
        big[r] = small_t[i]
    factor = t(rs.uniform(0.6, 1.4, (4, 3)).astype(np.float32))
    order = t(np.array([[1, 2, 0], [0, 1, 2], [2, 1, 0], [1, 0, 2]], np.uint8))
    flip = t(np.array([1, 0, 0, 1], np.uint8))
    got = ops.prepare_frames(big, torch.tensor(rows, device=DEV), factor=factor, order=order, flip=flip, normalizer=NORMALIZER)
    exp = ops.prepare_frames(small_t, torch.arange(4, device=DEV), factor=factor, order=order, flip=flip, normalizer=NORMALIZER)
    assert torch.equal(got, exp)
    assert same_bits(exp[:1], FO.prepare_frames(small, [0], factor.cpu().numpy(), order.cpu().numpy(), [1], MEAN_STD))
    del big


def test_graph_replay_equals_eager(golden):
    import mvpnet_amd.ops as ops
    frames = t(golden['s6x8_images'])
    rs = np.random.RandomState(9)

    def draw():
        return (rs.randint(0, len(frames), 6).astype(np.int64), rs.uniform(0.6, 1.4, (6, 3)).astype(np.float32),
                np.stack([rs.permutation(3) for _ in range(6)]).astype(np.uint8), rs.randint(0, 2, 6).astype(np.uint8))
    first = draw()
    picked, factor, order, flip = (t(a) for a in first)
    call = lambda: ops.prepare_frames(frames, picked, factor=factor, order=order, flip=flip, normalizer=NORMALIZER)
    eager = call().clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for args in (first, draw(), draw()):
        for dst, a in zip((picked, factor, order, flip), args):
            dst.copy_(t(a))
        out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, call())
        assert same_bits(out, FO.prepare_frames(golden['s6x8_images'], args[0], args[1], args[2], args[3], MEAN_STD))
    assert not torch.equal(out, eager)


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def test_the_law_of_the_draws():
    from mvpnet_amd.augment import draw_color_jitter
    gen = torch.Generator(device=DEV).manual_seed(2024)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        factor, order = draw_color_jitter(6000, (0.4, 0.4, 0.4), DEV, generator=gen)
        f2, o2 = draw_color_jitter(6000, (0.4, 0, 0.4), DEV, generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert factor.device.type == 'cuda' and factor.dtype == torch.float32 and order.dtype == torch.uint8
    codes = (order[:, 0].long() * 9 + order[:, 1].long() * 3 + order[:, 2].long()).cpu().numpy()
    perms = {a * 9 + b * 3 + c: 0 for a, b, c in [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]}
    for c in codes:
        assert c in perms, 'not a permutation'
        perms[c] += 1
    print('order counts', sorted(perms.values()))
    assert all(800 <= v <= 1200 for v in perms.values()), perms  # expected 1000, sd ~ 29
    f = factor.double().cpu().numpy()
    print('factor min / max / mean', f.min(), f.max(), f.mean(0))
    assert f.min() >= np.float32(0.6) and f.max() <= np.float32(1.4) and (np.abs(f.mean(0) - 1) < 0.01).all()
    assert not (o2 == 1).any() and (f2[:, 1] == 1).all() and (o2[:, 2] == 3).all()
    assert 2700 <= int((o2[:, 0] == 0).sum()) <= 3300
    f2 = f2[:, [0, 2]].double().cpu().numpy()
    assert f2.min() >= np.float32(0.6) and f2.max() <= np.float32(1.4) and (np.abs(f2.mean(0) - 1) < 0.01).all()


# ---- a raw store ------------------------------------------------------------------------------------------------------------------------
def _store(raw):
    """2 scenes, 6 frames of 6x8 in all; the overlap rows are random bits (the frame choice is tested elsewhere)"""
    rs = np.random.RandomState(31)
    n = [3000, 2000]
    points = (rs.rand(sum(n), 3) * 3).astype(np.float32)
    label = rs.randint(0, 20, sum(n)).astype(np.int64)
    frames = rs.randint(0, 256, (6, 6, 8, 3)).astype(np.uint8)
    images = frames if raw else FO.prepare_frames(frames, np.arange(6), mean_std=MEAN_STD)
    host = dict(points=points, seg_label=label, scene_offsets=np.array([0, 3000, 5000], np.int64),
                base_point_ind=np.stack([rs.choice(k, 64, replace=False) for k in n]).astype(np.int64),
                overlap_bits=rs.randint(-2 ** 31, 2 ** 31, (6, 2)).astype(np.int32), frame_offsets=np.array([0, 4, 6], np.int64),
                depth=rs.randint(0, 4000, (6, 6, 8)).astype(np.int16), images=images, pose=rs.rand(6, 4, 4).astype(np.float32),
                cam=rs.rand(2, 3, 3).astype(np.float32), kinv=rs.rand(2, 3, 3).astype(np.float32))
    return frames, {k: t(v) for k, v in host.items()}


KW = dict(nb_pts=256, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2), chunk_thresh=0.3)


def _picks(store, soc, gen):
    """the draw and the frame choice of scene.sample_train_batch, by hand: advances `gen` as the call does"""
    import mvpnet_amd.ops as ops
    from mvpnet_amd import chunks as CH
    ch = CH.sample_train_chunks(store['points'], store['seg_label'], store['scene_offsets'], soc, base_point_ind=store['base_point_ind'], generator=gen,
                                **KW)
    begin = store['frame_offsets'][soc]
    return ops.select_frames_batched(store['overlap_bits'], ch['base_bits'], 3, frame_begin=begin, frame_count=store['frame_offsets'][soc + 1] - begin)


def test_sample_train_batch_on_a_raw_store():
    import mvpnet_amd.ops as ops
    from mvpnet_amd import augment as A
    from mvpnet_amd import scene as SC
    frames, store = _store(raw=True)
    soc = t(np.array([0, 1, 1, 0, 0], np.int64))
    gen = lambda: torch.Generator(device=DEV).manual_seed(17)
    aug = dict(color_jitter=(0.4, 0.4, 0.4), image_normalizer=NORMALIZER, flip=0.5)
    SC.sample_train_batch(store, soc, num_rgbd_frames=3, k=3, generator=gen(), **aug, **KW)  # (scratch and the normaliser's 6 floats exist from here on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        batch = SC.sample_train_batch(store, soc, num_rgbd_frames=3, k=3, generator=gen(), **aug, **KW)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert sorted(batch) == sorted(['images', 'points', 'seg_label', 'depth', 'cam_matrix', 'kinv', 'pose', 'k', 'pixel_box', 'flip'])
    g = gen()
    picked = _picks(store, soc, g)
    factor, order = A.draw_color_jitter((5, 3), aug['color_jitter'], DEV, generator=g)
    flip = A.draw_flip((5, 3), 0.5, DEV, generator=g)
    assert torch.equal(batch['pose'], store['pose'][picked]) and torch.equal(batch['depth'], store['depth'][picked])
    assert batch['flip'].dtype == torch.uint8 and tuple(batch['flip'].shape) == (5, 3) and torch.equal(batch['flip'], flip)
    assert 0 < int(flip.sum()) < 15
    assert tuple(batch['images'].shape) == (5, 3, 3, 6, 8)
    assert torch.equal(batch['images'], ops.prepare_frames(store['images'], picked, factor=factor, order=order, flip=flip, normalizer=NORMALIZER))
    assert same_bits(batch['images'], FO.prepare_frames(frames, picked.cpu().numpy(), factor.cpu().numpy(), order.cpu().numpy(), flip.cpu().numpy(),
                                                        MEAN_STD).reshape(5, 3, 3, 6, 8))
    # batch['flip'] marks exactly the mirrored views
    plain = ops.prepare_frames(store['images'], picked, factor=factor, order=order, normalizer=NORMALIZER)
    assert torch.equal(batch['images'], torch.where(flip.bool().view(5, 3, 1, 1, 1), plain.flip(-1), plain))
    # no jitter, no flip, channels-last memory: the normalised frames, no 'flip' key
    quiet = SC.sample_train_batch(store, soc, num_rgbd_frames=3, k=3, generator=gen(), image_normalizer=NORMALIZER, channels_last=True, **KW)
    assert 'flip' not in quiet and quiet['images'].stride()[-3:] == (1, 24, 3)
    assert torch.equal(quiet['images'], ops.prepare_frames(store['images'], picked, normalizer=NORMALIZER))


def test_a_float_store_behaves_as_before():
    from mvpnet_amd import scene as SC
    _, store = _store(raw=False)
    soc = t(np.array([1, 0, 1], np.int64))
    gen = lambda: torch.Generator(device=DEV).manual_seed(4)
    batch = SC.sample_train_batch(store, soc, num_rgbd_frames=3, k=3, generator=gen(), color_jitter=(), image_normalizer=None, flip=0.0,
                                  channels_last=False, **KW)
    assert sorted(batch) == sorted(['images', 'points', 'seg_label', 'depth', 'cam_matrix', 'kinv', 'pose', 'k', 'pixel_box'])
    picked = _picks(store, soc, gen())
    assert batch['images'].is_contiguous() and torch.equal(batch['images'], store['images'][picked])  # the gather of today
    assert torch.equal(batch['pose'], store['pose'][picked])
    again = SC.sample_train_batch(store, soc, num_rgbd_frames=3, k=3, generator=gen(), **KW)
    assert all(torch.equal(batch[k], again[k]) for k in batch if k != 'k')
    for bad in (dict(color_jitter=(0.4, 0.4, 0.4)), dict(flip=0.5), dict(image_normalizer=NORMALIZER), dict(channels_last=True)):
        with pytest.raises(RuntimeError):  # a float store is final
            SC.sample_train_batch(store, soc, num_rgbd_frames=3, k=3, generator=gen(), **bad, **KW)


def test_prepare_scene_takes_raw_frames():
    """prepare_scene / prepare_scene_bucketed on (F,H,W,3) uint8 frames = the same calls on the frames normalised beforehand"""
    from mvpnet_amd.synthetic import make_rgbd_scene
    from mvpnet_amd.scene import prepare_scene, prepare_scene_bucketed
    sc = make_rgbd_scene(3, 8, n_pts=6000, h=30, w=40)
    frames = np.random.RandomState(8).randint(0, 256, (8, 30, 40, 3)).astype(np.uint8)
    floats = t(FO.prepare_frames(frames, np.arange(8), mean_std=MEAN_STD))
    pts, depth, pose = t(sc['points']), t(sc['depth_mm'].astype(np.int16)), t(sc['pose'])
    kw = dict(num_rgbd_frames=3, k=3, min_nb_pts=512, num_base_pts=300, chunk_size=(1.5, 1.5), chunk_stride=1.0, chunk_thresh=100,
              chunk_margin=(0.2, 0.2))
    gen = lambda: torch.Generator(device=DEV).manual_seed(7)
    for fn, extra in ((prepare_scene, {}), (prepare_scene_bucketed, dict(pad_seed=3))):
        want = fn(pts, depth, sc['cam_matrix'], pose, floats, generator=gen(), **extra, **kw)[0]
        got = fn(pts, depth, sc['cam_matrix'], pose, t(frames), generator=gen(), image_normalizer=NORMALIZER, **extra, **kw)[0]
        assert len(got) == len(want) >= 1
        for a, b in zip(got, want):
            assert a['images'].shape == b['images'].shape and torch.equal(a['images'], b['images'])
            assert torch.equal(a['depth'], b['depth'])
    with pytest.raises(RuntimeError):
        prepare_scene(pts, depth, sc['cam_matrix'], pose, floats, generator=gen(), image_normalizer=NORMALIZER, **kw)

"""The definition of mvp_sample_chunks_f32 is the reference's: tests/train_sample_oracle.py reproduces, bit for bit, what
ScanNet2D3DChunks.__getitem__ and ScanNet3DChunks.__getitem__ did on the fixture scene (tests/golden/train_sample.npz, written by
tests/golden/make_train_sample_golden.py from the reference itself); and the counter-hash resampling has the properties the header
states.  No GPU, no kernel."""
import numpy as np
import pytest

from tests import train_sample_oracle as TO


@pytest.fixture(scope='module')
def fixture(golden):
    return golden('train_sample')


@pytest.fixture(scope='module')
def cloud():
    points = TO.fixture_points()
    return points, [TO.fixture_labels(points, kind) for kind in TO.FIXTURE['label_kinds']]


def test_the_fixture_holds_every_case(fixture):
    t, m, nb, f64 = fixture['try_index'], fixture['m'], fixture['nb_pts'], fixture['f64']
    assert (t == 0).any() and (t >= 2).any() and (t == -1).any()
    assert ((nb > 0) & (m < nb)).any() and ((nb > 0) & (m >= nb)).any()
    assert f64.any() and (f64 & (t >= 1)).any()


def test_oracle_reproduces_the_reference_draws(fixture, cloud):
    """try index, the box's bits, the member mask, and the pad prefix: points[choice[:m]] = points[mask]."""
    points, labels = cloud
    P = TO.FIXTURE
    n = len(points)
    for i in range(len(fixture['kind'])):
        label = labels[int(fixture['kind'][i])]
        centers = fixture['centers'][i]
        centers = centers[centers >= 0]
        f64 = bool(fixture['f64'][i])
        # the reference stops drawing at the passing try: the oracle is given the remaining tries too and must not need them
        tried = np.concatenate([centers, np.zeros(P['num_tries'] - len(centers), centers.dtype)])
        t, box, mask = TO.draw_chunk(points, label, tried, P['chunk_size'], P['chunk_margin'], P['chunk_thresh'], bounds_f64=f64)
        assert t == int(fixture['try_index'][i]), i
        assert np.array_equal(np.packbits(mask, bitorder='little'), fixture['mask_bits'][i]), i
        assert int(mask.sum()) == int(fixture['m'][i])
        ref_box = fixture['box'][i]
        if not np.isnan(ref_box).all():
            assert np.array_equal(box, ref_box.astype(np.float32)), i  # (float32 draws: exact; float64 draws: the bounds rounded)
            if not f64:
                assert np.array_equal(ref_box.astype(np.float32).astype(np.float64), ref_box)
        if t >= 0 and f64:  # the float64 bounds themselves
            lo, hi = TO.try_box(points[int(centers[t]), :2], P['chunk_size'], P['chunk_margin'], True)
            assert np.array_equal(np.hstack([lo, hi]), ref_box)
        nb = int(fixture['nb_pts'][i])
        if nb:
            choice = TO.resample(mask, nb, seed=int(fixture['seed'][i]), b=i)
            m = int(mask.sum())
            assert choice.shape == (nb,) and mask[choice].all()
            if m < nb:
                assert np.array_equal(points[choice[:m]], points[mask])
    assert n == P['n_pts']


def test_hash_keys_are_distinct():
    for sb in (0, 0x9E3779B9, TO.chunk_seed(12345, 3)):
        keys = TO.lowbias32(np.arange(500000, dtype=np.uint32) ^ np.uint32(sb))
        assert len(np.unique(keys)) == 500000
    assert TO.lowbias32(np.uint32(1))[0] != 1 and TO.chunk_seed(5, 0) != TO.chunk_seed(5, 1) != TO.chunk_seed(6, 1)


@pytest.mark.parametrize('m,nb_pts', [(1, 64), (63, 64), (64, 64), (65, 64), (5000, 2048), (3000, 8192)])
def test_resampling_is_a_permuted_subset_or_a_prefix_plus_repeats(m, nb_pts):
    rs = np.random.RandomState(m + nb_pts)
    mask = np.zeros(3 * m + 11, bool)
    mask[rs.choice(len(mask), m, replace=False)] = True
    members = np.nonzero(mask)[0]
    c0, c1 = TO.resample(mask, nb_pts, 7, 0), TO.resample(mask, nb_pts, 7, 1)
    assert np.array_equal(c0, TO.resample(mask, nb_pts, 7, 0))
    if m >= nb_pts:
        assert len(np.unique(c0)) == nb_pts and mask[c0].all()  # without replacement
        if m == nb_pts:
            assert np.array_equal(np.sort(c0), members)
        if nb_pts > 8:
            assert not np.array_equal(c0, np.sort(c0)), 'the crop is in key order, not in index order'
            assert not np.array_equal(c0, c1), 'every chunk of a batch has its own keys'
    else:
        assert np.array_equal(c0[:m], members) and mask[c0[m:]].all()
        if m > 1 and nb_pts - m > 8:
            assert len(np.unique(c0[m:])) > 1 and not np.array_equal(c0[m:], c1[m:])
        # the pad formula stays in [0, m) for every 32-bit hash value
        assert ((np.array([0, 1, 2 ** 32 - 1], np.uint64) * np.uint64(m)) >> np.uint64(32)).max() < m


def test_ranged_selection_is_selection_on_the_slice():
    rs = np.random.RandomState(5)
    ov = rs.rand(40, 17) < 0.2
    masks = rs.rand(3, 40) < 0.5
    begin, count = np.array([0, 5, 16]), np.array([5, 11, 1])
    picked, gain = TO.select_frames_ranges(ov, masks, begin, count, 3)
    assert ((picked >= begin[:, None]) & (picked < (begin + count)[:, None])).all() and (picked[2] == 16).all()
    from tests import scene_prep_oracle as SO
    assert np.array_equal(picked[1] - 5, SO.select_frames(ov[masks[1]][:, 5:16], 3))


def test_limits_are_refused_before_any_launch():
    """Over-limit nb_pts / T / Ntot: MVP_EUNSUPPORTED; shape errors: MVP_EINVAL; both before any HIP call (safe without a GPU)."""
    import ctypes
    from mvpnet_amd import _lib
    lib = _lib.lib()
    d = ctypes.c_void_p(16)

    def entry(T, nb_pts, Ntot=1000, B=2, ws=d):
        return lib.mvp_sample_chunks_f32(d, d, d, d, d, None, Ntot, 1, B, T, 0, nb_pts, 1.5, 1.5, 0.2, 0.2, 0.3, 0, 0, None, d, d, d, d, d, d,
                                         None, ws, 1 << 40, None)
    assert entry(10, 8193) == -2 and entry(33, 2048) == -2 and entry(10, 2048, Ntot=2 ** 31) == -2 and entry(10, 2048, B=65536) == -2
    assert entry(0, 2048) == -1 and entry(10, 0) == -1 and entry(10, 2048, Ntot=0) == -1
    assert entry(10, 2048, ws=None) == -3 and entry(10, 2048, ws=ctypes.c_void_p(8)) == -1  # no / misaligned scratch
    assert lib.mvp_sample_chunks_f32(None, d, d, d, d, None, 1000, 1, 2, 10, 0, 2048, 1.5, 1.5, 0.2, 0.2, 0.3, 0, 0, None, d, d, d, d, d, d,
                                     None, d, 1 << 40, None) == -3
    assert lib.mvp_sample_chunks_workspace(1000, 2, 33, 2048) == 0 and lib.mvp_sample_chunks_workspace(1000, 2, 10, 8193) == 0
    small, big = lib.mvp_sample_chunks_workspace(1000, 2, 10, 64), lib.mvp_sample_chunks_workspace(4800000, 32, 10, 8192)
    assert 0 < small < big < 16 << 20
    assert lib.mvp_select_frames_ranges_u32(d, d, d, d, 0, 4, 8, 3, d, None, None) == -1   # no frame at all: frame_count >= 1 cannot hold
    assert lib.mvp_select_frames_ranges_u32(d, d, d, None, 5, 4, 8, 3, d, None, None) == -3
    assert lib.mvp_select_frames_ranges_u32(d, d, d, d, 5, 4, 1025, 3, d, None, None) == -2

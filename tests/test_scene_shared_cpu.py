"""scene.plan_store_groups: the host arithmetic that cuts a scene's batches into runs sharing one feature store (infer_scene_shared)."""
import numpy as np
import pytest

from mvpnet_amd.scene import plan_store_groups


def _check(frames_of_batch, max_frames):
    runs = plan_store_groups(frames_of_batch, max_frames)
    at = 0
    for lo, hi, distinct in runs:
        assert lo == at and hi > lo, 'runs are consecutive and cover every batch once'
        union = set()
        for f in frames_of_batch[lo:hi]:
            union |= {int(x) for x in f}
        assert distinct == sorted(union)
        assert len(distinct) <= max_frames or hi - lo == 1, 'only a single batch may exceed the cap'
        at = hi
    assert at == len(frames_of_batch)
    return runs


def test_hand_made_frame_sets():
    sets = [{0, 1, 2}, {1, 2, 3}, {3, 4}, {7, 8, 9, 10, 11, 12}, {12}, {0, 12}, {5}]
    assert _check(sets, 4) == [(0, 2, [0, 1, 2, 3]), (2, 3, [3, 4]), (3, 4, [7, 8, 9, 10, 11, 12]), (4, 7, [0, 5, 12])]
    assert _check(sets, 5) == [(0, 3, [0, 1, 2, 3, 4]), (3, 4, [7, 8, 9, 10, 11, 12]), (4, 7, [0, 5, 12])]
    assert [r[:2] for r in _check(sets, 1)] == [(i, i + 1) for i in range(len(sets))]
    assert _check(sets, 1000) == [(0, 7, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12])], 'a large cap gives one run'
    assert _check([[4, 4, 2, 2]], 2) == [(0, 1, [2, 4])], 'repeats count once'
    assert plan_store_groups([], 3) == []


def test_a_run_never_grows_past_the_cap_and_greedy_runs_cannot_be_merged():
    rs = np.random.RandomState(5)
    for trial in range(50):
        sets = [rs.choice(40, rs.randint(1, 9), replace=False).tolist() for _ in range(rs.randint(1, 30))]
        cap = int(rs.randint(1, 30))
        runs = _check(sets, cap)
        for a, b in zip(runs, runs[1:]):  # greedy: the next run's first batch did not fit
            assert len(set(a[2]) | {int(x) for x in sets[b[0]]}) > cap
        assert len(_check(sets, 40)) == 1


@pytest.mark.parametrize('cap', [0, -3])
def test_a_cap_below_one_frame_raises(cap):
    with pytest.raises(RuntimeError):
        plan_store_groups([{0}], cap)

"""Host side of the device-resident training meters (metric.DeviceMeters / MeterSnapshot, mvp_seg_loss_meter_f32's state layout), the
validation helpers (scene.val_batches, config.build_val, mvpnet3d.is_better) and the argument errors of the new entry point.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import yaml

from mvpnet_amd import config as C
from mvpnet_amd import metric as M
from tests import meters_oracle as MO
from tests.conftest import GOLDEN


def test_window_arithmetic_over_two_wraps():
    """45 updates with a window of 20: the ring of cumulative pairs and the loss ring wrap twice.  After every update the host arithmetic
    behind DeviceMeters.read() -- MeterSnapshot on the two state arrays, here kept by the NumPy restatement of the kernel's state update --
    gives the numbers and strings of metric.SegAccuracy, metric.SegIoU and a deque loss meter fed the same updates.  Integers equal; the
    two loss averages are float64 sums of the same <= 20 float32 values in possibly different order: rtol 1e-12 (derivable: 20 * 2^-53)."""
    Cn, W = 5, 20
    rs = np.random.RandomState(7)
    si, sf = MO.new_state(Cn, W)
    acc, iou, loss_meter = M.SegAccuracy(), M.SegIoU(Cn), MO.LossMeter(W)
    assert acc.WINDOW == W
    for it in range(45):
        n = int(rs.randint(30, 90))  # the updates weigh differently: a mean of per-update accuracies would not pass
        logit = rs.standard_normal((2, Cn, n)).astype(np.float32)
        logit[0, :, 0] = 1.0  # a tie: the first maximum wins
        label = rs.randint(0, Cn, (2, n)).astype(np.int64)
        label[rs.rand(2, n) < 0.1] = -100
        loss = np.float32(rs.uniform(0.5, 3.0))
        MO.update(si, sf, Cn, W, MO.confusion(logit, label), loss)
        preds, labels = {'seg_logit': torch.from_numpy(logit)}, {'seg_label': torch.from_numpy(label)}
        acc.update_dict(preds, labels)
        iou.update_dict(preds, labels)
        loss_meter.update(float(loss))
        snap = M.MeterSnapshot(si, sf, Cn, W)
        v_acc, v_iou, v_loss = snap.meters()
        assert (v_acc.name, v_iou.name, v_loss.name) == ('seg_acc', 'seg_iou', 'loss')
        assert snap.updates == it + 1 and (snap.correct, snap.valid) == (int(acc.sum), acc.count)
        assert (snap.window_correct, snap.window_valid) == (sum(c for c, _ in acc.recent), sum(v for _, v in acc.recent))
        assert v_acc.avg == acc.avg and v_acc.global_avg == acc.global_avg
        assert str(v_acc) == str(acc) and v_acc.summary_str == acc.summary_str
        np.testing.assert_array_equal(snap.mat, iou.mat.numpy())
        assert v_iou.global_avg == iou.global_avg and str(v_iou) == str(iou) and v_iou.summary_str == iou.summary_str
        assert snap.window_losses == list(loss_meter.values)
        np.testing.assert_allclose(v_loss.avg, loss_meter.avg, rtol=1e-12)
        np.testing.assert_allclose(v_loss.global_avg, loss_meter.global_avg, rtol=1e-12)
        assert str(v_loss) == str(loss_meter) and v_loss.summary_str == loss_meter.summary_str
    assert int(si[0]) == 45 and int(si[3]) == 0


def test_snapshot_of_a_fresh_state_and_of_an_update_without_a_loss():
    si, sf = MO.new_state(4, 3)
    snap = M.MeterSnapshot(si, sf, 4, 3)
    assert snap.updates == 0 and np.isnan(snap.acc_avg) and np.isnan(snap.acc_global_avg) and np.isnan(snap.loss_global_avg)
    assert str(snap.meters()[0]) == str(M.SegAccuracy())
    mat = np.diag([3, 0, 1, 0]).astype(np.int64)
    MO.update(si, sf, 4, 3, mat, np.float32(1.5))
    MO.update(si, sf, 4, 3, mat, None)  # (DeviceMeters.update_dict: the loss view must not average over fewer updates than it claims)
    snap = M.MeterSnapshot(si, sf, 4, 3)
    assert snap.acc_global_avg == 1.0 and np.isnan(snap.loss_avg) and np.isnan(snap.loss_global_avg)
    with pytest.raises(ValueError):
        M.MeterSnapshot(si[:-1], sf, 4, 3)
    with pytest.raises(ValueError):
        M.DeviceMeters(20, window=65)
    with pytest.raises(RuntimeError):
        M.DeviceMeters(4).update_dict({'seg_logit': torch.zeros(1, 4, 8)}, {'seg_label': torch.zeros(1, 8, dtype=torch.int64)})  # host tensors


@pytest.mark.parametrize('S,batch_size,repeats', [(5, 2, 3), (4, 4, 1), (3, 8, 2)])
def test_val_batches_follow_the_repeat_sampler(S, batch_size, repeats):
    from mvpnet_amd import scene as SC
    order = list(range(S)) * repeats
    want = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
    seen = []

    def sample(scene_of_chunk):
        assert scene_of_chunk.dtype == torch.int64 and scene_of_chunk.dim() == 1
        seen.append(scene_of_chunk.tolist())
        return {'index': len(seen) - 1}
    got = list(SC.val_batches(S, batch_size=batch_size, repeats=repeats, sample=sample, device='cpu'))
    assert seen == want and [b['index'] for b in got] == list(range(len(want)))


def test_is_better_truth_table():
    from mvpnet_amd.mvpnet3d import is_better
    table = [('seg_iou', 0.5, None, True), ('seg_iou', None, 0.4, False), ('seg_iou', None, None, False),
             ('seg_iou', 0.5, 0.4, True), ('seg_iou', 0.4, 0.5, False), ('seg_iou', 0.5, 0.5, False),
             ('seg_acc', 0.9, 0.8, True), ('loss', 0.5, 0.4, False), ('loss', 0.4, 0.5, True), ('loss', 0.5, 0.5, False),
             ('seg_loss', 1.0, 2.0, True), ('loss', 3.0, None, True), ('loss', None, 3.0, False)]
    for name, cur, best, want in table:
        assert is_better(name, cur, best) is want, (name, cur, best)


def test_build_val_on_the_three_committed_yamls():
    with open(os.path.join(GOLDEN, 'configs.json')) as f:
        y3d = json.load(f)
    with open(os.path.join(GOLDEN, 'configs_2d.json')) as f:
        y2d = json.load(f)
    text = lambda tree: yaml.safe_dump(tree)
    assert C.build_val(C.load_cfg(text=text(y3d['mvpnet_3d_unet_resnet34_pn2ssg']))) == \
        {'batch_size': 32, 'repeats': 5, 'period': 1000, 'metric': 'seg_iou'}
    assert C.build_val(C.load_cfg(text=text(y3d['pn2ssg_chunk']))) == {'batch_size': 32, 'repeats': 3, 'period': 1000, 'metric': 'seg_iou'}
    assert C.build_val(C.load_cfg(text=text(y2d['unet_resnet34']))) == {'batch_size': 32, 'repeats': 1, 'period': 2000, 'metric': 'seg_iou'}
    assert C.build_val(C.load_cfg(text='TASK: sem_seg_3d')) == {'batch_size': 1, 'repeats': 1, 'period': 0, 'metric': 'seg_iou'}


def test_seg_loss_meter_argument_errors_do_not_launch():
    """mvp_seg_loss_meter_f32: precondition failures return MVP_E* before any HIP call (safe without a GPU); a null pointer comes ahead of
    any other error."""
    from mvpnet_amd import _lib
    f = _lib.lib().mvp_seg_loss_meter_f32
    d = ctypes.c_void_p(16)
    ok = dict(logit=d, label=d, weight=None, acc=d, loss=d, si=d, sf=d, B=1, C=20, N=8, window=20)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['logit'], a['B'], a['C'], a['N'], a['C'] * a['N'], a['N'], 1, a['label'], a['weight'], -100, a['acc'], a['loss'], a['si'], a['sf'],
                 a['window'], None)
    for name in ('logit', 'label', 'si', 'sf'):
        assert call(**{name: None}) == -3, name                  # MVP_ENULL
        assert call(**{name: None}, window=0, C=0) == -3, name     # ... ahead of any other error
    assert call(acc=None) == -3 and call(loss=None) == -3          # exactly one of acc / loss
    assert call(acc=None, window=0) == -3
    assert call(window=0) == -1 and call(window=65) == -1 and call(window=-1) == -1   # MVP_EINVAL
    assert call(acc=None, loss=None, window=0) == -1 and call(acc=None, loss=None, window=65) == -1   # the meters-only form as well
    assert call(C=0) == -1 and call(C=1 << 16) == -1 and call(B=-1) == -1 and call(B=1 << 20, N=1 << 20) == -1   # check_seg's size limits

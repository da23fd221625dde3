"""bench.py as the driver runs it, on the MI355X: a plain run prints the headline line only (the side measurements need --full), and
--dump-outputs writes what the last of the --steps timed steps returned -- the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(dump):
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4', '--dump-outputs', str(dump)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), np.load(os.path.join(dump, 'loss.npy')), np.load(os.path.join(dump, 'seg_logit.npy'))


def test_plain_run_dumps_the_last_step(tmp_path):
    line, loss, logit = _plain_run(tmp_path / 'a')
    assert line['steps'] == 3 and line['warmup'] == 1 and line['unit'] == 'chunks/s' and line['dtype'] == 'f32' and line['higher_is_better'] is True
    assert line['ms_per_step'] > 0 and abs(line['value'] - 4 * 1e3 / line['ms_per_step']) <= 2e-3 * line['value']
    assert not {'cpu_baseline', 'roofline', 'ms_per_step_repeats', 'dense', 'fwd_only'} & set(line)   # --full only
    assert loss.dtype == np.float32 and loss.shape == () and np.isfinite(loss)
    assert logit.dtype == np.float32 and logit.shape == (4, 20, 8192) and np.isfinite(logit).all()
    # a second run with the same arguments: the same inputs, the same weights, the same dropout seeds -> the same outputs up to rounding.
    # What is left is the arrival order of the fused training levels' fp64 BatchNorm-statistics atomics, measured at the
    # bench shape (B = 32): loss 1 ulp, logits 3.9e-6 of their largest entry (4.9e-6 relative L2).  Training at the YAML's rate instead
    # compounded it to 7e-2 of the largest logit over the run's ~150 steps.
    _, loss2, logit2 = _plain_run(tmp_path / 'b')
    assert abs(float(loss2) - float(loss)) <= 1e-5 * abs(float(loss))
    assert np.abs(logit2.astype(np.float64) - logit).max() <= 1e-4 * np.abs(logit).max()

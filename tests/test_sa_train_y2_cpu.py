"""The kernel instances that the B = 32 training step launches for a stored y_2 (csrc/sa_train.hip, rows.SA_Y2_PASSES, profiles/sa_y2.txt):
they are in the built library and none keeps vector registers in scratch memory -- what tests/test_isa_cpu.py checks for the step's
other kernels (tests/golden/step_kernels_b32.txt, whose re-computing sa_train instances MVP_SA_Y2=0 still launches)."""
import os

import pytest

from mvpnet_amd import _lib
from tests.test_isa_cpu import OBJDUMP, READELF, kernel_metadata

# forward bf16x6 (3 pieces), backward bf16x3 (2 pieces); level 1 = block shape (1, 1, 2), level 2 = (2, 2, 4)
STEP_Y2_KERNELS = [
    'sa_train_fwd_y2_kernel<1, 1, 1, 3, 2, 1>',   # stage 2 stores
    'sa_train_fwd_y2_kernel<2, 2, 1, 3, 2, 1>',
    'sa_train_fwd_y2_kernel<1, 1, 2, 3, 3, 2>',   # stage 3 loads
    'sa_train_fwd_y2_kernel<2, 2, 4, 3, 3, 2>',
    'sa_train_bwd_y2_kernel<1, 1, 2, 2, 3>',      # layer-3 backward loads
    'sa_train_bwd_y2_kernel<2, 2, 4, 2, 3>',
]


def test_the_pass_table_names_the_instances_listed_here():
    from mvpnet_amd import rows
    assert rows.SA_Y2_PASSES == {(1, 1, 2): ('fwd3', 'bwd3'), (2, 2, 4): ('fwd3', 'bwd3')}
    assert rows.sa_y2_passes(32, 32, 64) == ('fwd3', 'bwd3') and rows.sa_y2_passes(64, 64, 128) == ('fwd3', 'bwd3')
    assert rows.sa_y2_passes(64, 64, 64) == ()


@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason='llvm-objdump / llvm-readelf of the ROCm toolchain are not installed')
def test_the_step_s_y2_kernels_do_not_spill(tmp_path):
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libmvp_hip.so is not built')
    meta = kernel_metadata(tmp_path)
    missing = [k for k in STEP_Y2_KERNELS if k not in meta]
    assert not missing, 'kernels of the step that the library does not hold: %s' % missing
    spilled = {k: meta[k] for k in STEP_Y2_KERNELS if meta[k][1] > 0}
    assert not spilled, 'y_2 kernels of the training step with vector registers in scratch memory (vgprs, vgpr spill, sgpr spill, lds): %s' % spilled

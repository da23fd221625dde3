"""The workgroups per CU that csrc/mlp_bwd_wide.hip declares for its 64-channel instances are what the built instances can hold.

A workgroup of the kernel is 8 waves, 2 on each SIMD of its CU; a second workgroup beside it needs 4 waves per SIMD, which the register file
(512 per lane and SIMD, VGPR + AGPR in one budget) grants only at 128 registers or fewer, and twice the LDS.  The launch bounds and the
launcher's grid come from ONE table in the source, kWideResidency {NS, MODE, CH, workgroups per CU}; this test reads the same table and the
code objects inside the built library (their AMDGPU metadata: what the loader reads).  An instance declared at two must have at most 128
registers and no scratch; every listed instance and every shipped 128-channel instance must be free of scratch.  (The mismatch this guards
against was invisible: the launcher asked for two per CU while every mode-1 / mode-3 instance of the 64-channel shape held 142 - 161
registers.  Today every instance is declared -- and launched -- at one: two resident workgroups were measured and bought nothing.)"""
import glob
import os
import re
import shutil
import subprocess

import pytest

from mvpnet_amd import _lib
from tests.test_isa_cpu import CXXFILT, OBJDUMP, READELF

SRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc', 'mlp_bwd_wide.hip')
LDS_PER_CU = 160 * 1024

pytestmark = pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)),
                                reason='llvm-objdump / llvm-readelf of the ROCm toolchain are not installed')


def declared_residency():
    """{(NS, MODE, CH): workgroups per CU} of kWideResidency, from the source text (an instance that is not listed runs one per CU)."""
    text = open(SRC).read()
    m = re.search(r'constexpr WideResidency kWideResidency\[\] = \{(.*?)\n\};', text, re.S)
    assert m, 'kWideResidency not found in %s' % SRC
    rows = [tuple(int(v) for v in t) for t in re.findall(r'\{\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(\d+)\s*\}', m.group(1))]
    assert rows and len({r[:3] for r in rows}) == len(rows), rows
    return {r[:3]: r[3] for r in rows}


def wide_lds_bytes(ns, ch):
    """The dynamic LDS the launcher asks for (mvp_mlp_layer_backward_wide_pooled_p_f32: `ldsz`)."""
    row = ch * 2 + 16
    return max(ns * (ch * row + 2 * 64 * row) + 64 + 11 * ch * 4, 2 * (512 // (ch // 4)) * ch * 8)


@pytest.fixture(scope='module')
def wide_instances(tmp_path_factory):
    """{(NS, MODE, CH, DWO): dict(vgpr, agpr, scratch, vgpr_spill)} of every mlp_bwd_wide_kernel instance in libmvp_hip.so."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libmvp_hip.so is not built')
    tmp = str(tmp_path_factory.mktemp('wide_regs'))
    lib = os.path.join(tmp, 'libmvp_hip.so')
    shutil.copy(_lib.LIB_PATH, lib)
    subprocess.run([OBJDUMP, '--offloading', lib], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
    recs = []
    for o in sorted(glob.glob(lib + '.*gfx950')):
        notes = subprocess.run([READELF, '--notes', o], check=True, capture_output=True, text=True).stdout
        parts = re.split(r'\n\s+- \.agpr_count:\s+(\d+)', notes)
        for agpr, blk in zip(parts[1::2], parts[2::2]):
            f = lambda k: re.search(r'\.' + k + r':\s+(\S+)', blk)
            if f('name') and 'mlp_bwd_wide_kernel' in f('name').group(1) and not f('name').group(1).endswith('.kd'):
                recs.append((f('name').group(1), dict(agpr=int(agpr), vgpr=int(f('vgpr_count').group(1)), scratch=int(f('private_segment_fixed_size').group(1)),
                                                      vgpr_spill=int(f('vgpr_spill_count').group(1)))))
    dem = subprocess.run([CXXFILT], input='\n'.join(r[0] for r in recs), check=True, capture_output=True, text=True).stdout.split('\n')
    out = {}
    for (_, rec), d in zip(recs, dem):
        m = re.search(r'mlp_bwd_wide_kernel<(\d+), (-?\d+), (\d+), (true|false)>', d)
        assert m, d
        out[(int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == 'true')] = rec
    assert len(out) >= 20, 'mlp_bwd_wide_kernel instances found in the library: %d' % len(out)
    return out


def test_the_table_names_what_the_step_runs():
    """The 64-channel instances of the default (bf16x3) backward are declared: the aggregation MLP's inner layers run them."""
    table = declared_residency()
    assert (2, 1, 64) in table and (2, 3, 64) in table
    for (ns, mode, ch), per_cu in table.items():
        assert per_cu in (1, 2), ((ns, mode, ch), per_cu)
        assert per_cu * wide_lds_bytes(ns, ch) <= LDS_PER_CU, '%d workgroups of <%d, %d, %d> need more LDS than a CU has' % (per_cu, ns, mode, ch)


def test_declared_instances_fit_their_registers_without_scratch(wide_instances):
    for (ns, mode, ch), per_cu in declared_residency().items():
        rec = wide_instances.get((ns, mode, ch, False))
        assert rec is not None, 'the library holds no mlp_bwd_wide_kernel<%d, %d, %d, false>' % (ns, mode, ch)
        # 8 waves per workgroup on 4 SIMDs: 2 per SIMD and workgroup; 512 registers per lane and SIMD, allocated in steps of 8
        # (.vgpr_count of a gfx950 code object is the unified count; adding .agpr_count again can only make the test stricter)
        regs = max(rec['vgpr'], rec['vgpr'] + rec['agpr'] if rec['agpr'] else 0)
        assert regs <= 512 // (2 * per_cu), ((ns, mode, ch), per_cu, rec)
        assert rec['scratch'] == 0 and rec['vgpr_spill'] == 0, ((ns, mode, ch), rec)


def test_the_128_channel_instances_keep_out_of_scratch(wide_instances):
    """The shipped CH = 128 instances (the fast modes and the weight-gradient-only ones): no scratch.  (MODE -1, everything decided at run time, is
    exempt: it spilled 15 - 18 registers before the 64-channel instances were given their own budget and is not in the training step.)"""
    checked = 0
    for (ns, mode, ch, dwo), rec in sorted(wide_instances.items()):
        if ch == 128 and mode >= 0:
            assert rec['scratch'] == 0 and rec['vgpr_spill'] == 0, ((ns, mode, ch, dwo), rec)
            checked += 1
    assert checked >= 12, checked

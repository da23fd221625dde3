"""Residency report of the library's kernels: what the compiler gave each instance, and how many waves and workgroups that lets a CU hold.

CPU only.  Rebuilds mvpnet_amd/csrc/*.hip (device side, gfx950, the Makefile's own flags) into a scratch directory with
-Rpass-analysis=kernel-resource-usage and prints, per kernel instance: VGPR and AGPR counts, scratch bytes per lane, static LDS, the
workgroup size the code object declares (launch bounds; 1024 = none declared), the waves per SIMD the registers allow, and the workgroups per
CU allowed by registers and by LDS.  Dynamic LDS is not in the code object: for the kernels listed in DYNAMIC_LDS it is computed as their
launcher computes it, for any other pass --lds BYTES.

    python tools/residency.py                      every kernel of every file
    python tools/residency.py --step               the kernels of the B = 32 training step (tests/golden/step_kernels_b32.txt)
    python tools/residency.py mlp_bwd_wide.hip     one file;  --filter TEXT: instances whose name contains TEXT

Register file (gfx950): 512 registers per lane and SIMD, VGPR + AGPR in one budget, allocated in steps of 8; a CU has 4 SIMDs, 160 KB of LDS
and room for 32 waves."""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mvpnet_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
READELF = '/opt/rocm/lib/llvm/bin/llvm-readelf'
CXXFILT = shutil.which('c++filt') or '/opt/rocm/lib/llvm/bin/llvm-cxxfilt'
LDS_PER_CU, WAVES_PER_CU, REGS_PER_SIMD = 160 * 1024, 32, 512


def makefile_flags():
    """(common flags, names of the files built with -fno-slp-vectorize) as the Makefile has them."""
    text = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS = (.*)$', text, re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    no_slp = re.search(r'^NO_SLP = (.*)$', text, re.M).group(1).split()
    return flags, set(no_slp)


def wide_lds(name):
    """Dynamic LDS of an mlp_bwd_wide_kernel<NS, MODE, CH, DWO> instance, as mvp_mlp_layer_backward_wide_pooled_p_f32 / mlp_dw_wide_launch size it."""
    m = re.match(r'mlp_bwd_wide_kernel<(\d+), (-?\d+), (\d+), (true|false)>', name)
    if not m:
        return None
    ns, ch, dwo = int(m.group(1)), int(m.group(3)), m.group(4) == 'true'
    row = ch * 2 + 16
    if dwo:
        return ns * 2 * 64 * row + 64 + 11 * ch * 4
    return max(ns * (ch * row + 2 * 64 * row) + 64 + 11 * ch * 4, 2 * (512 // (ch // 4)) * ch * 8)


DYNAMIC_LDS = [wide_lds]


def demangle(names):
    out = subprocess.run([CXXFILT], input='\n'.join(names), check=True, capture_output=True, text=True).stdout.split('\n')
    res = []
    for d in out[:len(names)]:
        d = d.replace('void ', '').replace('(anonymous namespace)::', '')
        depth, name = 0, ''
        for c in d:
            depth += c == '<'
            depth -= c == '>'
            if c == '(' and depth == 0:
                break
            name += c
        res.append(name)
    return res


def compile_one(src, tmp, flags, no_slp):
    stem = os.path.splitext(os.path.basename(src))[0]
    co = os.path.join(tmp, stem + '.co')
    cmd = [HIPCC] + flags + (['-fno-slp-vectorize'] if stem in no_slp else []) + [
        '--cuda-device-only', '--no-gpu-bundle-output', '-c', src, '-o', co, '-Rpass-analysis=kernel-resource-usage']
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    if r.returncode != 0:
        raise RuntimeError('%s failed:\n%s' % (' '.join(cmd), r.stderr[-2000:]))
    recs = {}
    for b in re.split(r'Function Name: ', r.stderr)[1:]:
        def g(k):
            m = re.search(k + r': (\d+)', b)
            return int(m.group(1)) if m else 0
        recs[b.split('\n')[0].split()[0]] = dict(vgpr=g('VGPRs'), agpr=g('AGPRs'), scratch=g(r'ScratchSize \[bytes/lane\]'), spill=g('VGPRs Spill'),
                                                 lds=g(r'LDS Size \[bytes/block\]'))
    wg = {}
    if os.path.exists(READELF):
        notes = subprocess.run([READELF, '--notes', co], capture_output=True, text=True).stdout
        for blk in re.split(r'\n\s+- \.agpr_count', notes)[1:]:
            n, w = re.search(r'\.name:\s+(\S+)', blk), re.search(r'\.max_flat_workgroup_size:\s+(\d+)', blk)
            if n and w:
                wg[n.group(1)] = int(w.group(1))
    return stem, recs, wg


def residency(r, block, lds):
    alloc = max(8, (r['vgpr'] + r['agpr'] + 7) // 8 * 8)
    waves_simd = min(8, REGS_PER_SIMD // alloc)
    waves_wg = (block + 63) // 64
    by_regs = min(waves_simd * 4, WAVES_PER_CU) // waves_wg
    by_lds = LDS_PER_CU // lds if lds else None
    return waves_simd, by_regs, by_lds


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('files', nargs='*', help='.hip files of mvpnet_amd/csrc (default: all of the Makefile)')
    ap.add_argument('--filter', default='', help='only instances whose demangled name contains this')
    ap.add_argument('--step', action='store_true', help='only the kernels of tests/golden/step_kernels_b32.txt')
    ap.add_argument('--lds', type=int, default=0, help='dynamic LDS bytes to add for kernels not in DYNAMIC_LDS')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    flags, no_slp = makefile_flags()
    files = a.files
    if not files:
        files = re.search(r'^SRCS = (.*)$', open(os.path.join(CSRC, 'Makefile')).read(), re.M).group(1).split()
    files = [os.path.join(CSRC, os.path.basename(f)) for f in files]
    step = None
    if a.step:
        with open(os.path.join(ROOT, 'tests', 'golden', 'step_kernels_b32.txt')) as f:
            step = {l.strip() for l in f if l.strip() and not l.startswith('#')}
    tmp = tempfile.mkdtemp(prefix='residency_')
    try:
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
            results = list(ex.map(lambda s: compile_one(s, tmp, flags, no_slp), files))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print('# %-58s %5s %5s %8s %7s %6s | %10s %9s %8s' % ('kernel instance (file)', 'VGPR', 'AGPR', 'scratch', 'LDS', 'block', 'waves/SIMD', 'WG/CU reg', 'WG/CU LDS'))
    for stem, recs, wg in results:
        names = list(recs)
        for mangled, name in zip(names, demangle(names) if names else []):
            if a.filter not in name or (step is not None and name not in step):
                continue
            r = recs[mangled]
            dyn = next((v for v in (f(name) for f in DYNAMIC_LDS) if v is not None), None)
            lds = r['lds'] + (dyn if dyn is not None else a.lds)
            block = wg.get(mangled, 1024)
            waves_simd, by_regs, by_lds = residency(r, block, lds)
            print('%-60s %5d %5d %8d %7d %6d | %10d %9d %8s' % (('%s (%s)' % (name, stem))[:60], r['vgpr'], r['agpr'], r['scratch'], lds, block, waves_simd, by_regs,
                                                              '-' if by_lds is None else by_lds))
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""The 64-channel one-pass backward (csrc/mlp_bwd_wide.hip, CH = 64): its grid, its ticket and the runs of tiles a draw hands out.

What workgroups that share one ticket can get wrong: a tile taken twice or not at all, a workgroup without a first tile, a partial tile
or a partial run handed out by ticket, results that depend on which workgroup took a tile.  Shapes, C = Cp = 64:
  R = 64 * (2 CUs) + 37 (rounded up to whole groups of K = 3): every workgroup of a grid of up to two per CU has a static first tile and
      the partial tile goes by ticket (32 805 rows on 256 CUs);
  R = 64 * (32 CUs + 2) + 37 ("runs"): enough tiles per workgroup that a draw hands out a RUN of 2 tiles; the last run holds one tile,
      and that tile is partial;
  R = 65: one full tile and a one-row tile;  R = 1.
Modes 1 (dz_i given) and 3 (behind a sum over K neighbours: mvp_mlp_layer_backward_wide_pooled_p_f32, one gradient row per K rows), bf16x3 and
bf16x6 backward.  The pooled form needs whole groups (R % K == 0, K > 1 to be mode 3 at all), so it runs 65 rows as 13 groups of K = 5 and,
in place of R = 1, its smallest shape: one group of K = 3 rows.

Checked: dZ, the two column sums and dW against float64 with the tolerances of test_ops_gpu.test_mlp_layer_backward_wide for the same
precision; dZ -- a per-row result, so independent of who took the tile -- bit for bit between the ticket path, a second run of it, the
static round-robin (no ticket) and the reproducible mode's workspace path; and the ticket word.  The ticket is caller memory that the
kernel only counts up (include/mvp_hip.h: "one zeroed int32 of caller memory"; the existing tests assert it is > 0 after a launch), so it
is NOT zero after the launch: what is asserted is the exact count of draws for the grid that the source's residency table (kWideResidency)
gives the instance -- single tiles: one draw per launched workgroup plus one per tile; runs of n tiles: one per run whose last-but-one
tile exists, (tiles + 1) // n.  That every tile was taken exactly once is checked on the results: dZ starts as NaN, and the kernel's
column sum of dZ must equal the sum over the dZ it wrote far more closely than one tile's worth."""
import numpy as np
import pytest
import torch

from tests.test_bwd_wide_regs_cpu import declared_residency

pytestmark = pytest.mark.gpu

C = 64
LOOSE = {'bf16x6': 4.0, 'bf16x3': 16.0}   # as test_mlp_layer_backward_wide


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def cases():
    out = []
    for precision in ('bf16x3', 'bf16x6'):
        for rows in ('big', 'runs', 65, 1):
            out.append((1, rows, 1, precision))
        for rows, k in (('big', 3), ('runs', 3), (65, 5), (3, 3)):
            out.append((3, rows, k, precision))
    return out


@pytest.mark.parametrize('mode,rows,K,precision', cases())
def test_grid_ticket_and_runs(dev, mode, rows, K, precision):
    from mvpnet_amd import _lib as L
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    R = rows if isinstance(rows, int) else -(-(64 * (2 * cus if rows == 'big' else 32 * cus + 2) + 37) // K) * K
    G = R // K
    ntiles = (R + 63) // 64
    if rows == 'big':
        assert 2 * cus < ntiles and R % 64 != 0   # every workgroup of the widest grid has a first tile; the last tile is partial
    prec = (L.MLP_PRECISIONS['bf16x6'], L.MLP_PRECISIONS[precision])
    loose = LOOSE[precision]
    hi = torch.float64
    torch.manual_seed(R + 7 * mode)
    w = torch.randn(C, C, device=dev) * 0.2
    x = torch.randn(R, C, device=dev)
    g = torch.randn(G, C, device=dev)
    yi = torch.randn(R, C, device=dev) * 1.5 + 0.2
    mean_i, invstd_i, gamma_i = torch.randn(C, device=dev) * 0.3, torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) + 0.5
    beta_i = torch.randn(C, device=dev) * 0.2
    stat_i = torch.randn(2 * C, device=dev, dtype=hi) * R * 0.01
    pm, pi = torch.randn(C, device=dev) * 0.3, torch.rand(C, device=dev) + 0.5
    pg, pb = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2

    # float64 reference; the two ReLU masks are decisions, taken in float32 with the kernel's operation order (see test_mlp_layer_backward_wide)
    f32 = lambda t: t.detach().cpu().numpy().astype(np.float32)
    mask_prev = torch.from_numpy((((f32(x) - f32(pm)) * f32(pi)) * f32(pg) + f32(pb)) > 0).to(dev)
    xh_i = (yi.to(hi) - mean_i.to(hi)) * invstd_i.to(hi)
    dzi = g.to(hi)
    if mode == 3:
        mask_i = torch.from_numpy((((f32(yi) - f32(mean_i)) * f32(invstd_i)) * f32(gamma_i) + f32(beta_i)) > 0).to(dev)
        dzi = torch.where(mask_i, dzi.repeat_interleave(K, 0), torch.zeros(R, C, dtype=hi, device=dev))
    dy = (gamma_i.to(hi) * invstd_i.to(hi)) * ((dzi - stat_i[:C] / R) - xh_i * (stat_i[C:] / R))
    xh = (x.to(hi) - pm.to(hi)) * pi.to(hi)
    a = torch.relu(xh * pg.to(hi) + pb.to(hi))
    ref_dw = (dy.t() @ a).cpu().numpy()
    ref_dz_t = torch.where(mask_prev, dy @ w.to(hi), torch.zeros(R, C, dtype=hi, device=dev))
    ref_dz = ref_dz_t.cpu().numpy()
    ref_s, ref_t = ref_dz_t.sum(0).cpu().numpy(), (ref_dz_t * xh).sum(0).cpu().numpy()
    sw, sz, big = max(1.0, float(np.abs(ref_dw).max())), max(1.0, float(np.abs(ref_dz).max())), max(1.0, R / 5000.0)

    wsbuf = torch.empty(L.lib().mvp_mlp_weight_grad_workspace_floats(), device=dev)

    def run(path):
        dw = torch.zeros(C, C + 4, device=dev)
        dz = torch.full((R, C), float('nan'), device=dev)
        stat = torch.zeros(2 * C, dtype=hi, device=dev)
        tk = torch.zeros(1, dtype=torch.int32, device=dev)
        dgb = torch.full((2, C), float('nan'), device=dev)
        ws = wsbuf if path == 'workspace' else None
        L.call('mvp_mlp_layer_backward_wide_pooled_f32', g, L.ptr(g), L.ptr(yi), L.ptr(mean_i), L.ptr(invstd_i), L.ptr(gamma_i),
               L.ptr(beta_i) if mode == 3 else None, L.ptr(stat_i), L.ptr(dgb[0]), L.ptr(dgb[1]), 1, 2 if mode == 3 else 1, K, 0.0, 0,
               L.ptr(x), C, L.ptr(pm), L.ptr(pi), L.ptr(pg), L.ptr(pb), L.ptr(w), C, R, C, C, L.ptr(dw), C + 4, L.ptr(dz), L.ptr(stat),
               None if path == 'static' else L.ptr(tk), L.ptr(ws), 0 if ws is None else ws.numel(), prec=prec)
        tag = 'mode={} R={} K={} {} {}'.format(mode, R, K, precision, path)
        dwn, dzn, stn = dw.cpu().numpy(), dz.cpu().numpy(), stat.cpu().numpy()
        np.testing.assert_allclose(dwn[:, :C], ref_dw, rtol=1e-4 * loose, atol=3e-5 * sw * loose, err_msg=tag)
        assert float(np.abs(dwn[:, C:]).max()) == 0.0, tag
        np.testing.assert_allclose(dzn, ref_dz, rtol=1e-5 * loose, atol=2e-5 * sz * loose, err_msg=tag)
        np.testing.assert_allclose(stn[:C], ref_s, rtol=1e-5 * loose, atol=2e-3 * loose * big * sz, err_msg=tag)
        np.testing.assert_allclose(stn[C:], ref_t, rtol=1e-5 * loose, atol=2e-3 * loose * big * sz, err_msg=tag)
        np.testing.assert_array_equal(dgb[0].cpu().numpy(), stat_i[C:].float().cpu().numpy())
        np.testing.assert_array_equal(dgb[1].cpu().numpy(), stat_i[:C].float().cpu().numpy())
        # every tile once: the kernel's fp64 column sums (of per-thread fp32 partial sums) against the sum of the dZ it wrote -- fp32 rounding of
        # at most a few hundred additions per thread, 1e-5 of the column's sum of magnitudes; a tile taken twice or skipped is 64 rows' worth
        dzs, dza = dz.to(hi).sum(0).cpu().numpy(), dz.to(hi).abs().sum(0).cpu().numpy()
        np.testing.assert_allclose(stn[:C], dzs, rtol=0, atol=1e-5 * float(dza.max()) + 1e-12, err_msg=tag)
        return dzn, int(tk)

    dz_ticket, tk = run('ticket')
    dz_again, tk_again = run('ticket')
    dz_static, _ = run('static')
    dz_ws, tk_ws = run('workspace')
    assert np.array_equal(dz_ticket, dz_again), 'dZ differs between two runs of the ticket path'
    assert np.array_equal(dz_ticket, dz_static), 'dZ of the ticket path differs from the static tile order'
    assert np.array_equal(dz_ticket, dz_ws), 'dZ of the ticket path differs from the workspace path'
    # the ticket: every launched workgroup draws once for its second tile and once more per tile it works on -- grid + ntiles draws in all
    ns = {'bf16x3': 2, 'bf16x6': 3}[precision]
    grid = min(ntiles, declared_residency().get((ns, mode, C), 1) * cus)
    run = max(1, min(4, ntiles // grid // 16))   # the launcher's rule (mvp_mlp_layer_backward_wide_pooled_p_f32: a.run)
    assert run == (2 if rows == 'runs' else 1), (run, ntiles, grid)
    draws = grid + ntiles if run == 1 else (ntiles + 1) // run
    assert tk == draws and tk_again == tk, (tk, tk_again, draws, grid, ntiles, run)
    assert tk_ws == (0 if grid > 1 else tk), tk_ws   # the workspace path keeps a static tile order and leaves the ticket alone

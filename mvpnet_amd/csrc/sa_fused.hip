// sa_fused.hip -- a whole set-abstraction level in ONE kernel for inference (BatchNorm with running statistics) on gfx950:
//   gather the ball's K = 32 neighbours -> first layer (its linear feature part was applied per point: zf) -> BatchNorm + ReLU ->
//   layer 2 -> BatchNorm + ReLU -> layer 3 -> BatchNorm + ReLU -> max over the 32 neighbours -> (B, M, C3).
// Replaces QueryGrouper + SharedMLP(ndim=2) + torch.max of the reference (mvpnet/models/pn2/modules.py:20-37,100-108;
// common/nn/modules/conv.py:41-51), whose (B,C,M,32) tensors make a round trip through HBM after every conv, BatchNorm and ReLU, and
// the unfused rows path of this repository (group_lin_rows + 2 x mlp_fwd + bn_act), which still writes and re-reads the three
// pre-BN tensors.  Here NOTHING between the gathered rows and the pooled output touches HBM:
//   * one wave = one ball: lane (row = lane & 31 = neighbour, half h = lane >> 5) holds the k = 8 t + 4 h + e channels of ITS neighbour
//     -- exactly the A-operand fragment order of v_mfma_f32_32x32x16_bf16, so the gathered / activated row feeds the MFMAs directly;
//   * an MFMA result tile is lane = output channel, registers = the 32 neighbours: BatchNorm + ReLU of a layer are per-lane
//     constants there, and the max over the neighbours is a max over the lane's 16 registers + one exchange with lane ^ 32;
//   * between layers the activated tile goes through a wave-private 32 x 32 LDS tile (written as columns, read back as rows) to
//     become the next layer's A fragments -- the "LDS-staged per-ball neighbourhood";
//   * both weight matrices sit in LDS for the whole kernel, pre-split in bf16 pieces, in fragment order (as mlp_stream.hip).
// Contraction: split-bf16 (mlp_common.h).  Arithmetic per element equals the unfused path (same operation order in the first
// layer, same BatchNorm expression), so the two agree to fp32 rounding of the accumulation order.
// The ball pipeline and gather, the first-layer tables, the BatchNorm constants and the tile between two layers, and the host side of the launch
// are those of the training kernels: sa_common.h.  This file's own are the kernel's frame, its one-pass first layer and its epilogue.
#include "sa_common.h"

namespace {

struct SaArgs {
  SaSrc s;               // (s.zf may be nullptr)
  const float* W2;       // (C2, C1)
  const float* bn2[4];   // mean, invstd, gamma, beta
  const float* W3;       // (C3, C2)
  const float* bn3[4];
  int C2, C3;
  float* out;            // (B*M, C3)
  uint8_t* arg;          // (B*M, C3) or nullptr
  int64_t tiles_per_wg;
};

// (workgroups per CU where the compiler, left alone, takes more registers than the launcher's grid counts on: <1, 1, 2, 1> then runs at 143 + 32
// registers and two waves per SIMD instead of four, and its 1024 workgroups take 107 us instead of 84; <2, 1, 1, *> at two instead of three)
template <int C1B, int C2B, int C3B, int NS>
__global__ __launch_bounds__(kFT, (C1B * C2B == 1 && C3B == 2 && NS == 1) ? 4 : (C1B == 2 && C2B * C3B == 1) ? 3 : 1) void sa_fused_fwd_kernel(SaArgs p) {
  constexpr int kW2 = C1B * NS * C2B * 32 * 64, kW3 = C2B * NS * C3B * 32 * 64;
  __shared__ __attribute__((aligned(16))) unsigned char W2l[kW2];
  __shared__ __attribute__((aligned(16))) unsigned char W3l[kW3];
  __shared__ __attribute__((aligned(16))) float P1[4 * C1B * 32];
  __shared__ __attribute__((aligned(16))) float Wx[C1B * 32][4];
  __shared__ __attribute__((aligned(16))) float tiles[4][32 * kFLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int C1 = p.s.C1, C2 = p.C2, C3 = p.C3;
  stage_weight<NS>(W2l, p.W2, C2, C1, C2B * 32, C1B, tid);
  stage_weight<NS>(W3l, p.W3, C3, C2, C3B * 32, C2B, tid);
  stage_layer1<C1B>(p.s, P1, Wx, tid);
  LaneBn<C2B> bn2;
  LaneBn<C3B> bn3;
  bn2.load(p.bn2, C2, li);
  bn3.load(p.bn3, C3, li);
  __syncthreads();
  float* st = tiles[wave];
  BallPipe<C1B, false, true> pipe;   // (only the INDEX of the next ball in flight; a level without input feature has s.zf == nullptr)
  for (int g = pipe.begin(p.s, p.tiles_per_wg, wave, li, lh); g < pipe.t_end; g += 4) {
    BallRows<C1B> rc;
    pipe.rows(p.s, g, li, lh, rc);
    // ---- layer 1 (its feature part is zf) + BatchNorm 1 + ReLU in ONE pass over the row, in the operation order of gather_finish + act_rows
    // (= group_lin_rows_kernel / bn_act).  Through those two helpers -- two passes -- the instances of the default precision measured 1 - 2 %
    // slower (profiles/sa_front_end_refactor.txt), so this part stays written out here.
    float v1[C1B][4][4];
    const bool ok = rc.ok;
    const float dx = rc.p[0] - rc.q[0], dy = rc.p[1] - rc.q[1], dz = rc.p[2] - rc.q[2];
#pragma unroll
    for (int sl = 0; sl < C1B; ++sl)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int k = 32 * sl + 8 * tt + 4 * lh;
        const float4 mm = *reinterpret_cast<const float4*>(P1 + 0 * (C1B * 32) + k), ii = *reinterpret_cast<const float4*>(P1 + 1 * (C1B * 32) + k);
        const float4 gg = *reinterpret_cast<const float4*>(P1 + 2 * (C1B * 32) + k), bb = *reinterpret_cast<const float4*>(P1 + 3 * (C1B * 32) + k);
        const float pm[4] = {mm.x, mm.y, mm.z, mm.w}, pi[4] = {ii.x, ii.y, ii.z, ii.w};
        const float pg[4] = {gg.x, gg.y, gg.z, gg.w}, pb[4] = {bb.x, bb.y, bb.z, bb.w};
        const float zz[4] = {rc.z[sl][tt].x, rc.z[sl][tt].y, rc.z[sl][tt].z, rc.z[sl][tt].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4 w = *reinterpret_cast<const float4*>(&Wx[k + e][0]);
          float y = (w.x * dx + w.y * dy) + w.z * dz;
          if (p.s.zf) y = y + zz[e];
          if (!ok) y = 0.f;  // an empty slot (index -1) is an all-zero row, as in the unfused kernel
          const float a = ((y - pm[e]) * pi[e]) * pg[e] + pb[e];
          v1[sl][tt][e] = a > 0.f ? a : 0.f;
        }
      }
    // ---- layer 2 + BatchNorm 2 + ReLU -> layer 3's A fragments
    f32x16 acc2[C2B];
    layer_mfma<C1B, C2B, NS>(v1, W2l, li, lh, acc2);
    float v2[C2B][4][4];
    act_tile_rows<C2B>(acc2, bn2, st, li, lh, v2);
    // ---- layer 3 + BatchNorm 3 + ReLU + max over the 32 neighbours (first arg-max: rows ascend with the register index)
    f32x16 acc3[C3B];
    layer_mfma<C2B, C3B, NS>(v2, W3l, li, lh, acc3);
#pragma unroll
    for (int jb = 0; jb < C3B; ++jb) {
      float best = -INFINITY;
      int bk = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float a = bn3.act(jb, acc3[jb][i]);
        if (a > best) { best = a; bk = acc_row(i, lh); }
      }
      const float ob = __shfl_xor(best, 32, kWave);
      const int ok2 = __shfl_xor(bk, 32, kWave);
      if (ob > best || (ob == best && ok2 < bk)) { best = ob; bk = ok2; }
      const int col = 32 * jb + li;
      if (lh == 0 && col < C3) {
        (p.out + (size_t)g * C3)[(unsigned)col] = best;
        if (p.arg) (p.arg + (size_t)g * C3)[(unsigned)col] = (uint8_t)bk;
      }
    }
  }
}

}  // namespace

// One set-abstraction level, inference mode, in ONE kernel (see the top of the file):
//   zf (B,N,C1) = first-layer weight's feature columns applied per point (NULL: no input feature), xyz (B,N,3), centre (B,M,3),
//   index (B,M,32) int64 ball-query result (-1 = empty slot), wxyz (C1,3) = the first layer's coordinate columns,
//   bnL_* (mean, invstd = 1/sqrt(running_var + eps), gamma, beta) of the three BatchNorms, W2 (C2,C1), W3 (C3,C2) row-major
//   -> out (B,M,C3) = max_k relu(bn3(W3 relu(bn2(W2 relu(bn1(zf[j_k] + wxyz (xyz[j_k] - centre))))))), arg (B,M,C3) uint8 or NULL.
// Needs K == 32, C1, C2 <= 64, C3 <= 128 (both weight images must fit the 160 KB of LDS), multiples of 4, a split-bf16 precision, and sizes
// within the limits of sa_level (sa_common.h): MVP_EUNSUPPORTED otherwise (levels 1 and 2 of the reference configuration qualify; 3 and 4
// keep the per-layer kernels).
MVP_API int mvp_sa_fused_forward_f32(const float* zf, const float* xyz, const float* centre, const int64_t* index, const float* wxyz,
                                     int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean,
                                     const float* bn1_invstd, const float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2,
                                     const float* bn2_mean, const float* bn2_invstd, const float* bn2_gamma, const float* bn2_beta,
                                     const float* W3, int64_t C3, const float* bn3_mean, const float* bn3_invstd, const float* bn3_gamma,
                                     const float* bn3_beta, float* out, uint8_t* arg, mvp_stream_t stream) {
  SaArgs a{{}, W2, {bn2_mean, bn2_invstd, bn2_gamma, bn2_beta}, W3, {bn3_mean, bn3_invstd, bn3_gamma, bn3_beta}, (int)C2, (int)C3, out, arg, 0};
  MVP_NONNULL(W3);
  MVP_NONNULL(out);
  for (int i = 0; i < 4; ++i) {
    MVP_NONNULL(a.bn2[i]);
    MVP_NONNULL(a.bn3[i]);
  }
  const int ns = mlp_fwd_pieces();
  SaLevel lv;
  const int rc = sa_level(zf, false, xyz, centre, index, wxyz, B, N, M, K, C1, {bn1_mean, bn1_invstd, bn1_gamma, bn1_beta}, W2, C2, C3,
                          C3 > 0, ns != 0 && (uintptr_t)zf % 16 == 0, &lv);
  if (rc != MVP_OK || lv.s.G == 0) return rc;
  a.s = lv.s;
  // (the estimate counts a 96-wide last layer as the 3 blocks it fills, not the 4 it runs as; no cap beyond 4 workgroups per CU)
  const int64_t lds = (int64_t)ns * 2048 * (lv.c1b * lv.c2b + lv.c2b * cdiv(C3, 32)) + 24 * 1024;
  const unsigned grid = sa_grid(lv.s.G, lds, 4, INT64_MAX, &a.tiles_per_wg);
  hipStream_t s = static_cast<hipStream_t>(stream);
  using Shapes = SaTable<SaRow<1, 1, 1>, SaRow<1, 1, 2>, SaRow<1, 2, 1>, SaRow<1, 2, 2>, SaRow<1, 2, 4>, SaRow<2, 1, 1>, SaRow<2, 1, 2>, SaRow<2, 2, 1>,
                         SaRow<2, 2, 2>, SaRow<2, 2, 4>>;
  // (sa_pick hands the matching row of a table to the lambda as a value of its own TYPE, SaRow<...>: decltype(row)::v[k] is the row's
  // k-th entry as a compile-time constant, usable as a template argument)
  const bool found = sa_pick(Shapes{}, {lv.c1b, lv.c2b, lv.c3b}, [&](auto sh) {
    sa_pick(SaPieces{}, {ns}, [&](auto pc) {
      hipLaunchKernelGGL((sa_fused_fwd_kernel<decltype(sh)::v[0], decltype(sh)::v[1], decltype(sh)::v[2], decltype(pc)::v[0]>), dim3(grid), dim3(kFT), 0, s, a);
    });
  });
  return found ? mvp_launch_status() : MVP_EUNSUPPORTED;
}

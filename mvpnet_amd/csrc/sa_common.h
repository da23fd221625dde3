// sa_common.h -- what the fused set-abstraction kernels share (sa_fused.hip: inference; sa_train.hip: training; layouts at the top of
// sa_train.hip): the resident weight image in B-fragment order, one shared-MLP layer on a wave's 32-row tile, the per-ball FRONT END --
// the level's input (SaSrc), the first-layer tables, the gather of a ball's rows with the next balls' loads in flight (BallPipe),
// BatchNorm + ReLU in row and in accumulator layout, the wave-private tile between the two -- and the host side of a launch: argument
// checks, block counts, shape dispatch and grid size (sa_level, sa_pick, sa_grid).
#pragma once
#include "mlp_common.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int kFT = 256;
constexpr int kFLd = 36;

// accumulator layout: the row (neighbour) that register q of a lane in half h holds
__device__ __forceinline__ constexpr int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// weight image of one layer: [slab][piece][col] x 64 bytes, 16-byte units XOR-swizzled (see mlp_stream.hip)
template <int NS>
__device__ __forceinline__ void stage_weight(unsigned char* Wl, const float* __restrict__ W, int Cout, int Cin, int cols, int slabs, int tid) {
  for (int t = tid; t < cols * slabs * 8; t += kFT) {
    const int co = t % cols, kqi = t / cols;
    const int k = 4 * kqi;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (co < Cout && k + e < Cin) ? W[(size_t)co * Cin + k + e] : 0.f;
    unsigned lo[NS], hi[NS];
    split_pair<NS>(v[0], v[1], lo);
    split_pair<NS>(v[2], v[3], hi);
    const int slab = kqi >> 3, kq = (kqi & 7) * 4;
    const int tt = kq >> 3, hh = (kq >> 2) & 1;
    const int unit = 2 * (tt >> 1) + hh, half = tt & 1;
#pragma unroll
    for (int pc = 0; pc < NS; ++pc)
      *reinterpret_cast<uint2*>(Wl + ((size_t)(slab * NS + pc) * cols + co) * 64 + ((unit ^ ((co >> 2) & 3)) * 16) + half * 8) = make_uint2(lo[pc], hi[pc]);
  }
}

// one layer: A fragments of `KS` slabs (v[sl][tt][e] activated values of this lane's row) x the resident image -> acc[NB]
template <int KS, int NB, int NS>
__device__ __forceinline__ void layer_mfma(const float (&v)[KS][4][4], const unsigned char* Wl, int li, int lh, f32x16 (&acc)[NB]) {
  using SP = SplitPairs<NS>;
  constexpr int kCols = NB * 32;
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
#pragma unroll
  for (int sl = 0; sl < KS; ++sl)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      unsigned q0[NS], q1[NS], q2[NS], q3[NS];
      split_pair<NS>(v[sl][2 * s][0], v[sl][2 * s][1], q0);
      split_pair<NS>(v[sl][2 * s][2], v[sl][2 * s][3], q1);
      split_pair<NS>(v[sl][2 * s + 1][0], v[sl][2 * s + 1][1], q2);
      split_pair<NS>(v[sl][2 * s + 1][2], v[sl][2 * s + 1][3], q3);
      u32x4 af[NS];
#pragma unroll
      for (int pc = 0; pc < NS; ++pc) af[pc] = u32x4{q0[pc], q1[pc], q2[pc], q3[pc]};
      constexpr int JG = NB >= 2 ? 2 : 1;
#pragma unroll
      for (int j0 = 0; j0 < NB; j0 += JG) {
        u32x4 bfr[JG][NS];
#pragma unroll
        for (int jj = 0; jj < JG; ++jj) {
          const int co = 32 * (j0 + jj) + li;
#pragma unroll
          for (int pc = 0; pc < NS; ++pc)
            bfr[jj][pc] = *reinterpret_cast<const u32x4*>(Wl + ((size_t)(sl * NS + pc) * kCols + co) * 64 + (((2 * s + lh) ^ ((co >> 2) & 3)) * 16));
        }
#pragma unroll
        for (int qd = 0; qd < SP::N; ++qd)
#pragma unroll
          for (int jj = 0; jj < JG; ++jj)
            acc[j0 + jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[SP::A[qd]]),
                                                                   __builtin_bit_cast(bf16x8, bfr[jj][SP::B[qd]]), acc[j0 + jj], 0, 0, 0);
      }
    }
  // (Round 3 found the -O3 build of the narrow variants returning run-to-run different results on a few in a million balls.  The cause
  // was not this kernel's schedule but a packed fp32 op with an op_sel source swizzle -- the SLP vectoriser's pairing of the
  // normalise / ReLU arithmetic -- misexecuting while other waves of the workgroup run MFMA on the same SIMD; see the Makefile, which
  // builds this file without that vectoriser, tests/test_isa_cpu.py and DESIGN.md 4.10.  tools/exp/sa_fused_count.py: 10248 corrupted
  // balls in 400 launches with the op_sel'd forms in the binary, 0 without them.)
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the per-ball front end
// ---------------------------------------------------------------------------------------------------------------------------------
struct SaSrc {            // the level's input: what y_1 is re-created from
  const float* zf;        // (B, N, C1): first-layer feature columns applied per point (inference: nullptr = a level without input feature)
  const float* xyz;       // (B, N, 3)
  const float* centre;    // (B, M, 3)
  const int64_t* index;   // (B, M, 32) ball query result (-1 = empty slot: an all-zero row, as in group_lin_rows_kernel)
  const float* wxyz;      // (C1, 3) first layer's coordinate columns
  const float* bn1[4];    // BatchNorm 1: mean, invstd, gamma, beta
  int64_t G;              // B * M balls
  int N, M, C1;
};

// first-layer tables of a workgroup: BatchNorm 1 per input channel of layer 2 (k runs along the registers in row layout) and the
// coordinate columns (wx, wy, wz, 0) per channel
template <int C1B>
__device__ __forceinline__ void stage_layer1(const SaSrc& p, float* P1 /* [4][C1B*32] */, float (*Wx)[4], int tid) {
  for (int k = tid; k < C1B * 32; k += kFT) {
    const int kc = min(k, p.C1 - 1);
#pragma unroll
    for (int a = 0; a < 4; ++a) P1[a * (C1B * 32) + k] = p.bn1[a] ? p.bn1[a][kc] : 0.f;
    Wx[k][0] = k < p.C1 ? p.wxyz[k * 3 + 0] : 0.f;
    Wx[k][1] = k < p.C1 ? p.wxyz[k * 3 + 1] : 0.f;
    Wx[k][2] = k < p.C1 ? p.wxyz[k * 3 + 2] : 0.f;
    Wx[k][3] = 0.f;
  }
}

// y_1 of ball g, row layout: v[sl][tt][e] = zf[j][k] + wxyz[k] . (xyz[j] - centre[g]),  k = 32 sl + 8 tt + 4 lh + e  (same operation
// order as group_lin_rows_kernel: (wx dx + wy dy) + wz dz, then + zf; an empty slot is a zero row).  In two halves: the loads of the NEXT
// ball are issued before the current one is worked on (a wave has one or two partners on its SIMD: nothing else hides the gather's
// round trip through L2 / MALL).  NOZF (gather_issue, BallPipe): the level may come without input feature (p.zf == nullptr, tested at run
// time: the inference kernel, which finishes the row itself); the training kernels instantiate the helpers without it and carry no such test.
template <int C1B>
struct BallRows {
  float4 z[C1B][4];
  float p[3], q[3];
  bool ok;
};
// (g: the wave's ball, a SCALAR -- callers pass it through readfirstlane --, so the chunk index, its division and the row bases are scalar
// arithmetic and the per-lane part of every address is a 32-bit offset: the 64-bit per-lane address arithmetic of the first version was 8 - 10 %
// of these VALU-bound kernels' vector instructions.  sa_level refuses the sizes these 32-bit offsets cannot hold.)
template <int C1B, bool NOZF = false>
__device__ __forceinline__ void gather_issue(const SaSrc& p, int g, int64_t j, int lh, BallRows<C1B>& r) {
  const int b = g / p.M;
  r.ok = j >= 0 && j < p.N;
  const unsigned jj = r.ok ? (unsigned)j : 0u;
  if (!NOZF || p.zf) {
    const float* zr = p.zf + (size_t)b * p.N * p.C1 + jj * (unsigned)p.C1;
#pragma unroll
    for (int sl = 0; sl < C1B; ++sl)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) r.z[sl][tt] = *reinterpret_cast<const float4*>(zr + min(32 * sl + 8 * tt + 4 * lh, p.C1 - 4));
  }
  const float* pp = p.xyz + (size_t)b * p.N * 3 + jj * 3u;
  const float* qc = p.centre + (size_t)g * 3;
  r.p[0] = pp[0]; r.p[1] = pp[1]; r.p[2] = pp[2];
  r.q[0] = qc[0]; r.q[1] = qc[1]; r.q[2] = qc[2];
}
template <int C1B>
__device__ __forceinline__ void gather_finish(const BallRows<C1B>& r, int lh, const float (*Wx)[4], float (&v)[C1B][4][4], float (&diff)[3]) {
  const bool ok = r.ok;
  const float dx = r.p[0] - r.q[0], dy = r.p[1] - r.q[1], dz = r.p[2] - r.q[2];
  diff[0] = ok ? dx : 0.f;
  diff[1] = ok ? dy : 0.f;
  diff[2] = ok ? dz : 0.f;
#pragma unroll
  for (int sl = 0; sl < C1B; ++sl)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int k = 32 * sl + 8 * tt + 4 * lh;
      const float zz[4] = {r.z[sl][tt].x, r.z[sl][tt].y, r.z[sl][tt].z, r.z[sl][tt].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float4 w = *reinterpret_cast<const float4*>(&Wx[k + e][0]);
        float y = (w.x * dx + w.y * dy) + w.z * dz;
        y = y + zz[e];
        v[sl][tt][e] = ok ? y : 0.f;
      }
    }
}

// The balls of a wave -- t_begin + wave, + 4, ... below t_end -- with the loads of the later ones in flight: the neighbour index of ball
// g + 4 and, with PF, the rows of ball g + 4 and the index of ball g + 8 while ball g is worked on.
//   BallPipe<..> pipe;  for (int g = pipe.begin(src, tiles_per_wg, wave, li, lh); g < pipe.t_end; g += 4) { pipe.rows(src, g, li, lh, rc); ... }
template <int C1B, bool PF, bool NOZF = false>
struct BallPipe {
  BallRows<C1B> rn;   // PF: the rows of the next ball
  int64_t jn;         // this lane's neighbour in the next ball (PF: in the one after)
  int64_t t_end;
  __device__ __forceinline__ int begin(const SaSrc& p, int64_t tiles_per_wg, int wave, int li, int lh) {
    const int64_t t_begin = (int64_t)blockIdx.x * tiles_per_wg;
    t_end = min(p.G, t_begin + tiles_per_wg);
    const int g = __builtin_amdgcn_readfirstlane((int)(t_begin + wave));   // (the wave's ball: scalar -- see gather_issue)
    jn = -1;
    if (PF) {
      if (g < t_end) gather_issue<C1B, NOZF>(p, g, p.index[(size_t)g * 32 + li], lh, rn);
      if (g + 4 < t_end) jn = p.index[(size_t)(g + 4) * 32 + li];
    } else if (g < t_end) {
      jn = p.index[(size_t)g * 32 + li];
    }
    return g;
  }
  __device__ __forceinline__ void rows(const SaSrc& p, int g, int li, int lh, BallRows<C1B>& rc) {
    if (PF) {
      rc = rn;
      if (g + 4 < t_end) {
        gather_issue<C1B, NOZF>(p, g + 4, jn, lh, rn);
        if (g + 8 < t_end) jn = p.index[(size_t)(g + 8) * 32 + li];
      }
    } else {
      const int64_t j = jn;
      if (g + 4 < t_end) jn = p.index[(size_t)(g + 4) * 32 + li];
      gather_issue<C1B, NOZF>(p, g, j, lh, rc);
    }
  }
};

// a_1 = relu(bn_1(y_1)) in place, row layout
template <int C1B>
__device__ __forceinline__ void act_rows(float (&v)[C1B][4][4], const float* P1, int lh) {
#pragma unroll
  for (int sl = 0; sl < C1B; ++sl)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int k = 32 * sl + 8 * tt + 4 * lh;
      const float4 mm = *reinterpret_cast<const float4*>(P1 + 0 * (C1B * 32) + k), ii = *reinterpret_cast<const float4*>(P1 + 1 * (C1B * 32) + k);
      const float4 gg = *reinterpret_cast<const float4*>(P1 + 2 * (C1B * 32) + k), bb = *reinterpret_cast<const float4*>(P1 + 3 * (C1B * 32) + k);
      const float pm[4] = {mm.x, mm.y, mm.z, mm.w}, pi[4] = {ii.x, ii.y, ii.z, ii.w};
      const float pg[4] = {gg.x, gg.y, gg.z, gg.w}, pb[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = ((v[sl][tt][e] - pm[e]) * pi[e]) * pg[e] + pb[e];
        v[sl][tt][e] = a > 0.f ? a : 0.f;
      }
    }
}

// per-lane (= per output channel, accumulator layout) BatchNorm constants of NB channel blocks; columns past C repeat the last one
template <int NB>
struct LaneBn {
  float m[NB], i[NB], g[NB], b[NB];
  __device__ __forceinline__ void load(const float* const (&bn)[4], int C, int li) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int col = min(32 * j + li, C - 1);
      m[j] = bn[0][col]; i[j] = bn[1][col]; g[j] = bn[2][col]; b[j] = bn[3][col];
    }
  }
  __device__ __forceinline__ float act(int j, float y) const {
    const float a = ((y - m[j]) * i[j]) * g[j] + b[j];
    return a > 0.f ? a : 0.f;
  }
};

// relu(bn(acc)), accumulator layout -> through the wave-private tile `st` (written as columns, read back as rows) -> row layout: the next
// layer's A fragments
template <int NB>
__device__ __forceinline__ void act_tile_rows(const f32x16 (&acc)[NB], const LaneBn<NB>& bn, float* st, int li, int lh, float (&v)[NB][4][4]) {
#pragma unroll
  for (int jb = 0; jb < NB; ++jb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) st[acc_row(i, lh) * kFLd + li] = bn.act(jb, acc[jb][i]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const float4 a = *reinterpret_cast<const float4*>(st + li * kFLd + 8 * tt + 4 * lh);
      v[jb][tt][0] = a.x; v[jb][tt][1] = a.y; v[jb][tt][2] = a.z; v[jb][tt][3] = a.w;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// row c of the wave-private tile, row step s (channels 16 s + 8 t + 4 h + e) -> split bf16 A fragments
template <int NS>
__device__ __forceinline__ void tile_row_frags(const float* tile, int c, int h, int s, u32x4 (&f)[NS]) {
  const float4 v0 = *reinterpret_cast<const float4*>(tile + c * kFLd + 16 * s + 4 * h);
  const float4 v1 = *reinterpret_cast<const float4*>(tile + c * kFLd + 16 * s + 8 + 4 * h);
  unsigned q0[NS], q1[NS], q2[NS], q3[NS];
  split_pair<NS>(v0.x, v0.y, q0);
  split_pair<NS>(v0.z, v0.w, q1);
  split_pair<NS>(v1.x, v1.y, q2);
  split_pair<NS>(v1.z, v1.w, q3);
#pragma unroll
  for (int pc = 0; pc < NS; ++pc) f[pc] = u32x4{q0[pc], q1[pc], q2[pc], q3[pc]};
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the host side of a launch
// ---------------------------------------------------------------------------------------------------------------------------------
// channel blocks of a layer: rounded up to 1, 2 or 4 (a 96-wide layer runs as 4 blocks with a zero block)
inline int blocks_of(int64_t c) { return c <= 32 ? 1 : c <= 64 ? 2 : 4; }

struct SaLevel {
  SaSrc s;          // s.G == 0: an empty level, nothing to launch
  int c1b, c2b, c3b;
};

// What the three entry points check and fill alike, after the entry point's own pointers: the level's pointers (MVP_ENULL: every null
// check comes before any other), then the sizes, the entry point's own (`own_sizes`) included (MVP_EINVAL), then what the kernels do not
// support (MVP_EUNSUPPORTED) -- the entry point's own conditions `own_ok` (a split-bf16 precision, alignment), the widths (C3 == 0: a pass
// that stops at layer 2) and the limits of the 32-bit ball and row-offset arithmetic: N, M <= INT_MAX, B * M <= 2^31 - 16 (the ball loops
// form g + 8), N * max(C1, 3) < 2^32.  y2: the stored y_2 (B*M*32, C2) of a training pass that writes or reads it, or nullptr -- 16-byte aligned
// rows (C2 % 4 == 0 holds for every level).
inline int sa_level(const float* zf, bool zf_required, const float* xyz, const float* centre, const int64_t* index, const float* wxyz, int64_t B,
                    int64_t N, int64_t M, int64_t K, int64_t C1, const float* const (&bn1)[4], const float* W2, int64_t C2, int64_t C3,
                    bool own_sizes, bool own_ok, SaLevel* lv, const float* y2 = nullptr) {
  if (zf_required) MVP_NONNULL(zf);
  MVP_NONNULL(xyz);
  MVP_NONNULL(centre);
  MVP_NONNULL(index);
  MVP_NONNULL(wxyz);
  for (const float* q : bn1) MVP_NONNULL(q);
  MVP_NONNULL(W2);
  MVP_REQUIRE(B >= 0 && N > 0 && M >= 0 && K > 0 && C1 > 0 && C2 > 0 && C3 >= 0 && own_sizes);
  const bool widths = K == 32 && C1 >= 4 && C1 <= 64 && C2 <= 64 && C3 <= 128 && C1 % 4 == 0 && C2 % 4 == 0 && C3 % 4 == 0;
  if (!own_ok || !widths || (uintptr_t)y2 % 16 != 0) return MVP_EUNSUPPORTED;
  constexpr int64_t kBalls = (int64_t(1) << 31) - 16, kOffsets = (int64_t(1) << 32) - 1;
  if (N > INT_MAX || M > INT_MAX || (M > 0 && B > kBalls / M) || N > kOffsets / std::max<int64_t>(C1, 3)) return MVP_EUNSUPPORTED;
  lv->s = SaSrc{zf, xyz, centre, index, wxyz, {bn1[0], bn1[1], bn1[2], bn1[3]}, B * M, (int)N, (int)M, (int)C1};
  lv->c1b = blocks_of(C1); lv->c2b = blocks_of(C2); lv->c3b = C3 ? blocks_of(C3) : 1;
  return MVP_OK;
}

// Shape dispatch: a table is a list of rows of template arguments; sa_pick calls f(Row{}) for the row that equals `key` and returns whether
// there is one.  Only the rows of the tables an entry point passes are instantiated.
template <int... V>
struct SaRow { static constexpr int v[sizeof...(V)] = {V...}; };
template <class... Rows>
struct SaTable {};
template <int... V>
inline bool sa_row_is(SaRow<V...>, const int (&key)[sizeof...(V)]) {
  int i = 0;
  return ((key[i++] == V) && ...);
}
template <class... Rows, int N, class F>
inline bool sa_pick(SaTable<Rows...>, const int (&key)[N], F&& f) {
  return ((sa_row_is(Rows{}, key) ? (f(Rows{}), true) : false) || ...);
}
// (c1b, c2b, c3b): the block shapes of a pass through all three layers, and of one that stops at layer 2 (stage 2, layer-2 backward)
using SaShapes3 = SaTable<SaRow<1, 1, 1>, SaRow<1, 1, 2>, SaRow<1, 2, 1>, SaRow<1, 2, 2>, SaRow<2, 1, 1>, SaRow<2, 1, 2>, SaRow<2, 2, 1>, SaRow<2, 2, 2>,
                          SaRow<2, 2, 4>>;   // (2, 2, 4) = (64, 64, 128): level 2 of the reference network
using SaShapes2 = SaTable<SaRow<1, 1, 1>, SaRow<1, 2, 1>, SaRow<2, 1, 1>, SaRow<2, 2, 1>>;
using SaPieces = SaTable<SaRow<1>, SaRow<2>, SaRow<3>>;

// persistent workgroups: as many per CU as LDS -- and `max_per_cu`, what the kernel's registers allow -- let be resident AT ONCE (a launch of
// 768 workgroups on 512 slots runs two rounds for the work of one and a half), at most `max_wgs` in all
inline unsigned sa_grid(int64_t G, int64_t lds_bytes, int64_t max_per_cu, int64_t max_wgs, int64_t* tiles_per_wg) {
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(max_per_cu, (150 * 1024) / lds_bytes));
  const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(max_wgs, 256 * per_cu), cdiv(G, 16)));
  *tiles_per_wg = cdiv(cdiv(G, wgs), 4) * 4;
  return (unsigned)cdiv(G, *tiles_per_wg);
}

}  // namespace

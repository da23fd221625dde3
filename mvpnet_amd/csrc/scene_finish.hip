// scene_finish.hip -- what every whole-scene test script does behind its scene logits, for gfx950: the model ensemble of
// mvpnet/ensemble.py:45-49 (sum of per-model softmaxes, argmax) in ONE launch, and the label confusion matrix of
// mvpnet/evaluate_3d.py:11-40 (sklearn's confusion_matrix(gt, pred, labels=...)) without a host copy.  Definitions: include/mvp_hip.h
// (mvp_ensemble_softmax_f32, mvp_label_confusion_i64).
//
//   ensemble_softmax_kernel : a streaming kernel, M*n*C*4 bytes in, n*(C*4 + 8) out.  A GROUP of G lanes owns one row, lane g of it VEC
//                             consecutive classes (the lane layout of lift_vote.hip): the row of every model, the probabilities and their
//                             sum live in registers.  All M rows are requested before the first is used.  The class-order sum is a chain
//                             through the group's lanes, the maximum and the argmax are butterflies inside it.  No atomics.
//   label_confusion_kernel  : position of gt and pred through the tables, a workgroup-private LDS histogram flushed with integer atomics
//                             (seg.hip's seg_confusion_kernel); global atomics when C*C does not fit the LDS table.
#include "chunk_common.h"  // nan_max
#include <math.h>
#include <algorithm>

namespace {

constexpr int kEnsThreads = 256;

struct EnsRows {
  const float* x[MVP_ENSEMBLE_MAX_MODELS];
};

template <int G, int VEC>
__global__ __launch_bounds__(kEnsThreads) void ensemble_softmax_kernel(EnsRows in, int M, int C, int64_t n, int64_t ld_r, int64_t ld_c,
                                                                       float* __restrict__ prob, int64_t* __restrict__ label) {
  const int64_t p = ((int64_t)blockIdx.x * kEnsThreads + threadIdx.x) / G;
  if (p >= n) return;  // (whole groups leave: G divides the workgroup, and a lane only ever reads lanes of its own group)
  const int g = (int)threadIdx.x & (G - 1);
  const int lead = ((int)threadIdx.x & (kWave - 1)) & ~(G - 1);
  const int c0 = g * VEC;
  const bool mine = c0 < C;              // (VEC = 4 comes with C % 4 == 0: a lane owns four classes or none)
  const int owners = (C + VEC - 1) / VEC;  // lanes of the group that own classes
  float x[MVP_ENSEMBLE_MAX_MODELS][VEC];
#pragma unroll
  for (int m = 0; m < MVP_ENSEMBLE_MAX_MODELS; ++m) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) x[m][v] = -INFINITY;
    if (m < M && mine) {
      const float* row = in.x[m] + p * ld_r;
      if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(row + c0);
        x[m][0] = q.x, x[m][1] = q.y, x[m][2] = q.z, x[m][3] = q.w;
      } else {
        x[m][0] = row[(int64_t)c0 * ld_c];
      }
    }
  }
  float P[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) P[v] = 0.f;
#pragma unroll
  for (int m = 0; m < MVP_ENSEMBLE_MAX_MODELS; ++m) {
    if (m < M) {  // (uniform)
      float mx = x[m][0];
#pragma unroll
      for (int v = 1; v < VEC; ++v) mx = nan_max(mx, x[m][v]);
#pragma unroll
      for (int k = G / 2; k >= 1; k >>= 1) mx = nan_max(mx, __shfl_xor(mx, k, kWave));
      float e[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) e[v] = mine ? expf(x[m][v] - mx) : 0.f;
      // s = ((e_0 + e_1) + ...) in class order: owner j takes the running sum of owner j - 1 and adds its own classes (0 + e_0 is e_0)
      float run = 0.f;
      for (int j = 0; j < owners; ++j) {
        float t = 0.f;
        if (G > 1) t = __shfl(run, lead + (j ? j - 1 : 0), kWave);
        if (g == j) {
          t = j ? t : 0.f;
#pragma unroll
          for (int v = 0; v < VEC; ++v) t += e[v];
          run = t;
        }
      }
      const float s = G > 1 ? __shfl(run, lead + owners - 1, kWave) : run;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float q = __fdiv_rn(e[v], s);
        P[v] = m == 0 ? q : P[v] + q;
      }
    }
  }
  // the first maximum by strict `>` from P_0: a NaN never wins, so an all-NaN row keeps class 0
  float bv = mine ? P[0] : -INFINITY;
  int bi = mine ? c0 : 0x7fffffff;
#pragma unroll
  for (int v = 1; v < VEC; ++v)
    if (mine && P[v] > bv) bv = P[v], bi = c0 + v;
#pragma unroll
  for (int k = G / 2; k >= 1; k >>= 1) {
    const float ov = __shfl_xor(bv, k, kWave);
    const int oi = __shfl_xor(bi, k, kWave);
    if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
  }
  if (g == 0) label[p] = bi;
  if (prob != nullptr && mine) {
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(prob + p * C + c0) = make_float4(P[0], P[1], P[2], P[3]);
    } else {
      prob[p * C + c0] = P[0];
    }
  }
}

constexpr int kConfThreads = 256;
constexpr int kConfHist = 4096;  // C <= 64

// position of a label value: through the table (entries outside [0,C) count as "not a label"), or the value itself
__device__ __forceinline__ int label_position(int64_t v, const int32_t* __restrict__ lut, int64_t L, int C) {
  if (lut != nullptr) {
    if (v < 0 || v >= L) return -1;
    const int q = lut[v];
    return q >= 0 && q < C ? q : -1;
  }
  return v >= 0 && v < C ? (int)v : -1;
}

__global__ __launch_bounds__(kConfThreads) void label_confusion_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int64_t n,
                                                                        int C, const int32_t* __restrict__ pred_lut, int64_t Lp,
                                                                        const int32_t* __restrict__ gt_lut, int64_t Lg,
                                                                        unsigned long long* __restrict__ mat) {
  __shared__ unsigned int hist[kConfHist];
  const bool lds = C * C <= kConfHist;
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += kConfThreads) hist[i] = 0u;
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * kConfThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kConfThreads) {
    const int row = label_position(gt[r], gt_lut, Lg, C), col = label_position(pred[r], pred_lut, Lp, C);
    if (row < 0 || col < 0) continue;
    if (lds)
      atomicAdd(&hist[row * C + col], 1u);
    else
      atomicAdd(mat + (int64_t)row * C + col, 1ull);
  }
  __syncthreads();
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += kConfThreads)
      if (hist[i]) atomicAdd(mat + i, (unsigned long long)hist[i]);
}

}  // namespace

MVP_API int mvp_ensemble_softmax_f32(const float* const* logits, int64_t M, int64_t n, int64_t C, int64_t ld_r, int64_t ld_c, float* prob,
                                     int64_t* label, mvp_stream_t stream) {
  MVP_NONNULL(logits);
  MVP_NONNULL(label);
  for (int64_t m = 0; m < M && m < MVP_ENSEMBLE_MAX_MODELS; ++m) MVP_NONNULL(logits[m]);
  MVP_REQUIRE(M >= 1 && C >= 1 && n >= 0 && ld_r >= 0 && ld_c >= 0);
  if (M > MVP_ENSEMBLE_MAX_MODELS || C > 64 || n >= (1ll << 31)) return MVP_EUNSUPPORTED;
  if (n == 0) return MVP_OK;
  EnsRows in;
  bool vec = C % 4 == 0 && ld_c == 1 && ld_r % 4 == 0 && (uintptr_t)prob % 16 == 0;
  for (int m = 0; m < MVP_ENSEMBLE_MAX_MODELS; ++m) {
    in.x[m] = logits[m < M ? m : 0];
    vec = vec && (uintptr_t)in.x[m] % 16 == 0;
  }
  const int lanes = (int)(vec ? C / 4 : C);
  int G = 1;
  while (G < lanes) G *= 2;
  const dim3 grid((unsigned)cdiv(n * G, kEnsThreads)), block(kEnsThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define MVP_ENS_LAUNCH(GG, VV) \
  hipLaunchKernelGGL((ensemble_softmax_kernel<GG, VV>), grid, block, 0, s, in, (int)M, (int)C, n, ld_r, ld_c, prob, label)
  if (vec) {
    switch (G) {
      case 1: MVP_ENS_LAUNCH(1, 4); break;
      case 2: MVP_ENS_LAUNCH(2, 4); break;
      case 4: MVP_ENS_LAUNCH(4, 4); break;
      case 8: MVP_ENS_LAUNCH(8, 4); break;
      default: MVP_ENS_LAUNCH(16, 4); break;
    }
  } else {
    switch (G) {
      case 1: MVP_ENS_LAUNCH(1, 1); break;
      case 2: MVP_ENS_LAUNCH(2, 1); break;
      case 4: MVP_ENS_LAUNCH(4, 1); break;
      case 8: MVP_ENS_LAUNCH(8, 1); break;
      case 16: MVP_ENS_LAUNCH(16, 1); break;
      case 32: MVP_ENS_LAUNCH(32, 1); break;
      default: MVP_ENS_LAUNCH(64, 1); break;
    }
  }
#undef MVP_ENS_LAUNCH
  return mvp_launch_status();
}

MVP_API int mvp_label_confusion_i64(const int64_t* pred, const int64_t* gt, int64_t n, int64_t C, const int32_t* pred_lut, int64_t Lp,
                                    const int32_t* gt_lut, int64_t Lg, int64_t* mat, mvp_stream_t stream) {
  MVP_NONNULL(pred);
  MVP_NONNULL(gt);
  MVP_NONNULL(mat);
  MVP_REQUIRE(n >= 0 && C >= 1 && Lp >= 0 && Lg >= 0 && (pred_lut == nullptr) == (Lp == 0) && (gt_lut == nullptr) == (Lg == 0));
  if (C > MVP_CONFUSION_MAX_CLASSES) return MVP_EUNSUPPORTED;
  if (n == 0) return MVP_OK;
  const unsigned blocks = (unsigned)std::min<int64_t>(256, cdiv(n, kConfThreads));
  hipLaunchKernelGGL(label_confusion_kernel, dim3(blocks), dim3(kConfThreads), 0, static_cast<hipStream_t>(stream), pred, gt, n, (int)C, pred_lut,
                     Lp, gt_lut, Lg, reinterpret_cast<unsigned long long*>(mat));
  return mvp_launch_status();
}

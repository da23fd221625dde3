// seg.hip -- the step after the path: weighted softmax cross-entropy with ignore_index
// (mvpnet/models/loss.py:5-21 = F.cross_entropy(logit (B,C,N), label (B,N), weight, ignore_index), mean reduction)
// forward + backward, and the confusion matrix of argmax(logit) against the labels (mvpnet/models/metric.py:13-53:
// argmax + mask + bincount).  gfx950 only.
//
// Both read the logits where the network left them: element (b, c, n) at logit[b*ld_b + c*ld_c + n*ld_n], so the
// reference's (B,C,N) tensor (ld_c = N, ld_n = 1: lanes walk n, coalesced) and the channels-last rows the MFMA kernels
// produce ((B*N, C): B = 1, ld_n = C, ld_c = 1) are both consumed without a transpose copy.  C is small (20 classes):
// one point per lane, the C logits are read twice (max, then sum of exponentials) straight from L1/L2 -- no
// (B,C,N) log-probability tensor is ever written, which is what ATen's log_softmax + nll_loss pair does.
#include "common.h"
#include <algorithm>

namespace {

constexpr int kST = 256;

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kST / kWave; ++w) t += red[w];
  __syncthreads();
  return t;  // valid in thread 0
}

// -log softmax(x)[y] of one point, fp32 like torch's log_softmax: (max + log(sum exp(x - max))) - x[y].
// Up to kRegC classes the point's logits are loaded ONCE, all loads in flight together (a run-time loop over C made every
// load wait for the previous one: 70 us for the 262144 x 20 batch); more classes take the two-pass loop.
constexpr int kRegC = 32;
__device__ __forceinline__ float row_lse(const float* __restrict__ p, int64_t ld_c, int C, float* mx_out, float* x /* kRegC */) {
  float mx, se = 0.f;
  if (C <= kRegC) {
    if (ld_c == 1 && (C & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      // channels-last rows (the layout PN2SSG hands out): the point's C logits are C / 4 16-byte loads instead of 32 4-byte ones whose
      // lanes sit 4 C bytes apart (34 -> ~12 us for the 262144 x 20 batch); same values, same arithmetic
#pragma unroll
      for (int q = 0; q < kRegC / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4 * min(q, C / 4 - 1));  // quads >= C / 4 repeat the last one
        x[4 * q + 0] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < kRegC; ++c) x[c] = p[(int64_t)min(c, C - 1) * ld_c];
    }
    mx = x[0];
#pragma unroll
    for (int c = 1; c < kRegC; ++c) mx = fmaxf(mx, x[c]);  // entries >= C repeat the last class
#pragma unroll
    for (int c = 0; c < kRegC; ++c)
      if (c < C) se += expf(x[c] - mx);
  } else {
    mx = p[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[(int64_t)c * ld_c]);
    for (int c = 0; c < C; ++c) se += expf(p[(int64_t)c * ld_c] - mx);
  }
  *mx_out = mx;
  return logf(se);
}

// ---- channels-last rows, C % 4 == 0, C <= kRegC, contiguous and 16-byte aligned: the wave-coalesced path -------------------------
// A wave's 64 rows are 64 * C contiguous floats.  With one row per lane straight from memory the lanes of a load sit 4 C bytes apart
// (every 16-byte load of the wave touches 64 different places).  Here lane l loads quads l, l + 64, ... of the wave's block -- C / 4
// fully coalesced 16-byte loads, nothing past C -- and the wave's slice of LDS hands each lane its own row (and takes the gradient
// rows back the same way).  Same values into the same arithmetic as row_lse: results do not change.
constexpr int kRegQ = kRegC / 4;
typedef float4 SegTile[kWave * kRegQ];  // one wave's 64 rows of up to kRegC floats (8 KB)

__device__ __forceinline__ bool seg_rows_layout(const float* p, int64_t B, int C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n) {
  return ld_c == 1 && ld_n == C && (B == 1 || ld_b == N * C) && (C & 3) == 0 && C <= kRegC && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// x[0 .. 4 Q) = logits of row (row0 + lane), row0 = first row of this wave's 64; rows >= R read as zeros.  Block-uniform call.
template <int Q>
__device__ __forceinline__ void seg_load_rows(const float* __restrict__ logit, int64_t row0, int64_t R, float4* tile, float* x) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t q0 = row0 * Q, nq = R * Q;
  float4 v[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int64_t k = q0 + lane + i * kWave;
    v[i] = k < nq ? *reinterpret_cast<const float4*>(logit + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();  // the tile's previous readers are done
#pragma unroll
  for (int i = 0; i < Q; ++i) tile[lane + i * kWave] = v[i];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const float4 t = tile[lane * Q + q];
    x[4 * q + 0] = t.x; x[4 * q + 1] = t.y; x[4 * q + 2] = t.z; x[4 * q + 3] = t.w;
  }
}

// row_lse on registers: same max (row_lse's entries >= C repeat the last class), same sum order
template <int Q>
__device__ __forceinline__ float regs_lse(const float* x, float* mx_out) {
  float mx = x[0], se = 0.f;
#pragma unroll
  for (int c = 1; c < 4 * Q; ++c) mx = fmaxf(mx, x[c]);
#pragma unroll
  for (int c = 0; c < 4 * Q; ++c) se += expf(x[c] - mx);
  *mx_out = mx;
  return logf(se);
}

// One workgroup's share of the forward sums on this layout: the same rows per lane, in the same order, as the strided loop.
template <int Q>
__device__ __forceinline__ void seg_loss_rows(const float* __restrict__ logit, int64_t R, const int64_t* __restrict__ label,
                                              const float* __restrict__ weight, int64_t ignore_index, float4* tile, double& s_nll,
                                              double& s_w) {
  constexpr int C = 4 * Q;
  for (int64_t base = (int64_t)blockIdx.x * kST; base < R; base += (int64_t)gridDim.x * kST) {
    const int64_t r = base + threadIdx.x;
    const int64_t y = r < R ? label[r] : -1;
    float x[C], mx;
    seg_load_rows<Q>(logit, base + (threadIdx.x & ~(kWave - 1)), R, tile, x);
    if (r >= R || y == ignore_index || y < 0 || y >= C) continue;
    const float lse = regs_lse<Q>(x, &mx);
    float xy = x[0];  // x[y] from the registers: a compare-select chain, not a second global load that waits for the label
#pragma unroll
    for (int c = 1; c < C; ++c) xy = c == (int)y ? x[c] : xy;
    const float nll = (mx + lse) - xy;
    const float w = weight ? weight[y] : 1.f;
    s_nll += (double)(w * nll);
    s_w += (double)w;
  }
}

// One workgroup's 256 gradient rows on this layout (logits and gradient both).
template <int Q>
__device__ __forceinline__ void seg_loss_bwd_rows(const float* __restrict__ logit, int64_t R, const int64_t* __restrict__ label,
                                                  const float* __restrict__ weight, int64_t ignore_index, const double* __restrict__ acc,
                                                  const float* __restrict__ grad_out, float* __restrict__ grad, float4* tile) {
  constexpr int C = 4 * Q;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row0 = (int64_t)blockIdx.x * kST + (threadIdx.x & ~(kWave - 1)), r = row0 + lane;
  const int64_t y = r < R ? label[r] : -1;
  const bool valid = r < R && y != ignore_index && y >= 0 && y < C;
  float x[C], mx;
  seg_load_rows<Q>(logit, row0, R, tile, x);
  const float lse = regs_lse<Q>(x, &mx);
  const float scale = valid ? (float)((double)(*grad_out) * (double)(weight ? weight[y] : 1.f) / acc[1]) : 0.f;
  __syncthreads();  // every lane has its row: the tile takes the gradient rows
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    float gv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 4 * q + i;
      gv[i] = valid ? scale * (expf((x[c] - mx) - lse) - (c == (int)y ? 1.f : 0.f)) : 0.f;  // exact zeros for ignored points
    }
    tile[lane * Q + q] = make_float4(gv[0], gv[1], gv[2], gv[3]);
  }
  __syncthreads();
  const int64_t q0 = row0 * Q, nq = R * Q;
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const int64_t k = q0 + lane + i * kWave;
    if (k < nq) *reinterpret_cast<float4*>(grad + 4 * k) = tile[lane + i * kWave];
  }
}

// the eight widths of the layout (C = 4 .. 32): exact trip counts, no guard per class
#define SEG_ROWS_DISPATCH(C, CALL)  \
  switch ((C) >> 2) {               \
    case 1: CALL(1); break;         \
    case 2: CALL(2); break;         \
    case 3: CALL(3); break;         \
    case 4: CALL(4); break;         \
    case 5: CALL(5); break;         \
    case 6: CALL(6); break;         \
    case 7: CALL(7); break;         \
    default: CALL(8); break;        \
  }

// acc[0] += sum w[y] * nll, acc[1] += sum w[y] over the valid points; the LAST workgroup (ticket in acc[2], as an
// unsigned 64-bit counter) writes loss = acc[0] / acc[1] -- no separate division launch.
__global__ __launch_bounds__(kST) void seg_loss_kernel(const float* __restrict__ logit, int64_t B, int C, int64_t N, int64_t ld_b,
                                                       int64_t ld_c, int64_t ld_n, const int64_t* __restrict__ label,
                                                       const float* __restrict__ weight, int64_t ignore_index,
                                                       double* __restrict__ acc, float* __restrict__ loss) {
  __shared__ double red[kST / kWave];
  __shared__ SegTile tile[kST / kWave];
  const int64_t R = B * N;
  double s_nll = 0.0, s_w = 0.0;
  if (seg_rows_layout(logit, B, C, N, ld_b, ld_c, ld_n)) {
#define SEG_CALL(Q) seg_loss_rows<Q>(logit, R, label, weight, ignore_index, tile[threadIdx.x >> 6], s_nll, s_w)
    SEG_ROWS_DISPATCH(C, SEG_CALL)
#undef SEG_CALL
  } else  // any other layout: one row per lane at its strides
  for (int64_t r = (int64_t)blockIdx.x * kST + threadIdx.x; r < R; r += (int64_t)gridDim.x * kST) {
    const int64_t y = label[r];
    if (y == ignore_index || y < 0 || y >= C) continue;
    const int64_t b = r / N, n = r - b * N;
    const float* p = logit + b * ld_b + n * ld_n;
    float mx, x[kRegC];
    const float lse = row_lse(p, ld_c, C, &mx, x);
    const float nll = (mx + lse) - p[y * ld_c];
    const float w = weight ? weight[y] : 1.f;
    s_nll += (double)(w * nll);
    s_w += (double)w;
  }
  const double t0 = block_sum(s_nll, red);
  const double t1 = block_sum(s_w, red);
  if (threadIdx.x == 0) {
    atomicAdd(acc + 0, t0);
    atomicAdd(acc + 1, t1);
    // the two device-scope atomics must be complete (performed at the memory side) before the ticket is drawn: a completion wait
    // (common.h), not a device-scope fence (that would write back and invalidate the XCD's L2 once per workgroup)
    wait_vm_complete();
    const unsigned long long ticket = atomicAdd(reinterpret_cast<unsigned long long*>(acc + 2), 1ull);
    if (ticket == (unsigned long long)gridDim.x - 1) {
      const double a0 = atomicAdd(acc + 0, 0.0), a1 = atomicAdd(acc + 1, 0.0);
      *loss = (float)(a0 / a1);  // no valid point: 0/0 = nan, as torch
    }
  }
}

// grad (same addressing with its own strides) = g * w[y] / W * (softmax(x) - onehot(y)); 0 for ignored points
__global__ __launch_bounds__(kST) void seg_loss_bwd_kernel(const float* __restrict__ logit, int64_t B, int C, int64_t N, int64_t ld_b,
                                                           int64_t ld_c, int64_t ld_n, const int64_t* __restrict__ label,
                                                           const float* __restrict__ weight, int64_t ignore_index,
                                                           const double* __restrict__ acc, const float* __restrict__ grad_out,
                                                           float* __restrict__ grad, int64_t gld_b, int64_t gld_c, int64_t gld_n) {
  __shared__ SegTile tile[kST / kWave];
  const int64_t R = B * N;
  const int64_t r = (int64_t)blockIdx.x * kST + threadIdx.x;
  if (seg_rows_layout(logit, B, C, N, ld_b, ld_c, ld_n) && seg_rows_layout(grad, B, C, N, gld_b, gld_c, gld_n)) {
#define SEG_CALL(Q) seg_loss_bwd_rows<Q>(logit, R, label, weight, ignore_index, acc, grad_out, grad, tile[threadIdx.x >> 6])
    SEG_ROWS_DISPATCH(C, SEG_CALL)
#undef SEG_CALL
    return;
  }
  if (r >= R) return;
  const int64_t b = r / N, n = r - b * N;
  float* g = grad + b * gld_b + n * gld_n;
  const int64_t y = label[r];
  const bool gvec = gld_c == 1 && (C & 3) == 0 && C <= kRegC && (reinterpret_cast<uintptr_t>(g) & 15) == 0;  // rows layout: 16-byte stores
  if (y == ignore_index || y < 0 || y >= C) {
    if (gvec)
      for (int q = 0; q < C / 4; ++q) *reinterpret_cast<float4*>(g + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
    else
      for (int c = 0; c < C; ++c) g[(int64_t)c * gld_c] = 0.f;
    return;
  }
  const float* p = logit + b * ld_b + n * ld_n;
  float mx, x[kRegC];
  const float lse = row_lse(p, ld_c, C, &mx, x);
  const float scale = (float)((double)(*grad_out) * (double)(weight ? weight[y] : 1.f) / acc[1]);
  if (C <= kRegC) {
    float gv[kRegC];
#pragma unroll
    for (int c = 0; c < kRegC; ++c) gv[c] = c < C ? scale * (expf((x[c] - mx) - lse) - (c == y ? 1.f : 0.f)) : 0.f;
    if (gvec) {
#pragma unroll
      for (int q = 0; q < kRegC / 4; ++q)
        if (4 * q < C) *reinterpret_cast<float4*>(g + 4 * q) = make_float4(gv[4 * q], gv[4 * q + 1], gv[4 * q + 2], gv[4 * q + 3]);
    } else {
#pragma unroll
      for (int c = 0; c < kRegC; ++c)
        if (c < C) g[(int64_t)c * gld_c] = gv[c];
    }
  } else {
    for (int c = 0; c < C; ++c) {
      const float sm = expf((p[(int64_t)c * ld_c] - mx) - lse);
      g[(int64_t)c * gld_c] = scale * (sm - (c == y ? 1.f : 0.f));
    }
  }
}

// mat[label][argmax] += 1 over the valid points (first maximum wins, as torch.argmax); workgroup-private histogram in LDS
constexpr int kMaxHist = 4096;  // C <= 64
__global__ __launch_bounds__(kST) void seg_confusion_kernel(const float* __restrict__ logit, int64_t B, int C, int64_t N, int64_t ld_b,
                                                            int64_t ld_c, int64_t ld_n, const int64_t* __restrict__ label,
                                                            int64_t ignore_index, unsigned long long* __restrict__ mat) {
  __shared__ unsigned int hist[kMaxHist];
  const bool lds = C * C <= kMaxHist;
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += kST) hist[i] = 0u;
  __syncthreads();
  const int64_t R = B * N;
  for (int64_t r = (int64_t)blockIdx.x * kST + threadIdx.x; r < R; r += (int64_t)gridDim.x * kST) {
    const int64_t y = label[r];
    if (y == ignore_index || y < 0 || y >= C) continue;
    const int64_t b = r / N, n = r - b * N;
    const float* p = logit + b * ld_b + n * ld_n;
    float mx;
    int am = 0;
    if (C <= kRegC) {
      float x[kRegC];
#pragma unroll
      for (int c = 0; c < kRegC; ++c) x[c] = p[(int64_t)min(c, C - 1) * ld_c];
      mx = x[0];
#pragma unroll
      for (int c = 1; c < kRegC; ++c)
        if (c < C && x[c] > mx) {
          mx = x[c];
          am = c;
        }
    } else {
      mx = p[0];
      for (int c = 1; c < C; ++c) {
        const float v = p[(int64_t)c * ld_c];
        if (v > mx) {
          mx = v;
          am = c;
        }
      }
    }
    if (lds)
      atomicAdd(&hist[(int)y * C + am], 1u);
    else
      atomicAdd(mat + y * C + am, 1ull);
  }
  __syncthreads();
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += kST)
      if (hist[i]) atomicAdd(mat + i, (unsigned long long)hist[i]);
}

// ---- loss + the meters of a training iteration in one launch (mvp_seg_loss_meter_f32) -------------------------------------------------
// seg_loss_kernel with the argmax and the confusion count taken from the row it already holds, and the meter state (include/mvp_hip.h)
// updated by the launch's last workgroup.  The loss half KEEPS seg_loss_kernel's row arithmetic (row_lse / regs_lse on the same values)
// and its workgroup partition (same grid, same rows per lane in the same order), so acc[0], acc[1] are fp64 sums of the same workgroup
// partials and the loss is the same float32 to within one ulp (tests/test_meters_gpu.py derives the bound from exactly this).
struct SegMeter {
  unsigned int* hist;        // the workgroup's (C,C) counts in LDS, or nullptr: straight to mat
  unsigned long long* mat;
  int C;
  unsigned int ok = 0u, valid = 0u;  // this lane's rows (at most R / 256 < 2^32)
  __device__ __forceinline__ void count(int y, int am) {
    if (hist)
      atomicAdd(&hist[y * C + am], 1u);
    else
      atomicAdd(mat + (int64_t)y * C + am, 1ull);
    valid += 1u;
    ok += am == y ? 1u : 0u;
  }
};

// first maximum of x[0 .. C): strict `>` from class 0, as seg_confusion_kernel and torch.argmax
template <int CMAX>
__device__ __forceinline__ int regs_argmax(const float* x, int C) {
  float mx = x[0];
  int am = 0;
#pragma unroll
  for (int c = 1; c < CMAX; ++c)
    if (c < C && x[c] > mx) {
      mx = x[c];
      am = c;
    }
  return am;
}

template <int Q>
__device__ __forceinline__ void seg_loss_meter_rows(const float* __restrict__ logit, int64_t R, const int64_t* __restrict__ label,
                                                    const float* __restrict__ weight, int64_t ignore_index, bool want_loss, float4* tile,
                                                    double& s_nll, double& s_w, SegMeter& meter) {
  constexpr int C = 4 * Q;
  for (int64_t base = (int64_t)blockIdx.x * kST; base < R; base += (int64_t)gridDim.x * kST) {
    const int64_t r = base + threadIdx.x;
    const int64_t y = r < R ? label[r] : -1;
    float x[C], mx;
    seg_load_rows<Q>(logit, base + (threadIdx.x & ~(kWave - 1)), R, tile, x);
    if (r >= R || y == ignore_index || y < 0 || y >= C) continue;
    meter.count((int)y, regs_argmax<C>(x, C));
    if (!want_loss) continue;
    const float lse = regs_lse<Q>(x, &mx);
    float xy = x[0];
#pragma unroll
    for (int c = 1; c < C; ++c) xy = c == (int)y ? x[c] : xy;
    const float nll = (mx + lse) - xy;
    const float w = weight ? weight[y] : 1.f;
    s_nll += (double)(w * nll);
    s_w += (double)w;
  }
}

__global__ __launch_bounds__(kST) void seg_loss_meter_kernel(const float* __restrict__ logit, int64_t B, int C, int64_t N, int64_t ld_b,
                                                             int64_t ld_c, int64_t ld_n, const int64_t* __restrict__ label,
                                                             const float* __restrict__ weight, int64_t ignore_index, double* __restrict__ acc,
                                                             float* __restrict__ loss, unsigned long long* __restrict__ mi,
                                                             double* __restrict__ mf, int W) {
  __shared__ double red[kST / kWave];
  __shared__ SegTile tile[kST / kWave];
  __shared__ unsigned int hist[kMaxHist];
  __shared__ unsigned long long wg_count[2];
  const int64_t R = B * N;
  const bool want_loss = acc != nullptr;
  // workgroup-private histogram as in seg_confusion_kernel; below 2^32 rows no 32-bit bin can wrap
  const bool lds = C * C <= kMaxHist && R < (1ll << 32);
  unsigned long long* mat = mi + 4 + 2 * (W + 1);
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += kST) hist[i] = 0u;
  if (threadIdx.x < 2) wg_count[threadIdx.x] = 0ull;
  __syncthreads();
  SegMeter meter{lds ? hist : nullptr, mat, C};
  double s_nll = 0.0, s_w = 0.0;
  if (seg_rows_layout(logit, B, C, N, ld_b, ld_c, ld_n)) {
#define SEG_CALL(Q) seg_loss_meter_rows<Q>(logit, R, label, weight, ignore_index, want_loss, tile[threadIdx.x >> 6], s_nll, s_w, meter)
    SEG_ROWS_DISPATCH(C, SEG_CALL)
#undef SEG_CALL
  } else  // any other layout: one row per lane at its strides
  for (int64_t r = (int64_t)blockIdx.x * kST + threadIdx.x; r < R; r += (int64_t)gridDim.x * kST) {
    const int64_t y = label[r];
    if (y == ignore_index || y < 0 || y >= C) continue;
    const int64_t b = r / N, n = r - b * N;
    const float* p = logit + b * ld_b + n * ld_n;
    float mx, x[kRegC];
    if (C <= kRegC) {
      const float lse = row_lse(p, ld_c, C, &mx, x);  // (the meters-only form pays for the exponentials here: it is not the hot layout)
      meter.count((int)y, regs_argmax<kRegC>(x, C));
      if (!want_loss) continue;
      const float nll = (mx + lse) - p[y * ld_c];
      const float w = weight ? weight[y] : 1.f;
      s_nll += (double)(w * nll);
      s_w += (double)w;
    } else {
      float top = p[0];
      int am = 0;
      for (int c = 1; c < C; ++c) {
        const float v = p[(int64_t)c * ld_c];
        if (v > top) {
          top = v;
          am = c;
        }
      }
      meter.count((int)y, am);
      if (!want_loss) continue;
      const float lse = row_lse(p, ld_c, C, &mx, x);
      const float nll = (mx + lse) - p[y * ld_c];
      const float w = weight ? weight[y] : 1.f;
      s_nll += (double)(w * nll);
      s_w += (double)w;
    }
  }
  // the lanes' counts: one LDS atomic per wave, one pair of global atomics per workgroup
  unsigned int ok = meter.ok, valid = meter.valid;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    ok += __shfl_xor(ok, m, kWave);
    valid += __shfl_xor(valid, m, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    atomicAdd(&wg_count[0], (unsigned long long)ok);
    atomicAdd(&wg_count[1], (unsigned long long)valid);
  }
  const double t0 = block_sum(s_nll, red);  // (its barriers also close the histogram and the two counts)
  const double t1 = block_sum(s_w, red);
  // The histogram goes out through waves 1 .. 3: up to 256 workgroups add to the same C * C words, those adds queue, and wave 0's
  // completion wait below must not stand in that queue (nothing in this launch reads the matrix: the kernel's end publishes it).
  if (lds && threadIdx.x >= kWave)
    for (int i = threadIdx.x - kWave; i < C * C; i += kST - kWave)
      if (hist[i]) atomicAdd(mat + i, (unsigned long long)hist[i]);
  if (threadIdx.x == 0) {
    if (want_loss) {
      atomicAdd(acc + 0, t0);
      atomicAdd(acc + 1, t1);
    }
    atomicAdd(mi + 1, wg_count[0]);
    atomicAdd(mi + 2, wg_count[1]);
    // as in seg_loss_kernel: this lane's device-scope atomics are complete before the ticket is drawn -- a completion wait, not a fence
    wait_vm_complete();
    const unsigned long long ticket = atomicAdd(mi + 3, 1ull);
    if (ticket == (unsigned long long)gridDim.x - 1) {
      // every workgroup's sums and counts have landed.  Nothing else touches the cursor, the rings or the ticket during the launch.
      // The words the adds went to are read with device-scope atomic LOADS (coherent at device scope like the adds; the compiler
      // itself turns an integer `atomicAdd(p, 0)` into one): read-modify-write atomics are bracketed and waited for one by one, a trip
      // to the memory side each (measured: +3.9 us for five of them on a 17 us launch), the loads are in flight together.
      double a0 = 0.0, a1 = 0.0;
      if (want_loss) {
        a0 = __hip_atomic_load(acc + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a1 = __hip_atomic_load(acc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const unsigned long long c = __hip_atomic_load(mi + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long v = __hip_atomic_load(mi + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long u = __hip_atomic_load(mi + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull;
      const double sum = __hip_atomic_load(mf + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      float l = __builtin_nanf("");
      if (want_loss) {
        l = (float)(a0 / a1);  // no valid point: 0/0 = nan, as torch
        *loss = l;
        reinterpret_cast<unsigned long long*>(acc)[2] = (unsigned long long)gridDim.x;  // what seg_loss_kernel's ticket ends at
      }
      unsigned long long* snap = mi + 4 + 2 * (u % (unsigned long long)(W + 1));
      snap[0] = c;
      snap[1] = v;
      mf[1 + u % (unsigned long long)W] = (double)l;
      mf[0] = sum + (double)l;
      __hip_atomic_store(mi + 0, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(mi + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the ticket resets itself: no zero fill per call
    }
  }
}

int check_seg(const float* logit, int64_t B, int64_t C, int64_t N, const int64_t* label) {
  MVP_NONNULL(logit);
  MVP_NONNULL(label);
  MVP_REQUIRE(B >= 0 && N >= 0 && C >= 1 && C < (1 << 16) && B * N < (1ll << 40));
  return MVP_OK;
}

}  // namespace

MVP_API int mvp_seg_loss_f32(const float* logit, int64_t B, int64_t C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n,
                             const int64_t* label, const float* weight, int64_t ignore_index, double* acc, float* loss,
                             mvp_stream_t stream) {
  int rc = check_seg(logit, B, C, N, label);
  if (rc) return rc;
  MVP_NONNULL(acc);
  MVP_NONNULL(loss);
  const int64_t R = B * N;
  // at most 256 workgroups: each ends in three fp64 atomics on ONE cache line (sums + ticket), which queue (262144 points: 23.7 us with
  // 256, 28.7 with 512, 45.5 with 1024, 24.5 with 128 workgroups -- tools/exp/seg_loss_time.py)
  const unsigned blocks = (unsigned)std::min<int64_t>(256, std::max<int64_t>(1, cdiv(R, kST)));
  hipLaunchKernelGGL(seg_loss_kernel, dim3(blocks), dim3(kST), 0, static_cast<hipStream_t>(stream), logit, B, (int)C, N, ld_b, ld_c, ld_n,
                     label, weight, ignore_index, acc, loss);
  return mvp_launch_status();
}

MVP_API int mvp_seg_loss_meter_f32(const float* logit, int64_t B, int64_t C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n,
                                   const int64_t* label, const float* weight, int64_t ignore_index, double* acc, float* loss,
                                   int64_t* meter_i64, double* meter_f64, int64_t window, mvp_stream_t stream) {
  MVP_NONNULL(logit);  // every null ahead of any other error
  MVP_NONNULL(label);
  MVP_NONNULL(meter_i64);
  MVP_NONNULL(meter_f64);
  if ((acc == nullptr) != (loss == nullptr)) return MVP_ENULL;  // both: the loss as well; neither: the meters only
  int rc = check_seg(logit, B, C, N, label);
  if (rc) return rc;
  MVP_REQUIRE(window >= 1 && window <= MVP_SEG_METER_MAX_WINDOW);
  const int64_t R = B * N;
  // mvp_seg_loss_f32's grid, for the reason written there (here five atomics per workgroup on two cache lines) -- and because the loss
  // must be summed over the same workgroup partials
  const unsigned blocks = (unsigned)std::min<int64_t>(256, std::max<int64_t>(1, cdiv(R, kST)));
  hipLaunchKernelGGL(seg_loss_meter_kernel, dim3(blocks), dim3(kST), 0, static_cast<hipStream_t>(stream), logit, B, (int)C, N, ld_b, ld_c,
                     ld_n, label, weight, ignore_index, acc, loss, reinterpret_cast<unsigned long long*>(meter_i64), meter_f64, (int)window);
  return mvp_launch_status();
}

MVP_API int mvp_seg_loss_backward_f32(const float* logit, int64_t B, int64_t C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n,
                                      const int64_t* label, const float* weight, int64_t ignore_index, const double* acc,
                                      const float* grad_out, float* grad_logit, int64_t gld_b, int64_t gld_c, int64_t gld_n,
                                      mvp_stream_t stream) {
  int rc = check_seg(logit, B, C, N, label);
  if (rc) return rc;
  MVP_NONNULL(acc);
  MVP_NONNULL(grad_out);
  MVP_NONNULL(grad_logit);
  const int64_t R = B * N;
  if (R == 0) return MVP_OK;
  hipLaunchKernelGGL(seg_loss_bwd_kernel, dim3((unsigned)cdiv(R, kST)), dim3(kST), 0, static_cast<hipStream_t>(stream), logit, B, (int)C, N,
                     ld_b, ld_c, ld_n, label, weight, ignore_index, acc, grad_out, grad_logit, gld_b, gld_c, gld_n);
  return mvp_launch_status();
}

MVP_API int mvp_seg_confusion_f32(const float* logit, int64_t B, int64_t C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n,
                                  const int64_t* label, int64_t ignore_index, int64_t* mat, mvp_stream_t stream) {
  int rc = check_seg(logit, B, C, N, label);
  if (rc) return rc;
  MVP_NONNULL(mat);
  const int64_t R = B * N;
  if (R == 0) return MVP_OK;
  const unsigned blocks = (unsigned)std::min<int64_t>(256, cdiv(R, kST));
  hipLaunchKernelGGL(seg_confusion_kernel, dim3(blocks), dim3(kST), 0, static_cast<hipStream_t>(stream), logit, B, (int)C, N, ld_b, ld_c,
                     ld_n, label, ignore_index, reinterpret_cast<unsigned long long*>(mat));
  return mvp_launch_status();
}

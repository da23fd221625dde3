// solver.hip -- the end of a stage-one training iteration for gfx950: SGD with momentum over ALL parameter tensors in one launch, and the
// global gradient-norm clip in two.
//
// The reference's 2D stage trains with torch.optim.SGD (common/solver/build.py:7-22 from configs/scannet/unet_resnet34.yaml: momentum 0.9,
// weight decay 1e-4) and clips with nn.utils.clip_grad_norm_ (train_2d.py:181-185).  torch's foreach SGD walks the parameter tensors in
// one multi_tensor_apply pass per operation (weight decay, momentum multiply, add, parameter update), each split into several launches,
// and the clip is a per-tensor norm pass, a stack, a norm, a clamp and a foreach multiply.  Here, as in adam.hip, the pointer lists and a
// block-prefix table travel in the kernel-argument block, a workgroup finds its tensor by a binary search on uniform values and every lane
// moves 16-byte vectors where a tensor's pointers allow it:
//   sgd_multi_kernel      p, g, momentum buffer read once and p, buffer written once per step (20 B per element; 12 B without momentum);
//   sqnorm_partials       one fp32 sum of squares per workgroup of 8192 gradient elements, written to its own slot -- no atomics;
//   clip_finish           EVERY workgroup adds all partials in the same fixed order (so all hold the same bits), forms the total norm and
//                         the clip coefficient and scales its own 8192 elements; no host synchronisation, bit-reproducible.
// The coefficient can instead stay on the device and be applied by the SGD kernel as it reads the gradient (grad_scale): the gradients
// are then read twice and never rewritten.
#include "common.h"
#include <math.h>

namespace {

constexpr int kSgdMax = 124;        // tensors per launch
constexpr int kSgdThreads = 256;
constexpr int kSgdPerBlock = 2048;  // elements per workgroup: two 16-byte vectors per lane

struct SgdArgs {
  float* p[kSgdMax];
  const float* g[kSgdMax];
  float* b[kSgdMax];                       // momentum buffers (unused when momentum == 0)
  int first_block[kSgdMax + 1];            // prefix over the tensors' workgroup counts
  int numel[kSgdMax];                      // < 2^31 each (host check)
  unsigned vec_mask[(kSgdMax + 31) / 32];    // bit i: the pointers of tensor i are 16-byte aligned
  unsigned first_mask[(kSgdMax + 31) / 32];  // bit i: tensor i takes its first momentum step (buffer = gradient, never read)
  const float* grad_scale;                 // null, or one float on the device: the gradient is multiplied by it as it is read
  int n;
  int use_momentum, nesterov;
  float lr, momentum, one_minus_dampening, weight_decay;  // 1 - dampening evaluated in double
};
static_assert(sizeof(SgdArgs) <= 4096, "kernel-argument block");

// torch.optim.SGD per element.  The library is built with -ffp-contract=off, so what fuses is written out: every `x + alpha y` of the rule
// (ATen's add(x, y, alpha)) is ONE fused multiply-add -- four roundings per element and step (weight decay, momentum multiply, momentum
// add, update) instead of six.  ATen's kernels appear to round the same way (its momentum buffers were observed bit-equal to these; its
// code objects were not read).  The deferred clip coefficient is a rounded product of its own: the gradient clip_grad_norm_ would have stored.
__device__ __forceinline__ void sgd_one(float& p, float g, float& b, const SgdArgs& a, bool scaled, float scale, bool first) {
  if (scaled) g = g * scale;
  if (a.weight_decay != 0.f) g = __fmaf_rn(a.weight_decay, p, g);
  if (a.use_momentum) {
    b = first ? g : __fmaf_rn(a.one_minus_dampening, g, a.momentum * b);
    g = a.nesterov ? __fmaf_rn(a.momentum, b, g) : b;
  }
  p = __fmaf_rn(-a.lr, g, p);
}

__global__ __launch_bounds__(kSgdThreads) void sgd_multi_kernel(const SgdArgs a) {
  // tensor of this workgroup: the last i with first_block[i] <= blockIdx.x (uniform: scalar loads from the argument block)
  int lo = 0, hi = a.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const int t = lo;
  const int base = ((int)blockIdx.x - a.first_block[t]) * kSgdPerBlock;
  const int n = a.numel[t];
  float* __restrict__ p = a.p[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ b = a.b[t];
  const bool vec = (a.vec_mask[t >> 5] >> (t & 31)) & 1u;
  const bool first = (a.first_mask[t >> 5] >> (t & 31)) & 1u;
  const bool mom = a.use_momentum != 0;
  const bool load_b = mom && !first;
  const bool scaled = a.grad_scale != nullptr;
  const float scale = scaled ? *a.grad_scale : 1.f;
  if (vec) {
#pragma unroll
    for (int u = 0; u < kSgdPerBlock / (4 * kSgdThreads); ++u) {
      const int e = base + (u * kSgdThreads + (int)threadIdx.x) * 4;
      if (e + 3 < n) {
        float4 pv = *reinterpret_cast<const float4*>(p + e);
        const float4 gv = *reinterpret_cast<const float4*>(g + e);
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (load_b) bv = *reinterpret_cast<const float4*>(b + e);
        sgd_one(pv.x, gv.x, bv.x, a, scaled, scale, first);
        sgd_one(pv.y, gv.y, bv.y, a, scaled, scale, first);
        sgd_one(pv.z, gv.z, bv.z, a, scaled, scale, first);
        sgd_one(pv.w, gv.w, bv.w, a, scaled, scale, first);
        *reinterpret_cast<float4*>(p + e) = pv;
        if (mom) *reinterpret_cast<float4*>(b + e) = bv;
      } else {
        for (int i = e; i < n; ++i) {  // the tensor's last 1..3 elements
          float pv = p[i], bv = load_b ? b[i] : 0.f;
          sgd_one(pv, g[i], bv, a, scaled, scale, first);
          p[i] = pv;
          if (mom) b[i] = bv;
        }
      }
    }
    return;
  }
  for (int i = base + (int)threadIdx.x; i < min(n, base + kSgdPerBlock); i += kSgdThreads) {
    float pv = p[i], bv = load_b ? b[i] : 0.f;
    sgd_one(pv, g[i], bv, a, scaled, scale, first);
    p[i] = pv;
    if (mom) b[i] = bv;
  }
}

constexpr int kNormMax = 240;         // tensors per launch
constexpr int kNormThreads = 256;
constexpr int kNormPerBlock = 8192;   // elements per workgroup: eight 16-byte vectors per lane
constexpr int kNormVecs = kNormPerBlock / (4 * kNormThreads);

struct GradTable {
  float* g[kNormMax];
  int first_block[kNormMax + 1];  // prefix over the tensors' workgroup counts (within this launch)
  int numel[kNormMax];
  unsigned vec_mask[(kNormMax + 31) / 32];  // bit i: tensor i is 16-byte aligned
  int n;
};
static_assert(sizeof(GradTable) + 64 <= 4096, "kernel-argument block");

// Sum over the workgroup, the same bits in every lane: xor butterflies inside a wave (both partners add the same two values), then the
// four wave sums in a fixed order.  log2(256) = 8 levels.
__device__ __forceinline__ float block_sum_all(float v, float* lds) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, kWave);
  __syncthreads();  // (an earlier use of lds is over)
  if (((int)threadIdx.x & (kWave - 1)) == 0) lds[(int)threadIdx.x / kWave] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
static_assert(kNormThreads == 4 * kWave, "block_sum_all adds four wave sums");

__device__ __forceinline__ int tensor_of_block(const GradTable& t, int block) {
  int lo = 0, hi = t.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.first_block[mid] <= block) lo = mid; else hi = mid;
  }
  return lo;
}

// Lane l owns elements base + (u * 256 + l) * 4 + {0,1,2,3}, u = 0..7, whether the tensor is aligned or not: the order of the additions
// -- and so the bits of the sum -- does not depend on where the allocator put the gradient.
__global__ __launch_bounds__(kNormThreads) void sqnorm_partials_kernel(const GradTable t, float* __restrict__ partials) {
  __shared__ float lds[kNormThreads / kWave];
  const int ti = tensor_of_block(t, (int)blockIdx.x);
  const int base = ((int)blockIdx.x - t.first_block[ti]) * kNormPerBlock;
  const int n = t.numel[ti];
  const float* __restrict__ g = t.g[ti];
  const bool vec = (t.vec_mask[ti >> 5] >> (ti & 31)) & 1u;
  float acc = 0.f;
  if (vec && base + kNormPerBlock <= n) {  // a full block: all eight loads in flight at once
    float4 x[kNormVecs];
#pragma unroll
    for (int u = 0; u < kNormVecs; ++u) x[u] = *reinterpret_cast<const float4*>(g + base + (u * kNormThreads + (int)threadIdx.x) * 4);
#pragma unroll
    for (int u = 0; u < kNormVecs; ++u) {
      acc = acc + x[u].x * x[u].x;
      acc = acc + x[u].y * x[u].y;
      acc = acc + x[u].z * x[u].z;
      acc = acc + x[u].w * x[u].w;
    }
  } else {
#pragma unroll
    for (int u = 0; u < kNormVecs; ++u) {
      const int e = base + (u * kNormThreads + (int)threadIdx.x) * 4;
      if (vec && e + 3 < n) {
        const float4 x = *reinterpret_cast<const float4*>(g + e);
        acc = acc + x.x * x.x;
        acc = acc + x.y * x.y;
        acc = acc + x.z * x.z;
        acc = acc + x.w * x.w;
      } else {
        for (int i = e; i < min(n, e + 4); ++i) {
          const float x = g[i];
          acc = acc + x * x;
        }
      }
    }
  }
  const float s = block_sum_all(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kNormThreads) void clip_finish_kernel(const GradTable t, const float* __restrict__ partials, int n_partials,
                                                                   float max_norm, int scale_grads, int write_scalars,
                                                                   float* __restrict__ total_norm_out, float* __restrict__ coef_out) {
  __shared__ float lds[kNormThreads / kWave];
  float acc = 0.f;
  for (int i = (int)threadIdx.x; i < n_partials; i += kNormThreads) acc = acc + partials[i];
  const float total = __fsqrt_rn(block_sum_all(acc, lds));
  // torch.clamp(max_norm / (total + 1e-6), max=1.0): a NaN stays a NaN (fminf would drop it).  max_norm < 0: no clipping.
  const float c = max_norm / (total + 1e-6f);
  const float coef = max_norm < 0.f ? 1.f : (c < 1.f ? c : (c != c ? c : 1.f));
  if (write_scalars && blockIdx.x == 0 && threadIdx.x == 0) {
    *total_norm_out = total;
    *coef_out = coef;
  }
  if (!scale_grads) return;
  const int ti = tensor_of_block(t, (int)blockIdx.x);
  const int base = ((int)blockIdx.x - t.first_block[ti]) * kNormPerBlock;
  const int n = t.numel[ti];
  float* __restrict__ g = t.g[ti];
  const bool vec = (t.vec_mask[ti >> 5] >> (ti & 31)) & 1u;
  if (vec) {
#pragma unroll
    for (int u = 0; u < kNormVecs; ++u) {
      const int e = base + (u * kNormThreads + (int)threadIdx.x) * 4;
      if (e + 3 < n) {
        float4 x = *reinterpret_cast<const float4*>(g + e);
        x.x = x.x * coef; x.y = x.y * coef; x.z = x.z * coef; x.w = x.w * coef;
        *reinterpret_cast<float4*>(g + e) = x;
      } else {
        for (int i = e; i < n; ++i) g[i] = g[i] * coef;  // the tensor's last 1..3 elements
      }
    }
    return;
  }
  for (int i = base + (int)threadIdx.x; i < min(n, base + kNormPerBlock); i += kNormThreads) g[i] = g[i] * coef;
}

// Fills the table with tensors [i0, i0 + kNormMax) that have elements; returns the launch's workgroup count, or a negative MVP_E*.
int fill_grad_table(GradTable& t, void* const* grads, const int64_t* numel, int64_t n, int64_t i0) {
  t.n = 0;
  for (unsigned& w : t.vec_mask) w = 0u;
  int64_t blocks = 0;
  for (int64_t i = i0; i < n && i < i0 + kNormMax; ++i) {
    if (numel[i] < 0 || numel[i] >= (1ll << 31) - kNormPerBlock) return MVP_EINVAL;
    if (numel[i] == 0) continue;
    if (grads[i] == nullptr) return MVP_ENULL;
    const int k = t.n++;
    t.g[k] = static_cast<float*>(grads[i]);
    t.numel[k] = (int)numel[i];
    t.first_block[k] = (int)blocks;
    blocks += cdiv(numel[i], kNormPerBlock);
    if (blocks >= (1ll << 31)) return MVP_EINVAL;
    if (((uintptr_t)grads[i] & 15) == 0) t.vec_mask[k >> 5] |= 1u << (k & 31);
  }
  t.first_block[t.n] = (int)blocks;
  return (int)blocks;
}

}  // namespace

// One torch.optim.SGD step of n float32 tensors (see include/mvp_hip.h).  Tensors are processed 124 per launch.
MVP_API int mvp_sgd_step_f32(void* const* params, const void* const* grads, void* const* momentum_buf, const int64_t* numel,
                             const uint8_t* first, int64_t n, double lr, double momentum, double dampening, double weight_decay,
                             int nesterov, const float* grad_scale, mvp_stream_t stream) {
  MVP_REQUIRE(n >= 0 && momentum >= 0.0 && lr >= 0.0);
  MVP_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0));
  if (n == 0) return MVP_OK;
  MVP_NONNULL(params);
  MVP_NONNULL(grads);
  MVP_NONNULL(numel);
  const bool mom = momentum != 0.0;
  if (mom) {
    MVP_NONNULL(momentum_buf);
    MVP_NONNULL(first);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  bool launched = false;
  for (int64_t i0 = 0; i0 < n; i0 += kSgdMax) {
    SgdArgs a;
    a.n = 0;
    a.grad_scale = grad_scale;
    a.use_momentum = mom ? 1 : 0;
    a.nesterov = nesterov ? 1 : 0;
    a.lr = (float)lr;
    a.momentum = (float)momentum;
    a.one_minus_dampening = (float)(1.0 - dampening);
    a.weight_decay = (float)weight_decay;
    for (unsigned& w : a.vec_mask) w = 0u;
    for (unsigned& w : a.first_mask) w = 0u;
    int64_t blocks = 0;
    for (int64_t i = i0; i < n && i < i0 + kSgdMax; ++i) {
      MVP_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31) - kSgdPerBlock);
      if (numel[i] == 0) continue;
      MVP_NONNULL(params[i]);
      MVP_NONNULL(grads[i]);
      if (mom) MVP_NONNULL(momentum_buf[i]);
      const int k = a.n++;
      a.p[k] = static_cast<float*>(params[i]);
      a.g[k] = static_cast<const float*>(grads[i]);
      a.b[k] = mom ? static_cast<float*>(momentum_buf[i]) : nullptr;
      a.numel[k] = (int)numel[i];
      a.first_block[k] = (int)blocks;
      blocks += cdiv(numel[i], kSgdPerBlock);
      MVP_REQUIRE(blocks < (1ll << 31));
      const uintptr_t bits = (uintptr_t)params[i] | (uintptr_t)grads[i] | (mom ? (uintptr_t)momentum_buf[i] : (uintptr_t)0);
      if ((bits & 15) == 0) a.vec_mask[k >> 5] |= 1u << (k & 31);
      if (mom && first[i]) a.first_mask[k >> 5] |= 1u << (k & 31);
    }
    if (a.n == 0) continue;
    a.first_block[a.n] = (int)blocks;
    hipLaunchKernelGGL(sgd_multi_kernel, dim3((unsigned)blocks), dim3(kSgdThreads), 0, s, a);
    launched = true;
  }
  return launched ? mvp_launch_status() : MVP_OK;
}

// Number of fp32 partial sums mvp_grad_sqnorm_partials_f32 writes for these tensors (one per 8192 elements of each tensor, rounded up);
// negative MVP_E* on bad arguments.  Host only.
MVP_API int64_t mvp_grad_clip_partials_count(const int64_t* numel, int64_t n) {
  if (n < 0) return MVP_EINVAL;
  if (n == 0) return 0;
  if (numel == nullptr) return MVP_ENULL;
  int64_t total = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (numel[i] < 0 || numel[i] >= (1ll << 31) - kNormPerBlock) return MVP_EINVAL;
    total += cdiv(numel[i], kNormPerBlock);
  }
  return total < (1ll << 31) ? total : (int64_t)MVP_EINVAL;
}

MVP_API int mvp_grad_sqnorm_partials_f32(const void* const* grads, const int64_t* numel, int64_t n, float* partials, int64_t* n_partials_out,
                                         mvp_stream_t stream) {
  const int64_t count = mvp_grad_clip_partials_count(numel, n);
  if (count < 0) return (int)count;
  if (n_partials_out != nullptr) *n_partials_out = count;
  if (count == 0) return MVP_OK;
  MVP_NONNULL(grads);
  MVP_NONNULL(partials);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t done = 0;
  for (int64_t i0 = 0; i0 < n; i0 += kNormMax) {
    GradTable t;
    const int blocks = fill_grad_table(t, const_cast<void* const*>(grads), numel, n, i0);
    if (blocks < 0) return blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(sqnorm_partials_kernel, dim3((unsigned)blocks), dim3(kNormThreads), 0, s, t, partials + done);
    done += blocks;
  }
  return mvp_launch_status();
}

MVP_API int mvp_grad_clip_finish_f32(void* const* grads, const int64_t* numel, int64_t n, const float* partials, int64_t n_partials,
                                     double max_norm, float* total_norm_out, float* coef_out, mvp_stream_t stream) {
  MVP_REQUIRE(n_partials >= 0 && n_partials < (1ll << 31) && !(max_norm != max_norm));
  MVP_NONNULL(total_norm_out);
  MVP_NONNULL(coef_out);
  if (n_partials > 0) MVP_NONNULL(partials);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float mx = max_norm < 0.0 ? -1.f : (float)max_norm;
  int64_t done = 0;
  if (grads != nullptr) {
    MVP_REQUIRE(n >= 0);
    MVP_REQUIRE(mvp_grad_clip_partials_count(numel, n) == n_partials);  // the partials are those of THESE tensors
    for (int64_t i0 = 0; i0 < n; i0 += kNormMax) {
      GradTable t;
      const int blocks = fill_grad_table(t, grads, numel, n, i0);
      if (blocks < 0) return blocks;
      if (blocks == 0) continue;
      hipLaunchKernelGGL(clip_finish_kernel, dim3((unsigned)blocks), dim3(kNormThreads), 0, s, t, partials, (int)n_partials, mx, 1,
                         done == 0 ? 1 : 0, total_norm_out, coef_out);
      done += blocks;
    }
  }
  if (done == 0) {  // no gradient to scale: one workgroup writes the two scalars
    GradTable t;
    t.n = 0;
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(kNormThreads), 0, s, t, partials, (int)n_partials, mx, 0, 1, total_norm_out, coef_out);
  }
  return mvp_launch_status();
}

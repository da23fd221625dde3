// frames.hip -- the picked frames of a raw uint8 store as the 2D network reads them, on the device for gfx950: what a data-loader worker
// does per frame in the reference (mvpnet/data/scannet_2d3d.py:241-252 colour jitter, / 255, normalise; :293-296 flip; the same for 2D
// training, mvpnet/data/scannet_2d.py:158-171).  Definition (pinned, bit-identical to PIL's ImageEnhance chain for given factors and
// order): include/mvp_hip.h, mvp_prepare_frames_u8.
//
//   frames_gray_kernel    : only with a jitter.  The contrast step blends towards the rounded mean grey of the WHOLE image as it enters that
//                           step -- the one dependency across pixels.  Every pixel runs the steps in front of the contrast step, the
//                           workgroup sums its greys (integers: any order gives the same sum) and adds them to the frame's 64-bit word.
//   frames_finish_kernel  : the whole chain per pixel, byte -> float through a 3 x 256 table built per workgroup in LDS (the value depends
//                           on (channel, byte) only: 768 IEEE divisions per workgroup instead of two per value), the flip and the store.
//
// A (tiles, frames) grid of 256-thread workgroups, so every pixel of every picked frame is in flight whatever the frame size.  PX = 4
// (W % 4 == 0, aligned pointers): a lane takes four pixels of one image row at a time -- one 12-byte load, one 16-byte store per channel
// plane (three for channels-last), a mirrored group is reversed in registers.  PX = 1: any width, byte loads and dword stores.  A lane
// takes kFrameGroups such groups, 256 apart: what a workgroup does once -- the table, the mean's 64-bit division, the atomic -- is
// spread over 4096 pixels at PX = 4.  PX = 4 also needs `frames` 4-byte and `out` 16-byte aligned (torch allocations are; a sliced view
// of a store may not be): otherwise the entry takes PX = 1, the same bits at byte loads and dword stores.
// Measurements: DESIGN.md (Frames).
#include "common.h"

namespace {

constexpr int kFrameThreads = 256;
constexpr int kFrameGroups = 4;
constexpr int kMaxGridY = 65535;

typedef float f32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((aligned(4))) U32x3 {
  uint32_t x, y, z;
};

// PIL's convert('L'): ITU-R 601-2 luma in 16.16 fixed point, rounded
__device__ __forceinline__ int gray_u8(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// PIL's ImageChops blend of the degenerate value d and the pixel p: one float32 product, one float32 sum (the library is built with
// -ffp-contract=off), truncation, and the clip that PIL applies outside 0 <= f <= 1 (inside it t already lies in [0, 255]).  A NaN
// factor gives 0: the result always indexes the table.
__device__ __forceinline__ int blend_u8(int d, int p, float f) {
  const float t = (float)d + f * (float)(p - d);
  return t > 0.f ? (t >= 255.f ? 255 : (int)t) : 0;
}

// The jitter of one frame: the order codes and the factor that goes with each step, the same for every lane (scalar registers).
struct Jitter {
  int op0, op1, op2;
  float f0, f1, f2;
  __device__ __forceinline__ bool has_contrast() const { return op0 == 1 || op1 == 1 || op2 == 1; }
};

__device__ __forceinline__ Jitter load_jitter(const float* __restrict__ factor, const uint8_t* __restrict__ order, int f) {
  Jitter j;
  j.op0 = order[(size_t)f * 3 + 0];
  j.op1 = order[(size_t)f * 3 + 1];
  j.op2 = order[(size_t)f * 3 + 2];
  // there is one mean per frame: a second contrast code is no step
  if (j.op1 == 1 && j.op0 == 1) j.op1 = 3;
  if (j.op2 == 1 && (j.op0 == 1 || j.op1 == 1)) j.op2 = 3;
  const float* fac = factor + (size_t)f * 3;  // (brightness, contrast, saturation); a code above 2 is no step, its factor is not used
  j.f0 = fac[j.op0 > 2 ? 2 : j.op0];
  j.f1 = fac[j.op1 > 2 ? 2 : j.op1];
  j.f2 = fac[j.op2 > 2 ? 2 : j.op2];
  return j;
}

// One step on one pixel.  op: 0 brightness (towards black), 1 contrast (towards the mean grey m), 2 saturation (towards the pixel's
// own grey); anything else leaves the pixel alone.
__device__ __forceinline__ void jitter_step(int op, float f, int m, int& r, int& g, int& b) {
  if (op < 0 || op > 2) return;
  const int d = op == 0 ? 0 : (op == 1 ? m : gray_u8(r, g, b));
  r = blend_u8(d, r, f);
  g = blend_u8(d, g, f);
  b = blend_u8(d, b, f);
}

// FRONT: only the steps in front of the contrast step -- what the mean is taken of.  Otherwise the whole chain with the mean m.
template <bool FRONT>
__device__ __forceinline__ void jitter_pixel(const Jitter& j, int m, int& r, int& g, int& b) {
  if (FRONT && j.op0 == 1) return;
  jitter_step(j.op0, j.f0, m, r, g, b);
  if (FRONT && j.op1 == 1) return;
  jitter_step(j.op1, j.f1, m, r, g, b);
  if (FRONT && j.op2 == 1) return;
  jitter_step(j.op2, j.f2, m, r, g, b);
}

// The PX pixels of group `grp` of a frame as ints: px[k][c].
template <int PX>
__device__ __forceinline__ void load_group(const uint8_t* __restrict__ src, int grp, int (&px)[PX][3]) {
  if (PX == 4) {
    const U32x3 w = *reinterpret_cast<const U32x3*>(src + (size_t)grp * 12);
    const uint32_t words[3] = {w.x, w.y, w.z};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int byte = 3 * k + c;
        px[k][c] = (int)((words[byte >> 2] >> (8 * (byte & 3))) & 255u);
      }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) px[0][c] = src[(size_t)grp * 3 + c];
  }
}

__device__ __forceinline__ const uint8_t* frame_of(const uint8_t* __restrict__ frames, const int64_t* __restrict__ picked, int f, int64_t Ftot,
                                                   int frame_bytes) {
  int64_t row = picked[f];
  row = row < 0 ? 0 : (row >= Ftot ? Ftot - 1 : row);  // the contents of an index array are the caller's: a wrong frame, never a stray read
  return frames + (size_t)row * (size_t)frame_bytes;
}

template <int PX>
__global__ __launch_bounds__(kFrameThreads) void frames_gray_kernel(const uint8_t* __restrict__ frames, int64_t Ftot, int groups, int frame_bytes,
                                                                    const int64_t* __restrict__ picked, const float* __restrict__ factor,
                                                                    const uint8_t* __restrict__ order,
                                                                    unsigned long long* __restrict__ gray_sum) {
  __shared__ int wsum[kFrameThreads / kWave];
  const int f = blockIdx.y, tid = threadIdx.x;
  const Jitter j = load_jitter(factor, order, f);
  if (!j.has_contrast()) return;  // (uniform over the workgroup) nobody reads this frame's sum
  const uint8_t* src = frame_of(frames, picked, f, Ftot, frame_bytes);
  int sum = 0;
#pragma unroll
  for (int u = 0; u < kFrameGroups; ++u) {
    const int grp = (blockIdx.x * kFrameGroups + u) * kFrameThreads + tid;
    if (grp < groups) {
      int px[PX][3];
      load_group<PX>(src, grp, px);
#pragma unroll
      for (int k = 0; k < PX; ++k) {
        jitter_pixel<true>(j, 0, px[k][0], px[k][1], px[k][2]);
        sum += gray_u8(px[k][0], px[k][1], px[k][2]);
      }
    }
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, kWave);
  if ((tid & (kWave - 1)) == 0) wsum[tid / kWave] = sum;
  __syncthreads();
  if (tid == 0) {
    int total = 0;  // <= 4096 pixels * 255
#pragma unroll
    for (int i = 0; i < kFrameThreads / kWave; ++i) total += wsum[i];
    if (total) atomicAdd(&gray_sum[f], (unsigned long long)total);
  }
}

// One group of one frame: the chain, the table, the flip and the store.
template <int PX, bool CHANNELS_LAST>
__device__ __forceinline__ void frames_finish_group(const uint8_t* __restrict__ src, int grp, bool jitter, const Jitter& j, int m, bool mirror,
                                                    int W, int hw, const float* table, float* __restrict__ dst) {
  int px[PX][3];
  load_group<PX>(src, grp, px);
  if (jitter) {
#pragma unroll
    for (int k = 0; k < PX; ++k) jitter_pixel<false>(j, m, px[k][0], px[k][1], px[k][2]);
  }
  int first = grp * PX;  // the group's first pixel in the output; a mirrored group lands at the other end of its row, reversed
  if (mirror) {
    const int y = first / W, x = first - y * W;
    first = y * W + (W - PX - x);
  }
  if (PX == 4) {
    float v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[k][c] = table[c * 256 + (mirror ? px[3 - k][c] : px[k][c])];  // (constant indices: px stays in registers)
    }
    if (CHANNELS_LAST) {
      f32x4* o = reinterpret_cast<f32x4*>(dst + (size_t)first * 3);
      o[0] = f32x4{v[0][0], v[0][1], v[0][2], v[1][0]};
      o[1] = f32x4{v[1][1], v[1][2], v[2][0], v[2][1]};
      o[2] = f32x4{v[2][2], v[3][0], v[3][1], v[3][2]};
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(dst + (size_t)c * hw + first) = f32x4{v[0][c], v[1][c], v[2][c], v[3][c]};
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = table[c * 256 + px[0][c]];
      if (CHANNELS_LAST)
        dst[(size_t)first * 3 + c] = v;
      else
        dst[(size_t)c * hw + first] = v;
    }
  }
}

template <int PX, bool CHANNELS_LAST>
__global__ __launch_bounds__(kFrameThreads) void frames_finish_kernel(const uint8_t* __restrict__ frames, int64_t Ftot, int W, int groups,
                                                                      int frame_bytes, const int64_t* __restrict__ picked,
                                                                      const float* __restrict__ factor, const uint8_t* __restrict__ order,
                                                                      const uint8_t* __restrict__ flip, const float* __restrict__ mean_std,
                                                                      const unsigned long long* __restrict__ gray_sum,
                                                                      float* __restrict__ out) {
  __shared__ float table[3 * 256];
  __shared__ int mean_gray;
  const int f = blockIdx.y, tid = threadIdx.x;
  Jitter j = {3, 3, 3, 1.f, 1.f, 1.f};
  if (order) {
    j = load_jitter(factor, order, f);
    if (tid == 0 && j.has_contrast()) {  // PIL's int(S / n + 0.5) in integers, once per workgroup
      const unsigned long long n = (unsigned long long)groups * PX;
      mean_gray = (int)((2ull * gray_sum[f] + n) / (2ull * n));
    }
  }
  // numpy's float32 arithmetic: fl32(u / 255.f), then fl32(fl32(v - mean) / std), IEEE divisions
  for (int e = tid; e < 3 * 256; e += kFrameThreads) {
    const int c = e >> 8;
    float v = (float)(e & 255) / 255.f;
    if (mean_std) v = (v - mean_std[c]) / mean_std[3 + c];
    table[e] = v;
  }
  __syncthreads();
  const int m = j.has_contrast() ? mean_gray : 0;
  const bool mirror = flip != nullptr && flip[f] != 0;
  const uint8_t* src = frame_of(frames, picked, f, Ftot, frame_bytes);
  float* dst = out + (size_t)f * (size_t)frame_bytes;
  const int hw = groups * PX;
  for (int u = 0; u < kFrameGroups; ++u) {
    const int grp = (blockIdx.x * kFrameGroups + u) * kFrameThreads + tid;
    if (grp >= groups) return;  // (grp grows with u)
    frames_finish_group<PX, CHANNELS_LAST>(src, grp, order != nullptr, j, m, mirror, W, hw, table, dst);
  }
}

template <int PX>
void launch_frames(const uint8_t* frames, int64_t Ftot, int W, int hw, const int64_t* picked, int nf, const float* factor,
                   const uint8_t* order, const uint8_t* flip, const float* mean_std, int channels_last, float* out,
                   unsigned long long* gray_sum, hipStream_t s) {
  const int groups = hw / PX, frame_bytes = hw * 3;
  const dim3 grid((unsigned)cdiv(groups, kFrameThreads * kFrameGroups), (unsigned)nf), block(kFrameThreads);
  if (order)
    hipLaunchKernelGGL(frames_gray_kernel<PX>, grid, block, 0, s, frames, Ftot, groups, frame_bytes, picked, factor, order, gray_sum);
  if (channels_last)
    hipLaunchKernelGGL((frames_finish_kernel<PX, true>), grid, block, 0, s, frames, Ftot, W, groups, frame_bytes, picked, factor, order, flip,
                       mean_std, gray_sum, out);
  else
    hipLaunchKernelGGL((frames_finish_kernel<PX, false>), grid, block, 0, s, frames, Ftot, W, groups, frame_bytes, picked, factor, order, flip,
                       mean_std, gray_sum, out);
}

}  // namespace

MVP_API size_t mvp_prepare_frames_workspace(int64_t Nf) { return Nf > 0 ? (size_t)Nf * sizeof(unsigned long long) : 0; }

MVP_API int mvp_prepare_frames_u8(const uint8_t* frames, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, int64_t Nf,
                                  const float* factor, const uint8_t* order, const uint8_t* flip, const float* mean_std, int channels_last,
                                  float* out, void* workspace, mvp_stream_t stream) {
  MVP_NONNULL(frames);
  MVP_NONNULL(picked);
  MVP_NONNULL(out);
  MVP_REQUIRE(Ftot >= 1 && H >= 1 && W >= 1 && Nf >= 1);
  MVP_REQUIRE((factor == nullptr) == (order == nullptr));
  // each factor is bounded before it enters a product: no int64 product here can overflow
  if (H >= (1ll << 31) || W >= (1ll << 31) || H * W * 3 >= (1ll << 31)) return MVP_EUNSUPPORTED;
  if (order) {
    MVP_NONNULL(workspace);
    MVP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* gray_sum = static_cast<unsigned long long*>(workspace);
  if (order) {
    hipError_t e = hipMemsetAsync(gray_sum, 0, sizeof(unsigned long long) * (size_t)Nf, s);
    if (e != hipSuccess) return (int)e;
  }
  const int hw = (int)(H * W);
  const bool wide = W % 4 == 0 && reinterpret_cast<uintptr_t>(frames) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  for (int64_t f0 = 0; f0 < Nf; f0 += kMaxGridY) {  // (the y extent of a grid ends at 65535)
    const int nf = (int)(Nf - f0 < kMaxGridY ? Nf - f0 : kMaxGridY);
    const float* fac = factor ? factor + f0 * 3 : nullptr;
    const uint8_t* ord = order ? order + f0 * 3 : nullptr;
    const uint8_t* flp = flip ? flip + f0 : nullptr;
    float* o = out + (size_t)f0 * 3 * (size_t)hw;
    if (wide)
      launch_frames<4>(frames, Ftot, (int)W, hw, picked + f0, nf, fac, ord, flp, mean_std, channels_last, o, order ? gray_sum + f0 : nullptr, s);
    else
      launch_frames<1>(frames, Ftot, (int)W, hw, picked + f0, nf, fac, ord, flp, mean_std, channels_last, o, order ? gray_sum + f0 : nullptr, s);
  }
  return mvp_launch_status();
}

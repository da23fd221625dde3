// frame_eval.hip -- what surrounds stage one (the 2D network), on the device for gfx950: the confusion matrix of a batch of frames against
// raw 16-bit label images (mvpnet/test_2d.py:103-118, the validation pass of mvpnet/train_2d.py:240-312) and the label histograms behind
// the class weights (mvpnet/data/preprocess/compute_label_weights.py).  Definitions: include/mvp_hip.h, mvp_frame_confusion_f32 /
// mvp_label_histogram_u16 / mvp_label_histogram_i64.
//
//   frame_confusion_kernel : one lane per output pixel.  The lane reads its label as labels_kernel (resize.hip) does -- picked frame,
//                            Pillow's NEAREST indices, the mapping -- and the argmax of its C logits as seg_confusion_kernel (seg.hip) does,
//                            and counts the pair; the (Nf,h,w) int64 label tensor that lies between those two kernels is never written.
//   frame_histogram_kernel : the same label read, counted into bins.   label_histogram_kernel: a flat int64 label array counted into bins.
//
// The frame kernels' grid is (workgroups per frame, frames), as resize.hip's: the frame -- its picked row, its 64-bit label and logit bases
// -- is uniform in a workgroup and every offset inside it is 32-bit, no division by the frame size.  A frame's workgroups walk its pixels
// with a grid stride; there are about kMatBlocks (kHistBlocks) workgroups in all, each with its own histogram.
// Both chains of loads of a pixel -- label -> mapping, and the logits -- are issued unconditionally, so neither waits for the other: an
// ignored pixel's logits are read too (they are needed anyway when `pred` is asked for).
// Logit loads: with ld_x == 1 the lanes of a wave walk x, every per-channel load is contiguous; with ld_c == 1 (channels-last, C % 4 == 0,
// C <= 32, 16-byte aligned rows: frame_confusion_kernel<true>) a lane reads its row as C / 4 16-byte loads, the per-lane form of seg.hip's
// row_lse -- its wave tile in LDS would cost 8 KB per wave on top of the histogram.
// Counts: a workgroup-private histogram in LDS (16 KB: kMaxHist 32-bit counters, a workgroup sees fewer than 2^31 pixels) flushed with
// 64-bit integer atomics, every workgroup starting its flush at another bin so that concurrent flushes spread over the cache lines of the
// result; global 64-bit atomics beyond.  Integer sums only: the same bits every run.
#include "common.h"
#include <algorithm>

namespace {

constexpr int kFT = 256;
constexpr int kMaxHist = 4096;     // LDS counters: C <= 64 for the matrix, nbins <= 4096 for a histogram
constexpr int kRegC = 32;          // up to here a pixel's logits are loaded together (seg.hip)
// Workgroups of a launch.  Every workgroup ends in one 64-bit atomic per nonzero counter, and atomics on ONE address queue at the memory
// side: the flushes, not the pixels, set the kernel's time once there are many workgroups.  32 frames of 120 x 160, C = 20, dense random
// counts (tools/exp/frame_eval_time.py): the matrix 21.1 us with 256 workgroups, 21.5 with 512, 31 with 1024, 47 with 2048; the 20-bin
// histogram 11.5 us with 128, 9.7 with 256, 11.9 with 512, 19.2 with 1024.
constexpr int kMatBlocks = 256;
constexpr int kHistBlocks = 256;
constexpr int kFlatBlocks = 1024;  // the int64 stream (a 3D store's labels, 8 bytes a lane) keeps its lanes; its workgroup count is not measured
constexpr int kMaxGridY = 65535;   // frames per launch

struct FrameLabels {
  const uint16_t* labels;  // (Ftot,H,W)
  int64_t Ftot;
  int H, W;
  const int64_t* picked;  // the launch's frames
  int h, w;
  const int32_t* yi;       // (h) or NULL
  const int32_t* xi;       // (w) or NULL
  const int64_t* mapping;  // (T,) or NULL
  int64_t T;
};

// the label image of the workgroup's frame: picked row blockIdx.y, clamped (the contents of an index array are the caller's)
__device__ __forceinline__ const uint16_t* label_frame(const FrameLabels& a) {
  int64_t row = a.picked[blockIdx.y];
  row = row < 0 ? 0 : (row >= a.Ftot ? a.Ftot - 1 : row);
  return a.labels + (size_t)row * (size_t)(a.H * a.W);
}

// labels_kernel's read without the flip: the mapped label of output pixel (y, x)
__device__ __forceinline__ int64_t frame_label(const FrameLabels& a, const uint16_t* __restrict__ frame, int y, int x, int64_t ignore_value) {
  int sy = a.yi ? a.yi[y] : y, sx = a.xi ? a.xi[x] : x;
  sy = sy < 0 ? 0 : (sy > a.H - 1 ? a.H - 1 : sy);  // (the tables are the caller's)
  sx = sx < 0 ? 0 : (sx > a.W - 1 ? a.W - 1 : sx);
  const int64_t raw = frame[sy * a.W + sx];
  return a.mapping ? (raw < a.T ? a.mapping[raw] : ignore_value) : raw;
}

// The float at byte offset (pixel + channel) of a logit frame.  Both offsets are UNSIGNED 32-bit and are added in 32 bits before they meet
// the frame pointer (the host bounds a frame's extent to 2^30 elements: no wrap), so a wave-uniform channel offset is ONE scalar register:
// as 64-bit addends the 32 of argmax_row took 64 and spilled.
__device__ __forceinline__ float frame_at(const char* __restrict__ frame, unsigned pixel, unsigned channel) {
  return *reinterpret_cast<const float*>(frame + (size_t)(pixel + channel));
}

// the first maximum of the pixel's C logits by `>`, as seg_confusion_kernel.  kQuads: ld_c == 1, C % 4 == 0, C <= kRegC, 16-byte aligned rows
template <bool kQuads>
__device__ __forceinline__ int argmax_row(const char* __restrict__ frame, unsigned pixel, int ld_c, int C) {
  int am = 0;
  if (kQuads || C <= kRegC) {
    float x[kRegC];
    if (kQuads) {
#pragma unroll
      for (int q = 0; q < kRegC / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(frame + (size_t)(pixel + 16u * (unsigned)min(q, C / 4 - 1)));  // quads >= C / 4 repeat the last
        x[4 * q + 0] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < kRegC; ++c) x[c] = frame_at(frame, pixel, (unsigned)(min(c, C - 1) * ld_c) * 4u);
    }
    // entries >= C repeat one the scan has passed already: they never win a strict `>`, no test per class (32 wave-uniform masks)
    float mx = x[0];
#pragma unroll
    for (int c = 1; c < kRegC; ++c)
      if (x[c] > mx) {
        mx = x[c];
        am = c;
      }
  } else {
    float mx = frame_at(frame, pixel, 0u);
    for (int c = 1; c < C; ++c) {
      const float v = frame_at(frame, pixel, (unsigned)(c * ld_c) * 4u);
      if (v > mx) {
        mx = v;
        am = c;
      }
    }
  }
  return am;
}

// hist (n 32-bit LDS counters) added to out, the nonzero ones, from a start that differs per workgroup
__device__ __forceinline__ void flush_counters(const unsigned int* hist, int n, unsigned long long* __restrict__ out) {
  const int start = (int)(((blockIdx.y * gridDim.x + blockIdx.x) * 67u) % (unsigned)n);
  for (int k = threadIdx.x; k < n; k += kFT) {
    int i = start + k;
    i = i >= n ? i - n : i;
    if (hist[i]) atomicAdd(out + i, (unsigned long long)hist[i]);
  }
}

// logit, pred: the launch's first frame.  ld_c, ld_y, ld_x and every offset inside a logit frame fit 32 bits (checked on the host).
template <bool kQuads>
__global__ __launch_bounds__(kFT) void frame_confusion_kernel(const float* __restrict__ logit, int C, int64_t ld_f, int ld_c, int ld_y, int ld_x,
                                                              FrameLabels a, int64_t ignore_value, unsigned long long* __restrict__ mat,
                                                              int64_t* __restrict__ pred) {
  __shared__ unsigned int hist[kMaxHist];
  const bool lds = mat != nullptr && C * C <= kMaxHist;
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += kFT) hist[i] = 0u;
  __syncthreads();
  const unsigned hw = (unsigned)(a.h * a.w);
  const uint16_t* lab_frame = mat != nullptr ? label_frame(a) : nullptr;
  const char* frame = reinterpret_cast<const char*>(logit + (int64_t)blockIdx.y * ld_f);
  int64_t* pred_frame = pred != nullptr ? pred + (size_t)blockIdx.y * hw : nullptr;
  for (unsigned i = blockIdx.x * kFT + threadIdx.x; i < hw; i += gridDim.x * kFT) {  // (hw < 2^31, the stride <= 2^24: no wrap)
    const int y = (int)i / a.w, x = (int)i - y * a.w;
    const int64_t lab = mat != nullptr ? frame_label(a, lab_frame, y, x, ignore_value) : -1;
    const int am = argmax_row<kQuads>(frame, (unsigned)(y * ld_y + x * ld_x) * 4u, ld_c, C);
    if (pred_frame != nullptr) pred_frame[i] = am;
    if (lab < 0 || lab >= C) continue;
    if (lds)
      atomicAdd(&hist[(int)lab * C + am], 1u);
    else
      atomicAdd(mat + lab * C + am, 1ull);
  }
  __syncthreads();
  if (lds) flush_counters(hist, C * C, mat);
}

__global__ __launch_bounds__(kFT) void frame_histogram_kernel(FrameLabels a, int nbins, unsigned long long* __restrict__ out) {
  __shared__ unsigned int hist[kMaxHist];
  const bool lds = nbins <= kMaxHist;
  if (lds)
    for (int i = threadIdx.x; i < nbins; i += kFT) hist[i] = 0u;
  __syncthreads();
  const unsigned hw = (unsigned)(a.h * a.w);
  const uint16_t* lab_frame = label_frame(a);
  for (unsigned i = blockIdx.x * kFT + threadIdx.x; i < hw; i += gridDim.x * kFT) {
    const int y = (int)i / a.w;
    const int64_t v = frame_label(a, lab_frame, y, (int)i - y * a.w, -1);
    if (v < 0 || v >= nbins) continue;
    if (lds)
      atomicAdd(&hist[(int)v], 1u);
    else
      atomicAdd(out + v, 1ull);
  }
  __syncthreads();
  if (lds) flush_counters(hist, nbins, out);
}

__global__ __launch_bounds__(kFT) void label_histogram_kernel(const int64_t* __restrict__ label, int64_t n, int nbins,
                                                              unsigned long long* __restrict__ out) {
  __shared__ unsigned int hist[kMaxHist];
  const bool lds = nbins <= kMaxHist;
  if (lds)
    for (int i = threadIdx.x; i < nbins; i += kFT) hist[i] = 0u;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * kFT + threadIdx.x; p < n; p += (int64_t)gridDim.x * kFT) {
    const int64_t v = label[p];
    if (v < 0 || v >= nbins) continue;
    if (lds)
      atomicAdd(&hist[(int)v], 1u);
    else
      atomicAdd(out + v, 1ull);
  }
  __syncthreads();
  if (lds) flush_counters(hist, nbins, out);
}

// the label arguments the two frame entries share; MVP_OK or the code to return
int check_frame_labels(int64_t Ftot, int64_t H, int64_t W, int64_t Nf, int64_t h, int64_t w, const int32_t* yi, const int32_t* xi, int64_t T) {
  MVP_REQUIRE(Ftot >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && Nf >= 1 && T >= 0);
  MVP_REQUIRE((yi != nullptr) == (h != H) && (xi != nullptr) == (w != W));
  return MVP_OK;
}

// each factor is bounded before it enters a product: no int64 product here can overflow
bool frame_too_large(int64_t H, int64_t W, int64_t h, int64_t w) {
  return H >= (1ll << 31) || W >= (1ll << 31) || h >= (1ll << 31) || w >= (1ll << 31) || H * W >= (1ll << 31) || h * w >= (1ll << 31);
}

// workgroups per frame: about `most` in all over the launch's nf frames, one at least, no more than the frame has pixels for
unsigned blocks_per_frame(int64_t hw, int64_t nf, int most) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(most, nf), cdiv(hw, kFT)));
}

}  // namespace

MVP_API int mvp_frame_confusion_f32(const float* logit, int64_t Nf, int64_t C, int64_t h, int64_t w, int64_t ld_f, int64_t ld_c, int64_t ld_y,
                                    int64_t ld_x, const uint16_t* labels, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked,
                                    const int32_t* yi, const int32_t* xi, const int64_t* mapping, int64_t T, int64_t ignore_value, int64_t* mat,
                                    int64_t* pred, mvp_stream_t stream) {
  MVP_NONNULL(logit);
  if (labels != nullptr && mat != nullptr) MVP_NONNULL(picked);
  if (labels == nullptr && mat == nullptr) MVP_NONNULL(pred);
  MVP_REQUIRE((labels == nullptr) == (mat == nullptr));
  MVP_REQUIRE(C >= 1 && ld_f >= 0 && ld_c >= 0 && ld_y >= 0 && ld_x >= 0);
  int rc = check_frame_labels(Ftot, H, W, Nf, h, w, yi, xi, T);
  if (rc) return rc;
  if (C >= (1 << 16) || frame_too_large(H, W, h, w)) return MVP_EUNSUPPORTED;
  // a logit frame is addressed with 32-bit byte offsets (each stride is bounded before it enters a product)
  if (ld_c >= (1ll << 30) || ld_y >= (1ll << 30) || ld_x >= (1ll << 30) || (C - 1) * ld_c + (h - 1) * ld_y + (w - 1) * ld_x >= (1ll << 30))
    return MVP_EUNSUPPORTED;
  const bool quads = ld_c == 1 && C % 4 == 0 && C <= kRegC && reinterpret_cast<uintptr_t>(logit) % 16 == 0 && ld_f % 4 == 0 && ld_y % 4 == 0 && ld_x % 4 == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* m = reinterpret_cast<unsigned long long*>(mat);
  for (int64_t f0 = 0; f0 < Nf; f0 += kMaxGridY) {  // (the y extent of a grid ends at 65535: one launch up to there)
    const int64_t nf = std::min<int64_t>(Nf - f0, kMaxGridY);
    const FrameLabels a = {labels, Ftot, (int)H, (int)W, picked ? picked + f0 : nullptr, (int)h, (int)w, yi, xi, mapping, T};
    const dim3 grid(blocks_per_frame(h * w, nf, kMatBlocks), (unsigned)nf), block(kFT);
    const float* lg = logit + f0 * ld_f;
    int64_t* pr = pred ? pred + f0 * (h * w) : nullptr;
    if (quads)
      hipLaunchKernelGGL(frame_confusion_kernel<true>, grid, block, 0, s, lg, (int)C, ld_f, 1, (int)ld_y, (int)ld_x, a, ignore_value, m, pr);
    else
      hipLaunchKernelGGL(frame_confusion_kernel<false>, grid, block, 0, s, lg, (int)C, ld_f, (int)ld_c, (int)ld_y, (int)ld_x, a, ignore_value, m, pr);
  }
  return mvp_launch_status();
}

MVP_API int mvp_label_histogram_u16(const uint16_t* labels, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, int64_t Nf, int64_t h,
                                    int64_t w, const int32_t* yi, const int32_t* xi, const int64_t* mapping, int64_t T, int64_t nbins,
                                    int64_t* hist, mvp_stream_t stream) {
  MVP_NONNULL(labels);
  MVP_NONNULL(picked);
  MVP_NONNULL(hist);
  MVP_REQUIRE(nbins >= 1);
  int rc = check_frame_labels(Ftot, H, W, Nf, h, w, yi, xi, T);
  if (rc) return rc;
  if (nbins > MVP_HISTOGRAM_MAX_BINS || frame_too_large(H, W, h, w)) return MVP_EUNSUPPORTED;
  for (int64_t f0 = 0; f0 < Nf; f0 += kMaxGridY) {
    const int64_t nf = std::min<int64_t>(Nf - f0, kMaxGridY);
    const FrameLabels a = {labels, Ftot, (int)H, (int)W, picked + f0, (int)h, (int)w, yi, xi, mapping, T};
    hipLaunchKernelGGL(frame_histogram_kernel, dim3(blocks_per_frame(h * w, nf, kHistBlocks), (unsigned)nf), dim3(kFT), 0,
                       static_cast<hipStream_t>(stream), a, (int)nbins, reinterpret_cast<unsigned long long*>(hist));
  }
  return mvp_launch_status();
}

MVP_API int mvp_label_histogram_i64(const int64_t* label, int64_t n, int64_t nbins, int64_t* hist, mvp_stream_t stream) {
  MVP_NONNULL(label);
  MVP_NONNULL(hist);
  MVP_REQUIRE(n >= 0 && nbins >= 1);
  if (nbins > MVP_HISTOGRAM_MAX_BINS || n >= (1ll << 40)) return MVP_EUNSUPPORTED;  // (32-bit counters: fewer than 2^32 labels per workgroup)
  if (n == 0) return MVP_OK;
  hipLaunchKernelGGL(label_histogram_kernel, dim3((unsigned)std::min<int64_t>(kFlatBlocks, cdiv(n, kFT))), dim3(kFT), 0,
                     static_cast<hipStream_t>(stream), label, n, (int)nbins, reinterpret_cast<unsigned long long*>(hist));
  return mvp_launch_status();
}

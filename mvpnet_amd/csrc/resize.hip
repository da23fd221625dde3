// resize.hip -- the 2D stage's loader steps that change an image's size, on the device for gfx950: what a data-loader worker does per frame
// in the reference with `image.resize(size, Image.BILINEAR)` and `label.resize(size, Image.NEAREST)` (mvpnet/data/scannet_2d.py:153-156,
// mvpnet/data/scannet_2d3d.py:234-239), the label mapping (:167-168) and the label's half of the flip (:161-163).  Definitions (pinned,
// bit-identical to Pillow on uint8 RGB and on 16-bit label images): include/mvp_hip.h, mvp_resize_frames_u8 / mvp_prepare_labels_u16.
//
//   host tables          : Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter and the nearest index of a 16-bit
//                          image, in double on the host (mvp_resize_bilinear_table, mvp_resize_nearest_table: no GPU).  The caller
//                          uploads them once per (device, size pair).
//   resize_hv_kernel     : both axes change.  A workgroup of 256 lanes owns a tile of kTileH x kTileW output pixels: the horizontal pass
//                          for the input rows the tile's output rows draw on, ROUNDED TO uint8 as Pillow's intermediate image is, into
//                          LDS; a barrier; the vertical pass from LDS.  32-bit integer arithmetic throughout: 255 * 2^22 < 2^31.
//   resize_h / resize_v  : one axis changes: that pass alone, global to global, no LDS.
//   gather_frames_kernel : neither changes: the picked frames are copied, 16 bytes per lane where the alignment allows.
//   labels_kernel        : label[picked, yi[y], xi[flip ? w-1-x : x]] through the mapping, int64.
//
// LDS: kMaxRows x kTileW x 3 = 18432 bytes per workgroup (8 workgroups = 8 waves per SIMD fit a CU's 160 KiB).  A tile of kTileH output rows
// draws on at most (kTileH - 1) * scale + 2 * support + 2 input rows (scale = H / h, support = max(scale, 1)): the entry refuses a size pair
// beyond kMaxRows (H / h up to ~21; 968 -> 120 needs 75 rows) or with more than kMaxTaps taps on either axis, and launches nothing.
// The vertical pass reads bytes (ds_read_u8): the 32 lanes of a tile row read 96 consecutive bytes = 24 banks, the two tile rows of a wave
// sit whole input rows apart -- at worst a two-way conflict on the rows that both halves share.  The horizontal pass reads its taps as
// bytes from global memory: neighbouring lanes' windows overlap (at 640 -> 160 a lane's 8 pixels start 4 pixels behind its neighbour's), so
// every line is fetched once from L2 and the rest are L1 hits; the pixels are 3 bytes, no wider load is aligned.
// Measurements: DESIGN.md (2D stage).
#include <math.h>

#include "common.h"

namespace {

constexpr int kResizeThreads = 256;
constexpr int kTileW = 32, kTileH = 8;  // kTileW * kTileH == kResizeThreads: one output pixel per lane in the vertical pass
constexpr int kMaxRows = 192;           // input rows of a tile's intermediate image in LDS
constexpr int kMaxTaps = 64;
constexpr int kPrecisionBits = 32 - 8 - 2;  // Pillow's PRECISION_BITS for 8-bit channels
constexpr int kMaxGridY = 65535;

struct __attribute__((aligned(16))) Bytes16 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kPrecisionBits;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// acc + pixel * coef in wrapping arithmetic: the tables are the caller's, a wrong one gives a wrong pixel and nothing else
__device__ __forceinline__ int mac(int acc, int pixel, int coef) { return (int)((uint32_t)acc + (uint32_t)pixel * (uint32_t)coef); }

// One axis' table on the device: [first input index (outS) | taps (outS) | coefficients (outS * k)].  The window of output i, clamped
// into [0, inS): never a stray read whatever the table holds.
__device__ __forceinline__ void window_of(const int32_t* __restrict__ tab, int outS, int k, int inS, int i, int& lo, int& cnt) {
  lo = tab[i];
  cnt = tab[outS + i];
  lo = lo < 0 ? 0 : (lo > inS - 1 ? inS - 1 : lo);
  cnt = cnt < 0 ? 0 : (cnt > k ? k : cnt);
  if (cnt > inS - lo) cnt = inS - lo;
}

__device__ __forceinline__ const uint8_t* picked_frame(const uint8_t* __restrict__ base, const int64_t* __restrict__ picked, int f, int64_t Ftot,
                                                       size_t frame_bytes) {
  int64_t row = picked[f];
  row = row < 0 ? 0 : (row >= Ftot ? Ftot - 1 : row);  // the contents of an index array are the caller's: a wrong frame, never a stray read
  return base + (size_t)row * frame_bytes;
}

// The horizontal pass for one pixel: p = the first tap's pixel, kx = its coefficients.
__device__ __forceinline__ void taps_rgb(const uint8_t* __restrict__ p, const int32_t* __restrict__ kx, int cnt, int& r, int& g, int& b) {
  int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < cnt; ++t) {
    const int c = kx[t];
    a0 = mac(a0, p[3 * t + 0], c);
    a1 = mac(a1, p[3 * t + 1], c);
    a2 = mac(a2, p[3 * t + 2], c);
  }
  r = clip8(a0);
  g = clip8(a1);
  b = clip8(a2);
}

__global__ __launch_bounds__(kResizeThreads) void resize_hv_kernel(const uint8_t* __restrict__ frames, int64_t Ftot, int H, int W,
                                                                   const int64_t* __restrict__ picked, int h, int w,
                                                                   const int32_t* __restrict__ xtab, int xk, const int32_t* __restrict__ ytab,
                                                                   int yk, int tiles_x, uint8_t* __restrict__ out) {
  __shared__ uint8_t inter[kMaxRows * kTileW * 3];
  const int f = blockIdx.y, tid = threadIdx.x;
  const int x0 = (blockIdx.x % tiles_x) * kTileW, y0 = (blockIdx.x / tiles_x) * kTileH;
  const int y_last = (y0 + kTileH < h ? y0 + kTileH : h) - 1;
  const uint8_t* src = picked_frame(frames, picked, f, Ftot, (size_t)H * W * 3);
  int row0, cnt0, row1, cnt1;
  window_of(ytab, h, yk, H, y0, row0, cnt0);
  window_of(ytab, h, yk, H, y_last, row1, cnt1);
  int nrows = row1 + cnt1 - row0;  // (the windows' starts and ends grow with y)
  nrows = nrows < 0 ? 0 : (nrows > kMaxRows ? kMaxRows : nrows);
  const int32_t* xcoef = xtab + 2 * (size_t)w;
  for (int i = tid; i < nrows * kTileW; i += kResizeThreads) {
    const int x = x0 + (i & (kTileW - 1));
    if (x >= w) continue;
    int lo, cnt, r, g, b;
    window_of(xtab, w, xk, W, x, lo, cnt);
    taps_rgb(src + ((size_t)(row0 + (i / kTileW)) * W + lo) * 3, xcoef + (size_t)x * xk, cnt, r, g, b);
    inter[i * 3 + 0] = (uint8_t)r;
    inter[i * 3 + 1] = (uint8_t)g;
    inter[i * 3 + 2] = (uint8_t)b;
  }
  __syncthreads();
  const int oy = y0 + tid / kTileW, ox = x0 + (tid & (kTileW - 1));
  if (oy >= h || ox >= w) return;
  int lo, cnt;
  window_of(ytab, h, yk, H, oy, lo, cnt);
  int rel = lo - row0;
  if (rel < 0) rel = 0, cnt = 0;
  if (cnt > nrows - rel) cnt = nrows - rel < 0 ? 0 : nrows - rel;
  const int32_t* ky = ytab + 2 * (size_t)h + (size_t)oy * yk;
  const uint8_t* p = inter + ((size_t)rel * kTileW + (tid & (kTileW - 1))) * 3;
  int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < cnt; ++t) {
    const int c = ky[t];
    a0 = mac(a0, p[t * kTileW * 3 + 0], c);
    a1 = mac(a1, p[t * kTileW * 3 + 1], c);
    a2 = mac(a2, p[t * kTileW * 3 + 2], c);
  }
  uint8_t* dst = out + (((size_t)f * h + oy) * w + ox) * 3;
  dst[0] = (uint8_t)clip8(a0);
  dst[1] = (uint8_t)clip8(a1);
  dst[2] = (uint8_t)clip8(a2);
}

// Only the width changes (h == H): one output pixel per lane.
__global__ __launch_bounds__(kResizeThreads) void resize_h_kernel(const uint8_t* __restrict__ frames, int64_t Ftot, int H, int W,
                                                                  const int64_t* __restrict__ picked, int w, const int32_t* __restrict__ xtab,
                                                                  int xk, uint8_t* __restrict__ out) {
  const int f = blockIdx.y;
  const int i = blockIdx.x * kResizeThreads + threadIdx.x;
  if (i >= H * w) return;
  const int y = i / w, x = i - y * w;
  const uint8_t* src = picked_frame(frames, picked, f, Ftot, (size_t)H * W * 3);
  int lo, cnt, r, g, b;
  window_of(xtab, w, xk, W, x, lo, cnt);
  taps_rgb(src + ((size_t)y * W + lo) * 3, xtab + 2 * (size_t)w + (size_t)x * xk, cnt, r, g, b);
  uint8_t* dst = out + ((size_t)f * H * w + i) * 3;
  dst[0] = (uint8_t)r;
  dst[1] = (uint8_t)g;
  dst[2] = (uint8_t)b;
}

// Only the height changes (w == W): one output byte per lane, a wave reads 64 consecutive bytes of every input row.
__global__ __launch_bounds__(kResizeThreads) void resize_v_kernel(const uint8_t* __restrict__ frames, int64_t Ftot, int H, int W,
                                                                  const int64_t* __restrict__ picked, int h, const int32_t* __restrict__ ytab,
                                                                  int yk, uint8_t* __restrict__ out) {
  const int f = blockIdx.y, row_bytes = W * 3;
  const int i = blockIdx.x * kResizeThreads + threadIdx.x;
  if (i >= h * row_bytes) return;
  const int y = i / row_bytes, xb = i - y * row_bytes;
  const uint8_t* src = picked_frame(frames, picked, f, Ftot, (size_t)H * row_bytes);
  int lo, cnt;
  window_of(ytab, h, yk, H, y, lo, cnt);
  const int32_t* ky = ytab + 2 * (size_t)h + (size_t)y * yk;
  const uint8_t* p = src + (size_t)lo * row_bytes + xb;
  int acc = 1 << (kPrecisionBits - 1);
  for (int t = 0; t < cnt; ++t) acc = mac(acc, p[(size_t)t * row_bytes], ky[t]);
  out[(size_t)f * h * row_bytes + i] = (uint8_t)clip8(acc);
}

// Neither changes: the picked frames as they are, `units` elements of T per frame.
template <typename T>
__global__ __launch_bounds__(kResizeThreads) void gather_frames_kernel(const uint8_t* __restrict__ frames, int64_t Ftot, int units,
                                                                       const int64_t* __restrict__ picked, uint8_t* __restrict__ out) {
  const int f = blockIdx.y;
  const int i = blockIdx.x * kResizeThreads + threadIdx.x;
  if (i >= units) return;
  const size_t frame_bytes = (size_t)units * sizeof(T);
  const T* src = reinterpret_cast<const T*>(picked_frame(frames, picked, f, Ftot, frame_bytes));
  reinterpret_cast<T*>(out + (size_t)f * frame_bytes)[i] = src[i];
}

__global__ __launch_bounds__(kResizeThreads) void labels_kernel(const uint16_t* __restrict__ labels, int64_t Ftot, int H, int W,
                                                                const int64_t* __restrict__ picked, int h, int w, const int32_t* __restrict__ yi,
                                                                const int32_t* __restrict__ xi, const uint8_t* __restrict__ flip,
                                                                const int64_t* __restrict__ mapping, int64_t T, int64_t ignore_value,
                                                                int64_t* __restrict__ out) {
  const int f = blockIdx.y;
  const int i = blockIdx.x * kResizeThreads + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  const int xs = (flip != nullptr && flip[f] != 0) ? w - 1 - x : x;
  int sy = yi ? yi[y] : y, sx = xi ? xi[xs] : xs;
  sy = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy);  // (the tables are the caller's)
  sx = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx);
  int64_t row = picked[f];
  row = row < 0 ? 0 : (row >= Ftot ? Ftot - 1 : row);
  const int64_t raw = labels[((size_t)row * H + sy) * W + sx];
  out[(size_t)f * h * w + i] = mapping ? (raw < T ? mapping[raw] : ignore_value) : raw;
}

// Pillow's bilinear_filter
inline double triangle(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// ceil(support) * 2 + 1 of Pillow's precompute_coeffs, or 0 when it does not fit an int comfortably
inline int64_t taps_of(int64_t inS, int64_t outS) {
  const double scale = (double)inS / (double)outS;
  const double support = scale < 1.0 ? 1.0 : scale;
  const double c = ceil(support);
  return c > (double)(1 << 24) ? 0 : (int64_t)c * 2 + 1;
}

// Input rows a tile of kTileH output rows can draw on (an upper bound in double, with slack for the roundings of the bounds).
inline int64_t tile_rows_bound(int64_t H, int64_t h) {
  const double scale = (double)H / (double)h;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int64_t)ceil((kTileH - 1) * scale + 2.0 * support) + 2;
}

}  // namespace

MVP_API int mvp_resize_bilinear_table(int64_t inS, int64_t outS, int32_t* xmin, int32_t* count, int32_t* coef, int32_t* ksize) {
  MVP_NONNULL(ksize);
  MVP_REQUIRE(inS >= 1 && outS >= 1);
  if (inS >= (1ll << 31) || outS >= (1ll << 31)) return MVP_EUNSUPPORTED;
  const int64_t k = taps_of(inS, outS);
  if (k == 0 || k * outS >= (1ll << 31)) return MVP_EUNSUPPORTED;
  *ksize = (int32_t)k;
  if (xmin == nullptr && count == nullptr && coef == nullptr) return MVP_OK;  // the size query
  MVP_NONNULL(xmin);
  MVP_NONNULL(count);
  MVP_NONNULL(coef);
  const double scale = (double)inS / (double)outS;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;  // (the triangle filter's support is 1)
  const double ss = 1.0 / filterscale;
  double* pre = new double[(size_t)k];
  for (int64_t xx = 0; xx < outS; ++xx) {
    const double center = 0.0 + ((double)xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > inS) hi = (int)inS;
    const int n = hi - lo;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      const double wgt = triangle(((double)x + (double)lo - center + 0.5) * ss);
      pre[x] = wgt;
      ww += wgt;
    }
    int32_t* kk = coef + xx * k;
    for (int x = 0; x < (int)k; ++x) {
      double wgt = 0.0;
      if (x < n) wgt = ww != 0.0 ? pre[x] / ww : pre[x];
      kk[x] = wgt < 0.0 ? (int32_t)(-0.5 + wgt * (double)(1 << kPrecisionBits)) : (int32_t)(0.5 + wgt * (double)(1 << kPrecisionBits));
    }
    xmin[xx] = lo;
    count[xx] = n;
  }
  delete[] pre;
  return MVP_OK;
}

MVP_API int mvp_resize_nearest_table(int64_t inS, int64_t outS, int32_t* index) {
  MVP_NONNULL(index);
  MVP_REQUIRE(inS >= 1 && outS >= 1);
  if (inS >= (1ll << 31) || outS >= (1ll << 31)) return MVP_EUNSUPPORTED;
  const double scale = (double)inS / (double)outS;
  for (int64_t x = 0; x < outS; ++x) {
    const int64_t i = (int64_t)(scale * ((double)x + 0.5));
    index[x] = (int32_t)(i < inS - 1 ? i : inS - 1);
  }
  return MVP_OK;
}

MVP_API int mvp_resize_frames_u8(const uint8_t* frames, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, int64_t Nf, int64_t h,
                                 int64_t w, const int32_t* xtab, const int32_t* ytab, uint8_t* out, mvp_stream_t stream) {
  MVP_NONNULL(frames);
  MVP_NONNULL(picked);
  MVP_NONNULL(out);
  MVP_REQUIRE(Ftot >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && Nf >= 1);
  MVP_REQUIRE((xtab != nullptr) == (w != W) && (ytab != nullptr) == (h != H));
  // each factor is bounded before it enters a product: no int64 product here can overflow
  if (H >= (1ll << 31) || W >= (1ll << 31) || h >= (1ll << 31) || w >= (1ll << 31)) return MVP_EUNSUPPORTED;
  if (H * W * 3 >= (1ll << 31) || h * w * 3 >= (1ll << 31) || H * w * 3 >= (1ll << 31) || h * W * 3 >= (1ll << 31)) return MVP_EUNSUPPORTED;
  const int64_t xk = xtab ? taps_of(W, w) : 0, yk = ytab ? taps_of(H, h) : 0;
  if ((xtab && (xk == 0 || xk > kMaxTaps)) || (ytab && (yk == 0 || yk > kMaxTaps))) return MVP_EUNSUPPORTED;
  if (xtab && ytab && tile_rows_bound(H, h) > kMaxRows) return MVP_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kResizeThreads);
  const size_t out_frame = (size_t)h * (size_t)w * 3;
  for (int64_t f0 = 0; f0 < Nf; f0 += kMaxGridY) {  // (the y extent of a grid ends at 65535: one launch up to there)
    const unsigned nf = (unsigned)(Nf - f0 < kMaxGridY ? Nf - f0 : kMaxGridY);
    uint8_t* o = out + (size_t)f0 * out_frame;
    if (xtab && ytab) {
      const int tiles_x = (int)cdiv(w, kTileW), tiles_y = (int)cdiv(h, kTileH);
      if ((int64_t)tiles_x * tiles_y >= (1ll << 31)) return MVP_EUNSUPPORTED;
      hipLaunchKernelGGL(resize_hv_kernel, dim3((unsigned)(tiles_x * tiles_y), nf), block, 0, s, frames, Ftot, (int)H, (int)W, picked + f0, (int)h,
                         (int)w, xtab, (int)xk, ytab, (int)yk, tiles_x, o);
    } else if (xtab) {
      hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)cdiv(H * w, kResizeThreads), nf), block, 0, s, frames, Ftot, (int)H, (int)W, picked + f0,
                         (int)w, xtab, (int)xk, o);
    } else if (ytab) {
      hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)cdiv(h * W * 3, kResizeThreads), nf), block, 0, s, frames, Ftot, (int)H, (int)W,
                         picked + f0, (int)h, ytab, (int)yk, o);
    } else if (out_frame % 16 == 0 && reinterpret_cast<uintptr_t>(frames) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) {
      const int units = (int)(out_frame / 16);
      hipLaunchKernelGGL(gather_frames_kernel<Bytes16>, dim3((unsigned)cdiv(units, kResizeThreads), nf), block, 0, s, frames, Ftot, units,
                         picked + f0, o);
    } else {
      hipLaunchKernelGGL(gather_frames_kernel<uint8_t>, dim3((unsigned)cdiv((int64_t)out_frame, kResizeThreads), nf), block, 0, s, frames, Ftot,
                         (int)out_frame, picked + f0, o);
    }
  }
  return mvp_launch_status();
}

MVP_API int mvp_prepare_labels_u16(const uint16_t* labels, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, int64_t Nf, int64_t h,
                                   int64_t w, const int32_t* yi, const int32_t* xi, const uint8_t* flip, const int64_t* mapping, int64_t T,
                                   int64_t ignore_value, int64_t* out, mvp_stream_t stream) {
  MVP_NONNULL(labels);
  MVP_NONNULL(picked);
  MVP_NONNULL(out);
  MVP_REQUIRE(Ftot >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && Nf >= 1);
  MVP_REQUIRE((yi != nullptr || h == H) && (xi != nullptr || w == W));
  MVP_REQUIRE(mapping == nullptr || T >= 0);
  if (H >= (1ll << 31) || W >= (1ll << 31) || h >= (1ll << 31) || w >= (1ll << 31) || H * W >= (1ll << 31) || h * w >= (1ll << 31))
    return MVP_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int64_t f0 = 0; f0 < Nf; f0 += kMaxGridY) {
    const unsigned nf = (unsigned)(Nf - f0 < kMaxGridY ? Nf - f0 : kMaxGridY);
    hipLaunchKernelGGL(labels_kernel, dim3((unsigned)cdiv(h * w, kResizeThreads), nf), dim3(kResizeThreads), 0, s, labels, Ftot, (int)H, (int)W,
                       picked + f0, (int)h, (int)w, yi, xi, flip ? flip + f0 : nullptr, mapping, T, ignore_value,
                       out + (size_t)f0 * (size_t)(h * w));
  }
  return mvp_launch_status();
}

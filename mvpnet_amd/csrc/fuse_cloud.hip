// fuse_cloud.hip -- the scene cloud of an RGB-D recording, on the device for gfx950 (definition and table layout: include/mvp_hip.h):
//
//   fuse_insert_kernel : one lane per depth pixel: un-project (unproject_core.h, the bits of mvp_unproject_*), form the voxel key, find or
//                        claim the key's slot in an open-addressing table (64-bit compare-and-swap, linear probing) and add the pixel's
//                        fixed-point coordinates, its colour and 1 to the slot with INTEGER atomics.  Integer additions commute, so a
//                        voxel's state depends on the set of its pixels only -- not on the order of frames, launches, waves or lanes.
//   fuse_finish_kernel : one lane per surviving voxel (the caller lists the slots in ascending key order): mean point, mean colour,
//                        count, and the slot's row in `rank_of_slot`.
//   fuse_lookup_kernel : one lane per pixel of ANY frame: the same key, a read-only probe, the row of the pixel's voxel or -1.
//
// Replaces the offline mesh whose vertices the reference reads as `points` (mvpnet/data/preprocess/preprocess.py:204).
// No (F,h,w,3) tensor of world points is made.  Measurements: DESIGN.md (scene cloud from RGB-D).
#include "unproject_core.h"
#include <math.h>

namespace {

constexpr int kFuseThreads = 256;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int kIndexBias = 1 << 20;  // voxel indices lie in [-2^20, 2^20): 21 bits per axis

// the arrays of a table of `cap` slots (mvp_hip.h): key | sum[3] | csum[3] (with colours) | count | overflow
struct FuseTable {
  unsigned long long* key;
  unsigned long long* sum;   // int64 sums, added as two's complement
  unsigned long long* csum;  // nullptr without colours
  unsigned* count;
  unsigned* overflow;
};

__host__ __device__ inline FuseTable fuse_table(void* table, int64_t cap, bool colors) {
  FuseTable t;
  t.key = static_cast<unsigned long long*>(table);
  t.sum = t.key + cap;
  t.csum = colors ? t.sum + 3 * cap : nullptr;
  t.count = reinterpret_cast<unsigned*>(t.sum + (colors ? 6 : 3) * cap);
  t.overflow = t.count + cap;
  return t;
}

inline size_t fuse_table_bytes(int64_t cap, bool colors) {  // a multiple of 8
  return (size_t)cap * 8 * (colors ? 7 : 4) + (((size_t)cap * 4 + 8 + 7) & ~(size_t)7);
}

// first probe position: the 64-bit finalizer of MurmurHash3 over the key (neighbouring voxels differ in a few low bits of each field)
__device__ __forceinline__ unsigned fuse_home(unsigned long long k, unsigned mask) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned)k & mask;
}

// voxel index of one coordinate, biased into [0, 2^21); false when it falls outside (also for an infinite or NaN quotient)
__device__ __forceinline__ bool fuse_axis(float x, double voxel, unsigned long long& biased) {
  const double i = floor((double)x / voxel);  // a float64 division, correctly rounded: what NumPy computes
  if (!(i >= -(double)kIndexBias && i < (double)kIndexBias)) return false;
  biased = (unsigned long long)((int)i + kIndexBias);
  return true;
}

// The pixel `pix` of frame f: its float32 world point and voxel key; false for an invalid pixel.  f is uniform over the workgroup, so
// the camera's 21 floats are read once per wave.
template <typename DepthT>
__device__ __forceinline__ bool fuse_pixel(const DepthT* __restrict__ depth, const float* __restrict__ kinv, const float* __restrict__ pose,
                                           int f, int pix, int hw, int w, double voxel, float dmin, float dmax, float& x, float& y,
                                           float& z, unsigned long long& key) {
  const float d = depth_metres(depth, (size_t)f * hw + pix);
  if (!(d >= dmin && d <= dmax)) return false;  // (false for a NaN depth)
  const int v = pix / w, u = pix - v * w;
  const UnprojectCam cm = unproject_cam(kinv + (size_t)f * 9, pose + (size_t)f * 16);
  double xw, yw, zw, zc;
  unproject_pixel(cm, d, u, v, xw, yw, zw, zc);
  if (!(zc > 0.0)) return false;
  x = (float)xw;
  y = (float)yw;
  z = (float)zw;
  if (!(fabsf(x) < 32768.f && fabsf(y) < 32768.f && fabsf(z) < 32768.f)) return false;  // (false for inf and NaN)
  unsigned long long ix, iy, iz;
  if (!fuse_axis(x, voxel, ix) || !fuse_axis(y, voxel, iy) || !fuse_axis(z, voxel, iz)) return false;
  key = (iz << 42) | (iy << 21) | ix;
  return true;
}

// |x| < 32768, so the product is below 2^31 in magnitude and exact in float64; llrint rounds to nearest even (the default mode)
__device__ __forceinline__ unsigned long long fuse_fixed(float x) { return (unsigned long long)llrint((double)x * 65536.0); }

// One workgroup = kFuseThreads consecutive pixels of ONE frame (the last tile of a frame is partial).
template <typename DepthT>
__global__ __launch_bounds__(kFuseThreads) void fuse_insert_kernel(const DepthT* __restrict__ depth, const float* __restrict__ kinv,
                                                                   const float* __restrict__ pose, const uint8_t* __restrict__ images,
                                                                   int hw, int w, int tiles, double voxel, float dmin, float dmax,
                                                                   void* table, unsigned cap, int colors) {
  const int f = blockIdx.x / tiles;
  const int pix = (blockIdx.x - f * tiles) * kFuseThreads + threadIdx.x;
  if (pix >= hw) return;
  float x, y, z;
  unsigned long long key;
  if (!fuse_pixel(depth, kinv, pose, f, pix, hw, w, voxel, dmin, dmax, x, y, z, key)) return;
  const FuseTable t = fuse_table(table, cap, colors != 0);
  const unsigned mask = cap - 1u;
  unsigned slot = fuse_home(key, mask);
  bool found = false;
  for (unsigned step = 0; step < cap; ++step) {  // at most one pass over the table; no lane waits for another
    // a key, once written, never changes: a plain read that sees this key or another one is final, only `empty` needs the swap
    unsigned long long k = __atomic_load_n(&t.key[slot], __ATOMIC_RELAXED);
    if (k == kEmptyKey) k = atomicCAS(&t.key[slot], kEmptyKey, key);
    if (k == kEmptyKey || k == key) {
      found = true;
      break;
    }
    slot = (slot + 1u) & mask;
  }
  if (!found) {  // a full table: the pixel is dropped and the caller is told (CloudFuser.finish raises)
    atomicOr(t.overflow, 1u);
    return;
  }
  atomicAdd(&t.count[slot], 1u);
  atomicAdd(&t.sum[(size_t)slot * 3 + 0], fuse_fixed(x));
  atomicAdd(&t.sum[(size_t)slot * 3 + 1], fuse_fixed(y));
  atomicAdd(&t.sum[(size_t)slot * 3 + 2], fuse_fixed(z));
  if (images != nullptr) {
    const uint8_t* rgb = images + ((size_t)f * hw + pix) * 3;
    atomicAdd(&t.csum[(size_t)slot * 3 + 0], (unsigned long long)rgb[0]);
    atomicAdd(&t.csum[(size_t)slot * 3 + 1], (unsigned long long)rgb[1]);
    atomicAdd(&t.csum[(size_t)slot * 3 + 2], (unsigned long long)rgb[2]);
  }
}

__global__ __launch_bounds__(kFuseThreads) void fuse_finish_kernel(const void* table, unsigned cap, int colors,
                                                                   const int64_t* __restrict__ slots, int n, float* __restrict__ points,
                                                                   uint8_t* __restrict__ colors_out, int32_t* __restrict__ counts,
                                                                   int32_t* __restrict__ rank_of_slot) {
  const int r = blockIdx.x * kFuseThreads + threadIdx.x;
  if (r >= n) return;
  const int64_t slot = slots[r];
  if (slot < 0 || slot >= (int64_t)cap) return;  // not a slot of this table: the row stays as the caller left it
  const FuseTable t = fuse_table(const_cast<void*>(table), cap, colors != 0);
  const unsigned c = t.count[slot];
  const double dc = (double)c;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s = (double)(long long)t.sum[(size_t)slot * 3 + a];
    points[(size_t)r * 3 + a] = (float)(s / dc * (1.0 / 65536.0));
  }
  if (colors_out != nullptr) {
    const unsigned long long c2 = 2ull * c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned long long s = t.csum[(size_t)slot * 3 + a];
      colors_out[(size_t)r * 3 + a] = c ? (uint8_t)((2ull * s + c) / c2) : (uint8_t)0;
    }
  }
  counts[r] = (int32_t)c;
  rank_of_slot[slot] = r;
}

template <typename DepthT>
__global__ __launch_bounds__(kFuseThreads) void fuse_lookup_kernel(const DepthT* __restrict__ depth, const float* __restrict__ kinv,
                                                                   const float* __restrict__ pose, int hw, int w, int tiles, double voxel,
                                                                   float dmin, float dmax, const unsigned long long* __restrict__ keys,
                                                                   unsigned cap, const int32_t* __restrict__ rank_of_slot,
                                                                   int32_t* __restrict__ pixel_point) {
  const int f = blockIdx.x / tiles;
  const int pix = (blockIdx.x - f * tiles) * kFuseThreads + threadIdx.x;
  if (pix >= hw) return;
  float x, y, z;
  unsigned long long key;
  int32_t rank = -1;
  if (fuse_pixel(depth, kinv, pose, f, pix, hw, w, voxel, dmin, dmax, x, y, z, key)) {
    const unsigned mask = cap - 1u;
    unsigned slot = fuse_home(key, mask);
    for (unsigned step = 0; step < cap; ++step) {
      const unsigned long long k = keys[slot];
      if (k == key) {
        rank = rank_of_slot[slot];
        break;
      }
      if (k == kEmptyKey) break;
      slot = (slot + 1u) & mask;
    }
  }
  pixel_point[(size_t)f * hw + pix] = rank;
}

inline bool fuse_pow2(int64_t c) { return c >= 1 && (c & (c - 1)) == 0; }

// the checks that insert and lookup share, after their pointers
inline int fuse_frames_check(int64_t F, int64_t h, int64_t w, double voxel, float dmin, float dmax, int64_t cap) {
  MVP_REQUIRE(F >= 0 && h >= 1 && w >= 1);
  MVP_REQUIRE(isfinite(voxel) && voxel > 0.0);
  MVP_REQUIRE(!isnan(dmin) && !isnan(dmax));
  MVP_REQUIRE(fuse_pow2(cap));
  if (cap >= (1ll << 31)) return MVP_EUNSUPPORTED;
  // each factor is bounded before it enters a product: no int64 product here can overflow
  if (F >= (1ll << 31) || h >= (1ll << 31) || w >= (1ll << 31) || h * w >= (1ll << 31) || F * (h * w) >= (1ll << 31)) return MVP_EUNSUPPORTED;
  return MVP_OK;
}

template <typename DepthT>
int fuse_insert_entry(const DepthT* depth, const float* kinv, const float* pose, const uint8_t* images, int64_t F, int64_t h, int64_t w,
                      double voxel, float dmin, float dmax, void* table, int64_t cap, int colors, mvp_stream_t stream) {
  MVP_NONNULL(depth);
  MVP_NONNULL(kinv);
  MVP_NONNULL(pose);
  MVP_NONNULL(table);
  const int st = fuse_frames_check(F, h, w, voxel, dmin, dmax, cap);
  if (st != MVP_OK) return st;
  MVP_REQUIRE(images == nullptr || colors != 0);
  if (F == 0) return MVP_OK;
  const int hw = (int)(h * w);
  const int tiles = (int)cdiv(hw, kFuseThreads);  // F * tiles <= F * hw < 2^31
  hipLaunchKernelGGL(fuse_insert_kernel<DepthT>, dim3((unsigned)(F * tiles)), dim3(kFuseThreads), 0, static_cast<hipStream_t>(stream), depth,
                     kinv, pose, images, hw, (int)w, tiles, voxel, dmin, dmax, table, (unsigned)cap, colors);
  return mvp_launch_status();
}

template <typename DepthT>
int fuse_lookup_entry(const DepthT* depth, const float* kinv, const float* pose, int64_t F, int64_t h, int64_t w, double voxel, float dmin,
                      float dmax, const void* table, int64_t cap, const int32_t* rank_of_slot, int32_t* pixel_point, mvp_stream_t stream) {
  MVP_NONNULL(depth);
  MVP_NONNULL(kinv);
  MVP_NONNULL(pose);
  MVP_NONNULL(table);
  MVP_NONNULL(rank_of_slot);
  MVP_NONNULL(pixel_point);
  const int st = fuse_frames_check(F, h, w, voxel, dmin, dmax, cap);
  if (st != MVP_OK) return st;
  if (F == 0) return MVP_OK;
  const int hw = (int)(h * w);
  const int tiles = (int)cdiv(hw, kFuseThreads);
  hipLaunchKernelGGL(fuse_lookup_kernel<DepthT>, dim3((unsigned)(F * tiles)), dim3(kFuseThreads), 0, static_cast<hipStream_t>(stream), depth,
                     kinv, pose, hw, (int)w, tiles, voxel, dmin, dmax, static_cast<const unsigned long long*>(table), (unsigned)cap,
                     rank_of_slot, pixel_point);
  return mvp_launch_status();
}

}  // namespace

MVP_API size_t mvp_fuse_cloud_table_bytes(int64_t capacity, int colors) {
  if (!fuse_pow2(capacity) || capacity >= (1ll << 31)) return 0;
  return fuse_table_bytes(capacity, colors != 0);
}

MVP_API int mvp_fuse_cloud_insert_f32(const float* depth_m, const float* kinv, const float* pose, const uint8_t* images, int64_t F, int64_t h,
                                      int64_t w, double voxel, float depth_min, float depth_max, void* table, int64_t capacity, int colors,
                                      mvp_stream_t stream) {
  return fuse_insert_entry<float>(depth_m, kinv, pose, images, F, h, w, voxel, depth_min, depth_max, table, capacity, colors, stream);
}
MVP_API int mvp_fuse_cloud_insert_u16(const uint16_t* depth_mm, const float* kinv, const float* pose, const uint8_t* images, int64_t F,
                                      int64_t h, int64_t w, double voxel, float depth_min, float depth_max, void* table, int64_t capacity,
                                      int colors, mvp_stream_t stream) {
  return fuse_insert_entry<uint16_t>(depth_mm, kinv, pose, images, F, h, w, voxel, depth_min, depth_max, table, capacity, colors, stream);
}

MVP_API int mvp_fuse_cloud_finish(const void* table, int64_t capacity, int colors, const int64_t* slots, int64_t n, float* points,
                                  uint8_t* colors_out, int32_t* counts, int32_t* rank_of_slot, mvp_stream_t stream) {
  MVP_NONNULL(table);
  MVP_NONNULL(slots);
  MVP_NONNULL(points);
  MVP_NONNULL(counts);
  MVP_NONNULL(rank_of_slot);
  MVP_REQUIRE(fuse_pow2(capacity));
  if (capacity >= (1ll << 31)) return MVP_EUNSUPPORTED;
  MVP_REQUIRE(n >= 0 && n <= capacity);
  MVP_REQUIRE(colors_out == nullptr || colors != 0);
  if (n == 0) return MVP_OK;
  hipLaunchKernelGGL(fuse_finish_kernel, dim3((unsigned)cdiv(n, kFuseThreads)), dim3(kFuseThreads), 0, static_cast<hipStream_t>(stream), table,
                     (unsigned)capacity, colors, slots, (int)n, points, colors_out, counts, rank_of_slot);
  return mvp_launch_status();
}

MVP_API int mvp_fuse_cloud_lookup_f32(const float* depth_m, const float* kinv, const float* pose, int64_t F, int64_t h, int64_t w, double voxel,
                                      float depth_min, float depth_max, const void* table, int64_t capacity, const int32_t* rank_of_slot,
                                      int32_t* pixel_point, mvp_stream_t stream) {
  return fuse_lookup_entry<float>(depth_m, kinv, pose, F, h, w, voxel, depth_min, depth_max, table, capacity, rank_of_slot, pixel_point, stream);
}
MVP_API int mvp_fuse_cloud_lookup_u16(const uint16_t* depth_mm, const float* kinv, const float* pose, int64_t F, int64_t h, int64_t w,
                                      double voxel, float depth_min, float depth_max, const void* table, int64_t capacity,
                                      const int32_t* rank_of_slot, int32_t* pixel_point, mvp_stream_t stream) {
  return fuse_lookup_entry<uint16_t>(depth_mm, kinv, pose, F, h, w, voxel, depth_min, depth_max, table, capacity, rank_of_slot, pixel_point,
                                     stream);
}

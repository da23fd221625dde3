// chunker.hip -- the sliding-window chunker of a whole scene and the packing of its (ragged) chunks into padded batches, for gfx950:
// scene2chunks_legacy (mvpnet/utils/chunk_util.py:4-53) without the (windows x points) membership matrices, and the sparse-chunk rule of
// mvpnet/test_mvpnet_3d.py:146-154 for all chunks of a scene in one launch.  Definitions: include/mvp_hip.h (mvp_scene_chunks_*,
// mvp_pack_chunks_f32, mvp_pack_cloud_f32).
//
//   chunks_count_kernel : one workgroup per window walks all points once; per thread two integer counters (inner / outer test), one
//                         reduction at the end -- integers, no atomics.
//   chunks_fill_kernel  : one workgroup per KEPT window walks the points in tiles of kTile = kUnroll x kChkThreads; a point's place in
//                         the list is running base + (members in the sub-tiles and waves before its own) + (members among the lower
//                         lanes of its wave's ballot): ascending point index by construction, no atomics, no scan across workgroups
//                         (the pattern of sample.hip's select_kernel<0> and of ball_query.hip).  The z extent rides along; the
//                         base-point bits are chunk_common.h's write_base_bits.
//   chunks_pack_kernel  : slot s of chunk c -> a member (chunk_common.h's pad rule) -> three coordinates.
//   chunks_pack_cloud_kernel : the same slot -> member rule, computed once per slot, -> three coordinates and the point's feature row
//                         (colours / 255 or float channels): the 3D baselines' (B,3,N) + (B,Cf,N) batches.
// Every window re-reads the scene (12 bytes x n, out of L2 after the first): a per-point scatter into its windows would read less but
// needs a stable multi-split.
#include "chunk_common.h"
#include <math.h>

namespace {

constexpr int kChkThreads = 256;
constexpr int kChkWaves = kChkThreads / kWave;
constexpr int kUnroll = 4;  // points per thread and tile: four loads in flight per barrier
constexpr int kTile = kUnroll * kChkThreads;

struct Window {  // float32 corners are exact in double, so the tests below compare in double wherever the rule says so
  float lo_x, lo_y;                // inner, lower side: float32 compare
  double in_hx, in_hy;             // (double)lo + size
  double out_lx, out_ly, out_hx, out_hy;  // (double)lo - margin, ((double)lo + size) + margin
};

__device__ __forceinline__ Window window_of(const float* __restrict__ corners, int w, double sx, double sy, double mx, double my) {
  Window b;
  b.lo_x = corners[(size_t)w * 2 + 0];
  b.lo_y = corners[(size_t)w * 2 + 1];
  b.in_hx = (double)b.lo_x + sx;
  b.in_hy = (double)b.lo_y + sy;
  b.out_lx = (double)b.lo_x - mx;
  b.out_ly = (double)b.lo_y - my;
  b.out_hx = b.in_hx + mx;
  b.out_hy = b.in_hy + my;
  return b;
}

// (every comparison is false for a NaN coordinate)
__device__ __forceinline__ bool inner_test(const Window& b, float x, float y) {
  return x >= b.lo_x && y >= b.lo_y && (double)x <= b.in_hx && (double)y <= b.in_hy;
}
__device__ __forceinline__ bool outer_test(const Window& b, float x, float y) {
  const double xd = x, yd = y;
  return xd >= b.out_lx && xd <= b.out_hx && yd >= b.out_ly && yd <= b.out_hy;
}

__global__ __launch_bounds__(kChkThreads) void chunks_count_kernel(const float* __restrict__ points, int n,
                                                                   const float* __restrict__ corners, double sx, double sy, double mx,
                                                                   double my, int32_t* __restrict__ inner_count,
                                                                   int32_t* __restrict__ outer_count) {
  __shared__ int s_in[kChkWaves], s_out[kChkWaves];
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const Window b = window_of(corners, w, sx, sy, mx, my);
  int ci = 0, co = 0;
  for (int64_t base = 0; base < n; base += kTile) {
    float x[kUnroll], y[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t j = base + u * kChkThreads + tid;
      x[u] = y[u] = NAN;
      if (j < n) {
        x[u] = points[j * 3 + 0];
        y[u] = points[j * 3 + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      ci += inner_test(b, x[u], y[u]) ? 1 : 0;
      co += outer_test(b, x[u], y[u]) ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = kWave / 2; k >= 1; k >>= 1) {
    ci += __shfl_xor(ci, k, kWave);
    co += __shfl_xor(co, k, kWave);
  }
  if (lane == 0) {
    s_in[wave] = ci;
    s_out[wave] = co;
  }
  __syncthreads();
  if (tid == 0) {
    int a = 0, o = 0;
#pragma unroll
    for (int v = 0; v < kChkWaves; ++v) {
      a += s_in[v];
      o += s_out[v];
    }
    inner_count[w] = a;
    outer_count[w] = o;
  }
}

struct FillArgs {
  const float* points;
  const float* corners;
  const int32_t* kept;
  const int64_t* offsets;
  const int64_t* base_point_ind;
  int64_t* index;
  float* zbox;
  uint32_t* base_bits;
  double sx, sy, mx, my;
  int64_t total;
  int n, nc, nb;
};

__global__ __launch_bounds__(kChkThreads) void chunks_fill_kernel(FillArgs a) {
  __shared__ int s_tot[2][kUnroll][kChkWaves];
  __shared__ float s_z[kChkWaves][2];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const Window b = window_of(a.corners, (int)clamp_index(a.kept[c], a.nc), a.sx, a.sy, a.mx, a.my);
  // the chunk's slice of `index`, cut to the array: a list longer than its slice loses its tail, nothing is written outside
  int64_t off = a.offsets[c], end = a.offsets[c + 1];
  clamp_slice(off, end, a.total);
  const int64_t cap = end - off;
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t run = 0;
  float zlo = INFINITY, zhi = -INFINITY;
  int par = 0;
  for (int64_t base = 0; base < a.n; base += kTile, par ^= 1) {  // uniform over the workgroup: every lane takes part in the ballots
    float x[kUnroll], y[kUnroll], z[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t j = base + u * kChkThreads + tid;
      x[u] = y[u] = NAN;
      z[u] = 0.f;
      if (j < a.n) {
        x[u] = a.points[j * 3 + 0];
        y[u] = a.points[j * 3 + 1];
        z[u] = a.points[j * 3 + 2];
      }
    }
    bool in[kUnroll];
    int before[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      in[u] = outer_test(b, x[u], y[u]);
      const unsigned long long bal = __ballot(in[u]);
      before[u] = __popcll(bal & below);
      if (lane == 0) s_tot[par][u][wave] = __popcll(bal);
      if (in[u]) {
        zlo = nan_min(zlo, z[u]);
        zhi = nan_max(zhi, z[u]);
      }
    }
    __syncthreads();  // one barrier per tile: the next tile writes the other half of s_tot
    int ahead = 0;    // members of this tile in front of (sub-tile u, this wave)
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      int mine = ahead;
#pragma unroll
      for (int v = 0; v < kChkWaves; ++v) {
        const int t = s_tot[par][u][v];
        mine += v < wave ? t : 0;
        ahead += t;
      }
      const int64_t pos = run + mine + before[u];
      if (in[u] && pos < cap) a.index[off + pos] = base + u * kChkThreads + tid;
    }
    run += ahead;
  }
#pragma unroll
  for (int k = kWave / 2; k >= 1; k >>= 1) {
    zlo = nan_min(zlo, __shfl_xor(zlo, k, kWave));
    zhi = nan_max(zhi, __shfl_xor(zhi, k, kWave));
  }
  if (lane == 0) {
    s_z[wave][0] = zlo;
    s_z[wave][1] = zhi;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int v = 1; v < kChkWaves; ++v) {
      zlo = nan_min(zlo, s_z[v][0]);
      zhi = nan_max(zhi, s_z[v][1]);
    }
    a.zbox[(size_t)c * 2 + 0] = zlo;
    a.zbox[(size_t)c * 2 + 1] = zhi;
  }
  if (a.nb > 0)  // bit j: base point j is a member
    write_base_bits<kChkThreads>(a.base_bits + (size_t)c * ((a.nb + 31) >> 5), a.nb, [&](int j) {
      const int64_t p = clamp_index(a.base_point_ind[j], a.n);
      return outer_test(b, a.points[p * 3 + 0], a.points[p * 3 + 1]);
    });
}

__global__ __launch_bounds__(kChkThreads) void chunks_pack_kernel(const float* __restrict__ points, int64_t n,
                                                                  const int64_t* __restrict__ index, int64_t total,
                                                                  const int64_t* __restrict__ offsets,
                                                                  const int64_t* __restrict__ out_base,
                                                                  const int64_t* __restrict__ out_len, uint32_t seed32, int64_t out_floats,
                                                                  float* __restrict__ out) {
  const int c = blockIdx.y;
  int64_t off = offsets[c], end = offsets[c + 1];
  clamp_slice(off, end, total);
  const int64_t nc = end - off, N = out_len[c], ob = out_base[c];
  // the chunk's (3, N) rows lie inside `out`, or nothing of it is written
  if (N <= 0 || nc <= 0 || nc >= (1ll << 32) || ob < 0 || ob > out_floats || 3 * N > out_floats - ob) return;
  const uint32_t sc = chunk_seed(seed32, c);
  for (int64_t s = (int64_t)blockIdx.x * kChkThreads + threadIdx.x; s < N; s += (int64_t)gridDim.x * kChkThreads) {
    const int64_t p = clamp_index(index[off + pad_member(s, nc, sc)], n);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[ob + k * N + s] = points[p * 3 + k];
  }
}

// chunks_pack_kernel with the chunks placed in SLOTS and a per-point feature beside the coordinates: the member of a slot is computed once
// and both rows are read through it.  kColors: (n,3) uint8 written as c / 255 (mvp_gather_cloud_f32's expression); else (n,Cf) float32 rows
// copied as they are; Cf = 0: coordinates only.
struct PackCloudArgs {
  const float* points;
  const uint8_t* colors;
  const float* feature;
  const int64_t* index;
  const int64_t* offsets;
  const int64_t* slot_base;
  const int64_t* out_len;
  float* out_points;
  float* out_feature;
  int64_t n, total, out_slots;
  uint32_t seed32;
  int Cf;
};

template <bool kColors>
__global__ __launch_bounds__(kChkThreads) void chunks_pack_cloud_kernel(PackCloudArgs a) {
  const int c = blockIdx.y;
  int64_t off = a.offsets[c], end = a.offsets[c + 1];
  clamp_slice(off, end, a.total);
  const int64_t nc = end - off, N = a.out_len[c], sb = a.slot_base[c];
  // the chunk's N slots lie inside the buffers, or nothing of it is written
  if (N <= 0 || nc <= 0 || nc >= (1ll << 32) || sb < 0 || sb > a.out_slots || N > a.out_slots - sb) return;
  const uint32_t sc = chunk_seed(a.seed32, c);
  float* __restrict__ op = a.out_points + 3 * sb;
  float* __restrict__ of = a.out_feature + (int64_t)a.Cf * sb;
  for (int64_t s = (int64_t)blockIdx.x * kChkThreads + threadIdx.x; s < N; s += (int64_t)gridDim.x * kChkThreads) {
    const int64_t p = clamp_index(a.index[off + pad_member(s, nc, sc)], a.n);
#pragma unroll
    for (int k = 0; k < 3; ++k) op[k * N + s] = a.points[p * 3 + k];
    if (kColors) {
#pragma unroll
      for (int k = 0; k < 3; ++k) of[k * N + s] = (float)a.colors[p * 3 + k] / 255.0f;  // IEEE division
    } else {
      for (int k = 0; k < a.Cf; ++k) of[k * N + s] = a.feature[p * a.Cf + k];
    }
  }
}

inline bool chunker_shape_ok(int64_t n, int64_t nc, int64_t nb) {
  return n < (1ll << 31) && nc <= MVP_CHUNKER_MAX_WINDOWS && nb <= MVP_OVERLAP_MAX_BASE;
}

inline bool finite4(double a, double b, double c, double d) { return a == a && b == b && c == c && d == d; }

}  // namespace

MVP_API int mvp_scene_chunks_count_f32(const float* points, int64_t n, const float* corners, int64_t nc, double size_x, double size_y,
                                       double margin_x, double margin_y, int32_t* inner_count, int32_t* outer_count, mvp_stream_t stream) {
  MVP_NONNULL(points);
  MVP_NONNULL(corners);
  MVP_NONNULL(inner_count);
  MVP_NONNULL(outer_count);
  MVP_REQUIRE(n >= 1 && nc >= 1 && finite4(size_x, size_y, margin_x, margin_y));
  if (!chunker_shape_ok(n, nc, 0)) return MVP_EUNSUPPORTED;
  hipLaunchKernelGGL(chunks_count_kernel, dim3((unsigned)nc), dim3(kChkThreads), 0, static_cast<hipStream_t>(stream), points, (int)n, corners, size_x,
                     size_y, margin_x, margin_y, inner_count, outer_count);
  return mvp_launch_status();
}

MVP_API int mvp_scene_chunks_fill_f32(const float* points, int64_t n, const float* corners, int64_t nc, double size_x, double size_y,
                                      double margin_x, double margin_y, const int32_t* kept, const int64_t* offsets, int64_t C,
                                      const int64_t* base_point_ind, int64_t nb, int64_t* index, int64_t total, float* zbox,
                                      uint32_t* base_bits, mvp_stream_t stream) {
  MVP_NONNULL(points);
  MVP_NONNULL(corners);
  MVP_NONNULL(kept);
  MVP_NONNULL(offsets);
  MVP_NONNULL(zbox);
  MVP_REQUIRE(n >= 1 && nc >= 1 && C >= 0 && nb >= 0 && total >= 0 && finite4(size_x, size_y, margin_x, margin_y));
  if (total > 0) MVP_NONNULL(index);
  if (nb > 0) {
    MVP_NONNULL(base_point_ind);
    MVP_NONNULL(base_bits);
  }
  if (!chunker_shape_ok(n, nc, nb) || C > MVP_CHUNKER_MAX_WINDOWS) return MVP_EUNSUPPORTED;
  if (C == 0) return MVP_OK;
  FillArgs a;
  a.points = points, a.corners = corners, a.kept = kept, a.offsets = offsets, a.base_point_ind = base_point_ind, a.index = index;
  a.zbox = zbox, a.base_bits = base_bits, a.sx = size_x, a.sy = size_y, a.mx = margin_x, a.my = margin_y, a.total = total;
  a.n = (int)n, a.nc = (int)nc, a.nb = (int)nb;
  hipLaunchKernelGGL(chunks_fill_kernel, dim3((unsigned)C), dim3(kChkThreads), 0, static_cast<hipStream_t>(stream), a);
  return mvp_launch_status();
}

MVP_API int mvp_pack_chunks_f32(const float* points, int64_t n, const int64_t* index, int64_t total, const int64_t* offsets, int64_t C,
                                const int64_t* out_base, const int64_t* out_len, const int64_t* host_lengths, const int64_t* host_out_len,
                                uint64_t seed, float* out, int64_t out_floats, mvp_stream_t stream) {
  MVP_NONNULL(points);
  MVP_NONNULL(index);
  MVP_NONNULL(offsets);
  MVP_NONNULL(out_base);
  MVP_NONNULL(out_len);
  MVP_NONNULL(host_lengths);
  MVP_NONNULL(host_out_len);
  MVP_NONNULL(out);
  MVP_REQUIRE(n >= 1 && total >= 1 && C >= 0 && out_floats >= 0);
  int64_t widest = 0;
  for (int64_t c = 0; c < C; ++c) {
    MVP_REQUIRE(host_lengths[c] >= 1 && host_out_len[c] >= host_lengths[c]);
    widest = host_out_len[c] > widest ? host_out_len[c] : widest;
  }
  if (n >= (1ll << 31) || C > MVP_CHUNKER_MAX_WINDOWS || widest >= (1ll << 31)) return MVP_EUNSUPPORTED;
  if (C == 0) return MVP_OK;
  const int64_t gx = cdiv(widest, kChkThreads);
  const uint32_t seed32 = (uint32_t)(seed ^ (seed >> 32));
  hipLaunchKernelGGL(chunks_pack_kernel, dim3((unsigned)(gx > 1024 ? 1024 : gx), (unsigned)C), dim3(kChkThreads), 0, static_cast<hipStream_t>(stream),
                     points, n, index, total, offsets, out_base, out_len, seed32, out_floats, out);
  return mvp_launch_status();
}

MVP_API int mvp_pack_cloud_f32(const float* points, const uint8_t* colors, const float* feature, int64_t Cf, int64_t n, const int64_t* index,
                               int64_t total, const int64_t* offsets, int64_t C, const int64_t* slot_base, const int64_t* out_len,
                               const int64_t* host_lengths, const int64_t* host_out_len, uint64_t seed, float* out_points, float* out_feature,
                               int64_t out_slots, mvp_stream_t stream) {
  MVP_NONNULL(points);
  MVP_NONNULL(index);
  MVP_NONNULL(offsets);
  MVP_NONNULL(slot_base);
  MVP_NONNULL(out_len);
  MVP_NONNULL(host_lengths);
  MVP_NONNULL(host_out_len);
  MVP_NONNULL(out_points);
  const bool has_feature = colors != nullptr || feature != nullptr;
  if (has_feature) MVP_NONNULL(out_feature);
  MVP_REQUIRE(n >= 1 && total >= 1 && C >= 0 && out_slots >= 0 && !(colors != nullptr && feature != nullptr));
  MVP_REQUIRE(!has_feature || (colors != nullptr ? Cf == 3 : Cf >= 1));
  int64_t widest = 0;
  for (int64_t c = 0; c < C; ++c) {
    MVP_REQUIRE(host_lengths[c] >= 1 && host_out_len[c] >= host_lengths[c]);
    widest = host_out_len[c] > widest ? host_out_len[c] : widest;
  }
  if (n >= (1ll << 31) || C > MVP_CHUNKER_MAX_WINDOWS || widest >= (1ll << 31) || (has_feature && Cf > MVP_PACK_CLOUD_MAX_CHANNELS))
    return MVP_EUNSUPPORTED;
  if (C == 0) return MVP_OK;
  PackCloudArgs a;
  a.points = points, a.colors = colors, a.feature = feature, a.index = index, a.offsets = offsets, a.slot_base = slot_base, a.out_len = out_len;
  a.out_points = out_points, a.out_feature = out_feature, a.n = n, a.total = total, a.out_slots = out_slots;
  a.seed32 = (uint32_t)(seed ^ (seed >> 32)), a.Cf = has_feature ? (int)Cf : 0;
  const int64_t gx = cdiv(widest, kChkThreads);
  const dim3 grid((unsigned)(gx > 1024 ? 1024 : gx), (unsigned)C), block(kChkThreads);
  if (colors != nullptr)
    hipLaunchKernelGGL(chunks_pack_cloud_kernel<true>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(chunks_pack_cloud_kernel<false>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return mvp_launch_status();
}

// scene_sample.hip -- the 3D baselines' training batch drawn on the device for gfx950: `CropPad(nb_pts)` of B whole resident scenes
// (mvpnet/data/transforms.py:112-133 behind ScanNet3DScene.__getitem__, mvpnet/data/scannet_3d.py:206-221; nb_pts up to 65536 of up to
// 2^31 points per row) and the gather that turns a `choice` -- this call's or mvp_sample_chunks_f32's -- into what PN2SSG reads: rotated
// points, labels, `colors / 255` (transforms.py:64-85, scannet_3d.py:82).  Definitions: include/mvp_hip.h (mvp_sample_scenes_f32,
// mvp_gather_cloud_f32).
//
// The draw is the resampling rule of mvp_sample_chunks_f32 with every point of the scene a member, so no pass reads a coordinate: a
// point's key is a hash of its index.  A scene is cut into G segments of `seg` consecutive points, one workgroup each:
//   scene_init_kernel    : per row the scene's slice, s_b, pad or crop; zeroes the row's histograms.
//   scene_hist_kernel<P> / scene_digit_kernel<P> : radix select of the nb_pts-th smallest key, 8 + 12 + 12 bits.
//   scene_collect_kernel : the nb_pts points with key <= that key as (key, index) pairs, in any order (one returning atomic per wave).
//   scene_tile_kernel    : tiles of 8192 pairs sorted in 64 KiB of LDS (bitonic), in place; a pad row writes its choice here and is done.
//   scene_merge_kernel   : sorted runs of L pairs merged two by two in global memory, L = 8192, 16384, 32768: a pair's place is its rank
//                          in its own run + its rank in the sibling run (binary search; the keys are distinct).  Whatever the hash does
//                          with the keys, the work is the same; the last pass writes `choice`.
// Pad rows (n < nb_pts) skip the select, the collect, the sort and the merges.  The state, the keys, the select, the collect and the tile
// sort are keyed_select.h's, shared with sample.hip; this file adds the merges.  Measurements: DESIGN.md (3D-baseline batches).
#include "keyed_select.h"

namespace {

constexpr int kScnThreads = kSelThreads;
constexpr int kScnMaxSeg = 256;  // workgroups per row and pass
constexpr int kScnMaxPts = MVP_SAMPLE_SCENE_MAX_PTS;
constexpr int kTile = 8192;  // (key, index) pairs sorted in LDS by one workgroup = 64 KiB
constexpr int kTileThreads = 1024;

typedef SelectState RowState;  // per row, written by scene_init_kernel; crop: n >= nb_pts

__global__ __launch_bounds__(kScnThreads) void scene_init_kernel(const int64_t* __restrict__ scene_offsets, const int64_t* __restrict__ scene_of_row,
                                                                 const int64_t* __restrict__ seed_device, uint64_t seed, int S, int64_t Ntot,
                                                                 int G, int nb_pts, RowState* __restrict__ state,
                                                                 uint32_t* __restrict__ hist_all, int32_t* __restrict__ num_points) {
  const int b = blockIdx.x;
  zero_hist(hist_all, b);
  if (threadIdx.x != 0) return;
  const Slice sc = scene_slice(scene_offsets, scene_of_row, b, S, Ntot, G);
  RowState st;
  select_init(st, sc, sc.n, nb_pts, seed_device, seed, b);
  state[b] = st;
  num_points[b] = st.n;
}

// every point of the scene is a member, so no pass reads a coordinate
template <int PASS>
__global__ __launch_bounds__(kScnThreads) void scene_hist_kernel(const RowState* __restrict__ state, uint32_t* __restrict__ hist_all) {
  __shared__ uint32_t s_hist[kBins0];
  const int b = blockIdx.y;
  const RowState st = state[b];
  if (!st.crop) return;
  int64_t begin, end;
  segment_range(st, blockIdx.x, begin, end);
  if (begin >= end) return;
  uint32_t* hist = hist_all + (size_t)b * kHistWords;
  hist_begin<PASS>(s_hist);
  for (int64_t j = begin + threadIdx.x; j < end; j += kScnThreads) hist_key<PASS>(select_key(j, st.sb), st.prefix, s_hist, hist);
  hist_end<PASS>(s_hist, hist);
}

template <int PASS>
__global__ __launch_bounds__(kScnThreads) void scene_digit_kernel(RowState* __restrict__ state, const uint32_t* __restrict__ hist_all) {
  digit_search<PASS>(state, hist_all);
}

__global__ __launch_bounds__(kScnThreads) void scene_collect_kernel(RowState* __restrict__ state, int nb_pts,
                                                                    unsigned long long* __restrict__ pairs) {
  collect_pairs(state, nb_pts, pairs, [](const RowState&, int64_t) { return true; });
}

// tile t of row b: slots [t * kTile, t * kTile + cnt).  Crop rows: the tile's pairs sorted in place (`direct`: nb_pts <= kTile, the one
// tile is the result).  Pad rows: the pad rule.
__global__ __launch_bounds__(kTileThreads) void scene_tile_kernel(const RowState* __restrict__ state, unsigned long long* __restrict__ pairs,
                                                                  int nb_pts, int direct, int64_t* __restrict__ choice) {
  extern __shared__ __attribute__((aligned(16))) unsigned char scene_smem[];
  unsigned long long* buf = reinterpret_cast<unsigned long long*>(scene_smem);  // the tile's pairs, padded to a power of two
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const RowState st = state[b];
  const int lo = t * kTile;
  const int cnt = nb_pts - lo < kTile ? nb_pts - lo : kTile;
  if (!st.crop) {
    for (int i = tid; i < cnt; i += kTileThreads)
      choice[(size_t)b * nb_pts + lo + i] = st.n <= 0 ? 0 : pad_member(lo + i, st.n, st.sb);
    return;
  }
  unsigned long long* row = pairs + (size_t)b * nb_pts + lo;
  int P = 1;
  while (P < cnt) P <<= 1;
  bitonic_sort_lds<kTileThreads>(buf, row, cnt, P);
  for (int i = tid; i < cnt; i += kTileThreads) {
    if (direct) {
      choice[(size_t)b * nb_pts + lo + i] = choice_of(buf[i], st.n);
    } else {
      row[i] = buf[i];
    }
  }
}

// One merge pass: `src` holds sorted runs of L pairs (the last one shorter or missing); runs 2k and 2k+1 become one run of `dst`.  The pairs
// are distinct, so a pair's place is its position in its own run + the number of smaller pairs in the sibling run.  Whatever `src` holds,
// the place stays inside the two runs' slots.
__global__ __launch_bounds__(kScnThreads) void scene_merge_kernel(const RowState* __restrict__ state, const unsigned long long* __restrict__ src,
                                                                  int nb_pts, int L, int last, unsigned long long* __restrict__ dst,
                                                                  int64_t* __restrict__ choice) {
  const int b = blockIdx.y, i = blockIdx.x * kScnThreads + threadIdx.x;
  const RowState st = state[b];
  if (!st.crop || i >= nb_pts) return;
  const unsigned long long* row = src + (size_t)b * nb_pts;
  const unsigned long long x = row[i];
  const int r = i / L, own = r * L, base = (r & ~1) * L;
  int plo = (r ^ 1) * L;
  plo = plo < nb_pts ? plo : nb_pts;
  const int phi = plo + L < nb_pts ? plo + L : nb_pts;
  int lo = plo, hi = phi;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row[mid] < x) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  const int pos = base + (i - own) + (lo - plo);
  if (last) {
    choice[(size_t)b * nb_pts + pos] = choice_of(x, st.n);
  } else {
    dst[(size_t)b * nb_pts + pos] = x;
  }
}

inline int scene_segments(int64_t Ntot) { return segments(Ntot, 4 * kScnThreads, kScnMaxSeg); }

struct SceneLayout {
  size_t state, hist, pairs, pairs2, total;
};
inline SceneLayout scene_layout(int64_t B, int64_t nb_pts) {
  SceneLayout l;
  size_t at = 0;
  l.state = at, at = align16(at + sizeof(RowState) * (size_t)B);
  l.hist = at, at = align16(at + sizeof(uint32_t) * (size_t)B * kHistWords);
  l.pairs = at, at = align16(at + sizeof(unsigned long long) * (size_t)B * (size_t)nb_pts);
  l.pairs2 = at, at = align16(at + (nb_pts > kTile ? sizeof(unsigned long long) * (size_t)B * (size_t)nb_pts : 0));
  l.total = at;
  return l;
}

inline bool scene_shape_ok(int64_t Ntot, int64_t B, int64_t nb_pts) {
  return Ntot >= 1 && Ntot < (1ll << 31) && B >= 1 && B <= MVP_SAMPLE_MAX_CHUNKS && nb_pts >= 1 && nb_pts <= kScnMaxPts;
}

// ---- the gather ----------------------------------------------------------------------------------------------------------------------
constexpr int kGatThreads = 256;
constexpr int kGatRows = 4;  // scattered rows in flight per lane

struct GatherArgs {
  const float* points;
  const int64_t* label;
  const uint8_t* colors;
  const int64_t* scene_offsets;
  const int64_t* scene_of_row;
  const int64_t* choice;
  const float* rot;
  float* out_points;
  int64_t* out_label;
  float* out_feature;
  int64_t Ntot;
  int S, nb_pts;
};

// Slot s of row b reads row j of the store: 12 + 8 + 3 scattered bytes.  A lane takes kGatRows slots kGatThreads apart: all its loads are
// issued before the first store, and every store instruction of a wave writes 64 consecutive slots of one channel.
template <bool ROT>
__global__ __launch_bounds__(kGatThreads) void gather_cloud_kernel(GatherArgs a) {
  const int b = blockIdx.y, tid = threadIdx.x, nb = a.nb_pts;
  const int64_t sc = clamp_index(a.scene_of_row[b], a.S);
  int64_t off = a.scene_offsets[sc], end = a.scene_offsets[sc + 1];
  clamp_slice(off, end, a.Ntot);
  const int64_t n = end - off;
  const bool have = n > 0;  // a scene without points: zeros, label -100
  float R[9];
  if (ROT) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = a.rot[(size_t)b * 9 + i];
  }
  const int64_t s0 = (int64_t)blockIdx.x * (kGatThreads * kGatRows) + tid;
  size_t j[kGatRows];
#pragma unroll
  for (int k = 0; k < kGatRows; ++k) {
    const int64_t s = s0 + k * kGatThreads;
    const int64_t c = s < nb ? a.choice[(size_t)b * nb + s] : 0;
    j[k] = have ? (size_t)(off + clamp_index(c, n)) : 0;  // (row 0 exists: Ntot >= 1)
  }
  float x[kGatRows], y[kGatRows], z[kGatRows];
  int64_t lab[kGatRows];
  uint8_t col[kGatRows][3];
#pragma unroll
  for (int k = 0; k < kGatRows; ++k) {
    x[k] = a.points[j[k] * 3 + 0];
    y[k] = a.points[j[k] * 3 + 1];
    z[k] = a.points[j[k] * 3 + 2];
    lab[k] = a.label ? a.label[j[k]] : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) col[k][c] = a.colors ? a.colors[j[k] * 3 + c] : (uint8_t)0;
  }
#pragma unroll
  for (int k = 0; k < kGatRows; ++k) {
    const int64_t s = s0 + k * kGatThreads;
    if (s >= nb) continue;
    float* op = a.out_points + (size_t)b * 3 * nb + s;
    if (!have) {
      op[0] = op[nb] = op[2 * (size_t)nb] = 0.f;
    } else if (ROT) {
#pragma unroll
      for (int r = 0; r < 3; ++r) op[(size_t)r * nb] = (R[r * 3 + 0] * x[k] + R[r * 3 + 1] * y[k]) + R[r * 3 + 2] * z[k];  // never contracted
    } else {
      op[0] = x[k];
      op[nb] = y[k];
      op[2 * (size_t)nb] = z[k];
    }
    if (a.label) a.out_label[(size_t)b * nb + s] = have ? lab[k] : -100;
    if (a.colors) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.out_feature[((size_t)b * 3 + c) * nb + s] = have ? (float)col[k][c] / 255.0f : 0.f;  // IEEE division
    }
  }
}

}  // namespace

MVP_API int64_t mvp_sample_scenes_workspace(int64_t Ntot, int64_t B, int64_t nb_pts) {
  if (!scene_shape_ok(Ntot, B, nb_pts)) return 0;
  return (int64_t)scene_layout(B, nb_pts).total;
}

MVP_API int mvp_sample_scenes_f32(const int64_t* scene_offsets, const int64_t* scene_of_row, int64_t Ntot, int64_t S, int64_t B, int64_t nb_pts,
                                  uint64_t seed, const int64_t* seed_device, int64_t* choice, int32_t* num_points, void* workspace,
                                  int64_t workspace_bytes, mvp_stream_t stream) {
  MVP_NONNULL(scene_offsets);
  MVP_NONNULL(scene_of_row);
  MVP_NONNULL(choice);
  MVP_NONNULL(num_points);
  MVP_REQUIRE(Ntot >= 1 && S >= 1 && S < (1ll << 31) && B >= 0 && nb_pts >= 1);
  if (nb_pts > kScnMaxPts || Ntot >= (1ll << 31) || B > MVP_SAMPLE_MAX_CHUNKS) return MVP_EUNSUPPORTED;
  if (B == 0) return MVP_OK;
  const SceneLayout lay = scene_layout(B, nb_pts);
  MVP_NONNULL(workspace);
  MVP_REQUIRE(workspace_bytes >= (int64_t)lay.total && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  RowState* state = reinterpret_cast<RowState*>(ws + lay.state);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + lay.hist);
  unsigned long long* src = reinterpret_cast<unsigned long long*>(ws + lay.pairs);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(ws + lay.pairs2);
  const int G = scene_segments(Ntot), nb = (int)nb_pts;
  const dim3 grid((unsigned)G, (unsigned)B), rows((unsigned)B), block(kScnThreads);
  hipLaunchKernelGGL(scene_init_kernel, rows, block, 0, s, scene_offsets, scene_of_row, seed_device, seed, (int)S, Ntot, G, nb, state, hist, num_points);
  hipLaunchKernelGGL(scene_hist_kernel<0>, grid, block, 0, s, state, hist);
  hipLaunchKernelGGL(scene_digit_kernel<0>, rows, block, 0, s, state, hist);
  hipLaunchKernelGGL(scene_hist_kernel<1>, grid, block, 0, s, state, hist);
  hipLaunchKernelGGL(scene_digit_kernel<1>, rows, block, 0, s, state, hist);
  hipLaunchKernelGGL(scene_hist_kernel<2>, grid, block, 0, s, state, hist);
  hipLaunchKernelGGL(scene_digit_kernel<2>, rows, block, 0, s, state, hist);
  hipLaunchKernelGGL(scene_collect_kernel, grid, block, 0, s, state, nb, src);
  const int tiles = (int)cdiv(nb_pts, kTile);
  int P = 1;
  while (P < nb && P < kTile) P <<= 1;
  hipLaunchKernelGGL(scene_tile_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(kTileThreads), sizeof(unsigned long long) * (size_t)P, s, state, src, nb,
                     tiles == 1 ? 1 : 0, choice);
  const dim3 mgrid((unsigned)cdiv(nb_pts, kScnThreads), (unsigned)B);
  for (int L = kTile; L < nb; L *= 2) {
    hipLaunchKernelGGL(scene_merge_kernel, mgrid, block, 0, s, state, src, nb, L, 2 * L >= nb ? 1 : 0, dst, choice);
    unsigned long long* t = src;
    src = dst, dst = t;
  }
  return mvp_launch_status();
}

MVP_API int mvp_gather_cloud_f32(const float* points, const int64_t* seg_label, const uint8_t* colors, const int64_t* scene_offsets,
                                 const int64_t* scene_of_row, const int64_t* choice, const float* rot, int64_t Ntot, int64_t S, int64_t B,
                                 int64_t nb_pts, float* out_points, int64_t* out_label, float* out_feature, mvp_stream_t stream) {
  MVP_NONNULL(points);
  MVP_NONNULL(scene_offsets);
  MVP_NONNULL(scene_of_row);
  MVP_NONNULL(choice);
  MVP_NONNULL(out_points);
  if (seg_label) MVP_NONNULL(out_label);
  if (colors) MVP_NONNULL(out_feature);
  MVP_REQUIRE(Ntot >= 1 && S >= 1 && S < (1ll << 31) && B >= 0 && nb_pts >= 1);
  if (nb_pts >= (1ll << 31) || B > MVP_SAMPLE_MAX_CHUNKS) return MVP_EUNSUPPORTED;
  if (B == 0) return MVP_OK;
  GatherArgs a;
  a.points = points, a.label = seg_label, a.colors = colors, a.scene_offsets = scene_offsets, a.scene_of_row = scene_of_row, a.choice = choice;
  a.rot = rot, a.out_points = out_points, a.out_label = out_label, a.out_feature = out_feature, a.Ntot = Ntot, a.S = (int)S, a.nb_pts = (int)nb_pts;
  const dim3 grid((unsigned)cdiv(nb_pts, kGatThreads * kGatRows), (unsigned)B), block(kGatThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rot) {
    hipLaunchKernelGGL(gather_cloud_kernel<true>, grid, block, 0, s, a);
  } else {
    hipLaunchKernelGGL(gather_cloud_kernel<false>, grid, block, 0, s, a);
  }
  return mvp_launch_status();
}

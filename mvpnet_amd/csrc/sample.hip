// sample.hip -- a whole TRAINING batch of chunks drawn on the device for gfx950: what ScanNet2D3DChunks.__getitem__ does per sample in a
// data-loader worker (mvpnet/data/scannet_2d3d.py:341-381: random centre, box test, labelled-ratio test, up to T tries, whole-scene
// fallback, crop / pad to nb_pts) and the base-point mask of get_rgbd_data (:199-204), for B chunks of B (possibly different) resident
// scenes in ten launches and no host synchronisation.  Definition: include/mvp_hip.h (mvp_sample_chunks_f32).
//
// A chunk's scene is cut into G segments of `seg` consecutive points (seg a multiple of the workgroup size), one workgroup each, so every
// pass over the scene is a (G, B) grid and "ascending point index" is "ascending segment, then ascending position":
//   count_kernel   : every point once per chunk against all T boxes (LDS broadcast), per try the member and labelled-member counts by
//                    ballot + popcount, lane t of a wave keeps try t's counters; per workgroup ONE plain store of (m, l) per try and of
//                    the segment's xy extent -- integers and min / max: no atomics, independent of order.
//   pick_kernel    : per chunk the first passing try (or the fallback), the box, m, the segments' exclusive member offsets; zeroes the
//                    chunk's histograms.
//   select_kernel<0> : pad chunks (m < nb_pts): ordered compaction of the member list (segment offset + in-wave prefix);
//                      crop chunks: histogram of the top 8 key bits over the members (LDS histogram, integer atomics).
//   digit_kernel<P> / select_kernel<1,2> : radix select of the nb_pts-th smallest key, 8 + 12 + 12 bits.
//   collect_kernel : the nb_pts members with key <= that key as (key, index) pairs, in any order (one returning atomic per wave).
//   finish_kernel  : one workgroup per chunk: bitonic sort of the pairs in LDS (crop) or the pad rule, then the gather of points and
//                    labels and the base-point bits.
// The keys, the select, the collect and the sort are keyed_select.h's, shared with scene_sample.hip; this file adds what a member is (the
// box test), the tries and the ordered compaction of pad chunks.  Measurements: DESIGN.md (training chunks).
#include "keyed_select.h"
#include <math.h>

namespace {

constexpr int kSmpThreads = kSelThreads;
constexpr int kSmpMaxSeg = 64;      // workgroups per chunk and pass (one wave scans them in pick_kernel)
constexpr int kSmpMaxTries = MVP_SAMPLE_MAX_TRIES;
constexpr int kSmpMaxPts = MVP_SAMPLE_MAX_PTS;  // 8192 (key, index) pairs = 64 KiB of LDS
constexpr int kFinThreads = 1024;

struct ChunkState : SelectState {  // per chunk, written by pick_kernel; crop: m >= nb_pts
  double lo_x, lo_y, hi_x, hi_y;   // the winning box (float32 bounds are exact in double, so later passes compare in double only)
  int32_t m;                       // members
  int32_t all;                     // fallback: every point is a member
};

// the box of a try in BT = float (ScanNet2D3DChunks) or double (ScanNet3DChunks): (c -/+ half) -/+ margin, each operation rounded once
template <typename BT>
__device__ __forceinline__ void try_box(const float* __restrict__ points, const Slice& sc, int64_t ci, BT hx, BT hy, BT mx, BT my, BT& lox,
                                        BT& loy, BT& hix, BT& hiy) {
  if (sc.n <= 0) {
    lox = loy = hix = hiy = (BT)NAN;
    return;
  }
  ci = clamp_index(ci, sc.n);
  const BT cx = (BT)points[(sc.off + ci) * 3 + 0], cy = (BT)points[(sc.off + ci) * 3 + 1];
  lox = (cx - hx) - mx;
  loy = (cy - hy) - my;
  hix = (cx + hx) + mx;
  hiy = (cy + hy) + my;
}

template <typename BT>
__global__ __launch_bounds__(kSmpThreads) void count_kernel(const float* __restrict__ points, const int64_t* __restrict__ label,
                                                            const int64_t* __restrict__ scene_offsets,
                                                            const int64_t* __restrict__ scene_of_chunk,
                                                            const int64_t* __restrict__ center_ind, int S, int64_t Ntot, int T, BT hx, BT hy,
                                                            BT mx, BT my, int2* __restrict__ pcount, float4* __restrict__ pbox) {
  __shared__ BT s_lox[kSmpMaxTries], s_loy[kSmpMaxTries], s_hix[kSmpMaxTries], s_hiy[kSmpMaxTries];
  __shared__ int s_m[kSmpThreads / kWave][kSmpMaxTries], s_l[kSmpThreads / kWave][kSmpMaxTries];
  __shared__ float s_ext[kSmpThreads / kWave][4];
  const int g = blockIdx.x, G = gridDim.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const Slice sc = scene_slice(scene_offsets, scene_of_chunk, b, S, Ntot, G);
  if (tid < T) try_box<BT>(points, sc, center_ind[(size_t)b * T + tid], hx, hy, mx, my, s_lox[tid], s_loy[tid], s_hix[tid], s_hiy[tid]);
  __syncthreads();
  int64_t begin, end;
  segment_range(sc, g, begin, end);
  int mc = 0, lc = 0;
  float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
  for (int64_t base = begin; base < end; base += kSmpThreads) {  // uniform over the workgroup: every lane takes part in the ballots
    const int64_t j = base + tid;
    const bool valid = j < end;
    float xf = NAN, yf = NAN;
    bool lab = false;
    if (valid) {
      xf = points[(sc.off + j) * 3 + 0];
      yf = points[(sc.off + j) * 3 + 1];
      lab = label[sc.off + j] >= 0;
      mnx = nan_min(mnx, xf);
      mny = nan_min(mny, yf);
      mxx = nan_max(mxx, xf);
      mxy = nan_max(mxy, yf);
    }
    const BT x = (BT)xf, y = (BT)yf;
    for (int t = 0; t < T; ++t) {
      const bool in = valid && x >= s_lox[t] && x <= s_hix[t] && y >= s_loy[t] && y <= s_hiy[t];  // inclusive; false for NaN
      const unsigned long long bm = __ballot(in), bl = __ballot(in && lab);
      if (lane == t) {
        mc += __popcll(bm);
        lc += __popcll(bl);
      }
    }
  }
#pragma unroll
  for (int k = kWave / 2; k >= 1; k >>= 1) {
    mnx = nan_min(mnx, __shfl_xor(mnx, k, kWave));
    mny = nan_min(mny, __shfl_xor(mny, k, kWave));
    mxx = nan_max(mxx, __shfl_xor(mxx, k, kWave));
    mxy = nan_max(mxy, __shfl_xor(mxy, k, kWave));
  }
  if (lane < T) {
    s_m[wave][lane] = mc;
    s_l[wave][lane] = lc;
  }
  if (lane == 0) {
    s_ext[wave][0] = mnx;
    s_ext[wave][1] = mny;
    s_ext[wave][2] = mxx;
    s_ext[wave][3] = mxy;
  }
  __syncthreads();
  if (tid < T) {
    int m = 0, l = 0;
#pragma unroll
    for (int w = 0; w < kSmpThreads / kWave; ++w) {
      m += s_m[w][tid];
      l += s_l[w][tid];
    }
    pcount[((size_t)b * G + g) * T + tid] = make_int2(m, l);
  }
  if (tid == 0) {
    float4 e = make_float4(s_ext[0][0], s_ext[0][1], s_ext[0][2], s_ext[0][3]);
#pragma unroll
    for (int w = 1; w < kSmpThreads / kWave; ++w) {
      e.x = nan_min(e.x, s_ext[w][0]);
      e.y = nan_min(e.y, s_ext[w][1]);
      e.z = nan_max(e.z, s_ext[w][2]);
      e.w = nan_max(e.w, s_ext[w][3]);
    }
    pbox[(size_t)b * G + g] = e;
  }
}

struct PickArgs {
  const float* points;
  const int64_t* scene_offsets;
  const int64_t* scene_of_chunk;
  const int64_t* center_ind;
  const int64_t* seed_device;
  const int2* pcount;
  const float4* pbox;
  ChunkState* state;
  uint32_t* hist;
  int32_t* blockoff;
  float* chunk_box;
  int32_t* try_index;
  int32_t* num_members;
  double hx, hy, mx, my, thresh;
  uint64_t seed;
  int64_t Ntot;
  int S, T, G, nb_pts, f64;
};

__global__ __launch_bounds__(kSmpThreads) void pick_kernel(PickArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  zero_hist(a.hist, b);
  if (tid >= kWave) return;
  const int lane = tid, T = a.T, G = a.G;
  const Slice sc = scene_slice(a.scene_offsets, a.scene_of_chunk, b, a.S, a.Ntot, G);
  int m = 0, l = 0;
  if (lane < T)
    for (int g = 0; g < G; ++g) {
      const int2 c = a.pcount[((size_t)b * G + g) * T + lane];
      m += c.x;
      l += c.y;
    }
  // numpy.mean of a bool array: the count of True as a double divided by the length; compared with the threshold in double (:360)
  const bool pass = lane < T && m > 0 && (double)l / (double)m >= a.thresh;
  const unsigned long long bal = __ballot(pass);
  const int win = bal ? __ffsll((long long)bal) - 1 : -1;
  double lox, loy, hix, hiy;
  int mw;
  if (win >= 0) {
    const int64_t ci = a.center_ind[(size_t)b * T + win];
    if (a.f64) {
      try_box<double>(a.points, sc, ci, a.hx, a.hy, a.mx, a.my, lox, loy, hix, hiy);
    } else {
      float flx, fly, fhx, fhy;
      try_box<float>(a.points, sc, ci, (float)a.hx, (float)a.hy, (float)a.mx, (float)a.my, flx, fly, fhx, fhy);
      lox = flx, loy = fly, hix = fhx, hiy = fhy;
    }
    mw = __shfl(m, win, kWave);
  } else {  // :364-369: the whole scene, box = its xy extent -/+ margin in float32
    float4 e = lane < G ? a.pbox[(size_t)b * G + lane] : make_float4(INFINITY, INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int k = kWave / 2; k >= 1; k >>= 1) {
      e.x = nan_min(e.x, __shfl_xor(e.x, k, kWave));
      e.y = nan_min(e.y, __shfl_xor(e.y, k, kWave));
      e.z = nan_max(e.z, __shfl_xor(e.z, k, kWave));
      e.w = nan_max(e.w, __shfl_xor(e.w, k, kWave));
    }
    lox = e.x - (float)a.mx, loy = e.y - (float)a.my, hix = e.z + (float)a.mx, hiy = e.w + (float)a.my;
    mw = sc.n;
  }
  // exclusive member offsets of the segments (the ordered compaction's bases)
  int cnt = 0;
  if (lane < G) {
    if (win >= 0) {
      cnt = a.pcount[((size_t)b * G + lane) * T + win].x;
    } else {
      const int64_t lo = (int64_t)lane * sc.seg;
      cnt = lo >= sc.n ? 0 : (int)(lo + sc.seg <= sc.n ? sc.seg : sc.n - lo);
    }
  }
  int inc = cnt;
#pragma unroll
  for (int k = 1; k < kWave; k <<= 1) {
    const int o = __shfl_up(inc, k, kWave);
    if (lane >= k) inc += o;
  }
  if (lane < G) a.blockoff[(size_t)b * G + lane] = inc - cnt;
  if (lane == 0) {
    ChunkState st;
    select_init(st, sc, mw, a.nb_pts, a.seed_device, a.seed, b);
    st.lo_x = lox, st.lo_y = loy, st.hi_x = hix, st.hi_y = hiy;
    st.m = mw;
    st.all = win < 0;
    a.state[b] = st;
    a.chunk_box[(size_t)b * 4 + 0] = (float)lox;
    a.chunk_box[(size_t)b * 4 + 1] = (float)loy;
    a.chunk_box[(size_t)b * 4 + 2] = (float)hix;
    a.chunk_box[(size_t)b * 4 + 3] = (float)hiy;
    a.try_index[b] = win;
    a.num_members[b] = mw;
  }
}

__device__ __forceinline__ bool is_member(const ChunkState& st, float xf, float yf) {
  const double x = xf, y = yf;
  return st.all || (x >= st.lo_x && x <= st.hi_x && y >= st.lo_y && y <= st.hi_y);
}
// ... of point j of the chunk's scene
__device__ __forceinline__ bool is_member(const ChunkState& st, const float* __restrict__ points, int64_t j) {
  return is_member(st, points[(st.off + j) * 3 + 0], points[(st.off + j) * 3 + 1]);
}

// PASS 0: compaction (pad chunks) or the histogram of key bits 31..24 (crop chunks); PASS 1 / 2: bits 23..12 / 11..0 of the keys that
// share the bits fixed so far
template <int PASS>
__global__ __launch_bounds__(kSmpThreads) void select_kernel(const float* __restrict__ points, const ChunkState* __restrict__ state,
                                                             const int32_t* __restrict__ blockoff, int nb_pts,
                                                             uint32_t* __restrict__ hist_all, int32_t* __restrict__ members) {
  __shared__ uint32_t s_hist[kBins0];
  __shared__ int s_wtot[kSmpThreads / kWave];
  const int g = blockIdx.x, G = gridDim.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const ChunkState st = state[b];
  if (PASS > 0 && !st.crop) return;
  int64_t begin, end;
  segment_range(st, g, begin, end);
  if (begin >= end) return;
  uint32_t* hist = hist_all + (size_t)b * kHistWords;
  const bool compact = PASS == 0 && !st.crop;
  if (!compact) hist_begin<PASS>(s_hist);
  int run = PASS == 0 ? blockoff[(size_t)b * G + g] : 0;
  for (int64_t base = begin; base < end; base += kSmpThreads) {
    const int64_t j = base + tid;
    bool in = false;
    if (j < end) in = is_member(st, points, j);
    if (PASS == 0 && compact) {
      const unsigned long long bal = __ballot(in);
      const int before = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) s_wtot[wave] = __popcll(bal);
      __syncthreads();
      int wbase = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kSmpThreads / kWave; ++w) {
        wbase += w < wave ? s_wtot[w] : 0;
        total += s_wtot[w];
      }
      const int pos = run + wbase + before;
      if (in && pos < nb_pts) members[(size_t)b * nb_pts + pos] = (int32_t)j;
      run += total;
      __syncthreads();  // s_wtot is rewritten by the next tile
    } else if (in) {
      hist_key<PASS>(select_key(j, st.sb), st.prefix, s_hist, hist);
    }
  }
  if (!compact) hist_end<PASS>(s_hist, hist);
}

template <int PASS>
__global__ __launch_bounds__(kSmpThreads) void digit_kernel(ChunkState* __restrict__ state, const uint32_t* __restrict__ hist_all) {
  digit_search<PASS>(state, hist_all);
}

__global__ __launch_bounds__(kSmpThreads) void collect_kernel(const float* __restrict__ points, ChunkState* __restrict__ state, int nb_pts,
                                                              unsigned long long* __restrict__ pairs) {
  collect_pairs(state, nb_pts, pairs, [points](const ChunkState& st, int64_t j) { return is_member(st, points, j); });
}

struct FinishArgs {
  const float* points;
  const int64_t* label;
  const int64_t* base_point_ind;
  const ChunkState* state;
  const int32_t* members;
  const unsigned long long* pairs;
  const int64_t* scene_of_chunk;
  int64_t* choice;
  float* out_points;
  int64_t* out_label;
  uint32_t* base_bits;
  int S, nb_pts, P, nbp;
};

__global__ __launch_bounds__(kFinThreads) void finish_kernel(FinishArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sample_smem[];
  unsigned long long* buf = reinterpret_cast<unsigned long long*>(sample_smem);  // P pairs, P = nb_pts rounded up to a power of two
  const int b = blockIdx.x, tid = threadIdx.x;
  const ChunkState st = a.state[b];
  const int nb = a.nb_pts, P = a.P;
  if (st.crop) bitonic_sort_lds<kFinThreads>(buf, a.pairs + (size_t)b * nb, nb, P);
  for (int s = tid; s < nb; s += kFinThreads) {
    unsigned long long pair = 0ull;
    if (st.crop) {
      pair = buf[s];
    } else if (st.m > 0) {
      pair = (uint32_t)a.members[(size_t)b * nb + pad_member(s, st.m, st.sb)];
    }
    const int64_t idx = choice_of(pair, st.n);
    a.choice[(size_t)b * nb + s] = idx;
    const bool ok = st.n > 0;
    const size_t p = (size_t)(st.off + idx);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out_points[((size_t)b * 3 + c) * nb + s] = ok ? a.points[p * 3 + c] : 0.f;
    a.out_label[(size_t)b * nb + s] = ok ? a.label[p] : -100;
  }
  if (a.nbp > 0) {  // bit j: base point j of the chunk's scene is a member (:200-204)
    const int64_t sidx = clamp_index(a.scene_of_chunk[b], a.S);
    write_base_bits<kFinThreads>(a.base_bits + (size_t)b * ((a.nbp + 31) >> 5), a.nbp, [&](int j) {
      if (st.n <= 0) return false;
      const int64_t p = clamp_index(a.base_point_ind[(size_t)sidx * a.nbp + j], st.n);
      return is_member(st, a.points, p);
    });
  }
}

inline int sample_segments(int64_t Ntot) { return segments(Ntot, kSmpThreads, kSmpMaxSeg); }

struct SampleLayout {
  size_t state, hist, pcount, pbox, blockoff, members, pairs, total;
};
inline SampleLayout sample_layout(int64_t B, int64_t T, int64_t nb_pts, int G) {
  SampleLayout l;
  size_t at = 0;
  l.state = at, at = align16(at + sizeof(ChunkState) * (size_t)B);
  l.hist = at, at = align16(at + sizeof(uint32_t) * (size_t)B * kHistWords);
  l.pcount = at, at = align16(at + sizeof(int2) * (size_t)B * G * (size_t)T);
  l.pbox = at, at = align16(at + sizeof(float4) * (size_t)B * G);
  l.blockoff = at, at = align16(at + sizeof(int32_t) * (size_t)B * G);
  l.members = at, at = align16(at + sizeof(int32_t) * (size_t)B * (size_t)nb_pts);
  l.pairs = at, at = align16(at + sizeof(unsigned long long) * (size_t)B * (size_t)nb_pts);
  l.total = at;
  return l;
}

inline bool sample_shape_ok(int64_t Ntot, int64_t B, int64_t T, int64_t nb_pts) {
  return Ntot >= 1 && Ntot < (1ll << 31) && B >= 1 && B <= MVP_SAMPLE_MAX_CHUNKS && T >= 1 && T <= kSmpMaxTries && nb_pts >= 1 &&
         nb_pts <= kSmpMaxPts;
}

}  // namespace

MVP_API int64_t mvp_sample_chunks_workspace(int64_t Ntot, int64_t B, int64_t T, int64_t nb_pts) {
  if (!sample_shape_ok(Ntot, B, T, nb_pts)) return 0;
  return (int64_t)sample_layout(B, T, nb_pts, sample_segments(Ntot)).total;
}

MVP_API int mvp_sample_chunks_f32(const float* points, const int64_t* seg_label, const int64_t* scene_offsets, const int64_t* scene_of_chunk,
                                  const int64_t* center_ind, const int64_t* base_point_ind, int64_t Ntot, int64_t S, int64_t B, int64_t T,
                                  int64_t nbp, int64_t nb_pts, double size_x, double size_y, double margin_x, double margin_y,
                                  double chunk_thresh, int bounds_f64, uint64_t seed, const int64_t* seed_device, int64_t* choice,
                                  float* out_points, int64_t* out_label, float* chunk_box, int32_t* try_index, int32_t* num_members,
                                  uint32_t* base_bits, void* workspace, int64_t workspace_bytes, mvp_stream_t stream) {
  MVP_NONNULL(points);
  MVP_NONNULL(seg_label);
  MVP_NONNULL(scene_offsets);
  MVP_NONNULL(scene_of_chunk);
  MVP_NONNULL(center_ind);
  MVP_NONNULL(choice);
  MVP_NONNULL(out_points);
  MVP_NONNULL(out_label);
  MVP_NONNULL(chunk_box);
  MVP_NONNULL(try_index);
  MVP_NONNULL(num_members);
  MVP_REQUIRE(Ntot >= 1 && S >= 1 && S < (1ll << 31) && B >= 0 && T >= 1 && nb_pts >= 1 && nbp >= 0 && nbp < (1ll << 31));
  MVP_REQUIRE(size_x == size_x && size_y == size_y && margin_x == margin_x && margin_y == margin_y && chunk_thresh == chunk_thresh);
  if (nbp > 0) {
    MVP_NONNULL(base_point_ind);
    MVP_NONNULL(base_bits);
  }
  if (nb_pts > kSmpMaxPts || T > kSmpMaxTries || Ntot >= (1ll << 31) || B > MVP_SAMPLE_MAX_CHUNKS) return MVP_EUNSUPPORTED;
  if (B == 0) return MVP_OK;
  const int G = sample_segments(Ntot);
  const SampleLayout lay = sample_layout(B, T, nb_pts, G);
  MVP_NONNULL(workspace);
  MVP_REQUIRE(workspace_bytes >= (int64_t)lay.total && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  ChunkState* state = reinterpret_cast<ChunkState*>(ws + lay.state);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + lay.hist);
  int2* pcount = reinterpret_cast<int2*>(ws + lay.pcount);
  float4* pbox = reinterpret_cast<float4*>(ws + lay.pbox);
  int32_t* blockoff = reinterpret_cast<int32_t*>(ws + lay.blockoff);
  int32_t* members = reinterpret_cast<int32_t*>(ws + lay.members);
  unsigned long long* pairs = reinterpret_cast<unsigned long long*>(ws + lay.pairs);
  const dim3 grid((unsigned)G, (unsigned)B), block(kSmpThreads);
  // 0.5 * size in the arithmetic of the bounds: float32 chunk_size / chunk_margin (ScanNet2D3DChunks) or float64 (ScanNet3DChunks)
  if (bounds_f64) {
    hipLaunchKernelGGL(count_kernel<double>, grid, block, 0, s, points, seg_label, scene_offsets, scene_of_chunk, center_ind, (int)S, Ntot,
                       (int)T, 0.5 * size_x, 0.5 * size_y, margin_x, margin_y, pcount, pbox);
  } else {
    hipLaunchKernelGGL(count_kernel<float>, grid, block, 0, s, points, seg_label, scene_offsets, scene_of_chunk, center_ind, (int)S, Ntot,
                       (int)T, 0.5f * (float)size_x, 0.5f * (float)size_y, (float)margin_x, (float)margin_y, pcount, pbox);
  }
  PickArgs pa;
  pa.points = points, pa.scene_offsets = scene_offsets, pa.scene_of_chunk = scene_of_chunk, pa.center_ind = center_ind;
  pa.seed_device = seed_device, pa.pcount = pcount, pa.pbox = pbox, pa.state = state, pa.hist = hist, pa.blockoff = blockoff;
  pa.chunk_box = chunk_box, pa.try_index = try_index, pa.num_members = num_members;
  if (bounds_f64) {
    pa.hx = 0.5 * size_x, pa.hy = 0.5 * size_y, pa.mx = margin_x, pa.my = margin_y;
  } else {
    pa.hx = 0.5f * (float)size_x, pa.hy = 0.5f * (float)size_y, pa.mx = (float)margin_x, pa.my = (float)margin_y;
  }
  pa.thresh = chunk_thresh, pa.seed = seed, pa.Ntot = Ntot, pa.S = (int)S, pa.T = (int)T, pa.G = G, pa.nb_pts = (int)nb_pts;
  pa.f64 = bounds_f64 ? 1 : 0;
  hipLaunchKernelGGL(pick_kernel, dim3((unsigned)B), block, 0, s, pa);
  hipLaunchKernelGGL(select_kernel<0>, grid, block, 0, s, points, state, blockoff, (int)nb_pts, hist, members);
  hipLaunchKernelGGL(digit_kernel<0>, dim3((unsigned)B), block, 0, s, state, hist);
  hipLaunchKernelGGL(select_kernel<1>, grid, block, 0, s, points, state, blockoff, (int)nb_pts, hist, members);
  hipLaunchKernelGGL(digit_kernel<1>, dim3((unsigned)B), block, 0, s, state, hist);
  hipLaunchKernelGGL(select_kernel<2>, grid, block, 0, s, points, state, blockoff, (int)nb_pts, hist, members);
  hipLaunchKernelGGL(digit_kernel<2>, dim3((unsigned)B), block, 0, s, state, hist);
  hipLaunchKernelGGL(collect_kernel, grid, block, 0, s, points, state, (int)nb_pts, pairs);
  int P = 1;
  while (P < nb_pts) P <<= 1;
  FinishArgs fa;
  fa.points = points, fa.label = seg_label, fa.base_point_ind = base_point_ind, fa.state = state, fa.members = members, fa.pairs = pairs;
  fa.scene_of_chunk = scene_of_chunk, fa.choice = choice, fa.out_points = out_points, fa.out_label = out_label, fa.base_bits = base_bits;
  fa.S = (int)S, fa.nb_pts = (int)nb_pts, fa.P = P, fa.nbp = (int)nbp;
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)B), dim3(kFinThreads), sizeof(unsigned long long) * (size_t)P, s, fa);
  return mvp_launch_status();
}

// keyed_select.h -- the resampling core of the two samplers (sample.hip: the members of a chunk's box; scene_sample.hip: every point of a
// scene): among the members j of a row, the nb_pts with the smallest keys h(j ^ s_b), in key order.  The rule is pinned in
// include/mvp_hip.h (mvp_sample_chunks_f32, mvp_sample_scenes_f32); this is the one place that states it in code:
//   scene_slice / select_init : a row's clamped slice cut into G segments of `seg` points, pad or crop, s_b from the folded seed
//   hist_key<PASS> / digit_search<PASS> : radix select of the nb_pts-th smallest key in 8 + 12 + 12 bits; `prefix` ends as that key
//   collect_pairs             : the members with key <= prefix as (key << 32 | index) pairs, in any order
//   bitonic_sort_lds / choice_of : up to 8192 pairs sorted in LDS, a pair's index as the row's choice
// The callers keep their kernels, grids, segment sizes and what a member is; every pass runs workgroups of kSelThreads.
#pragma once
#include "chunk_common.h"

namespace {

constexpr int kSelThreads = 256;
constexpr int kBins0 = 256, kBins12 = 4096;       // bins of pass 0 and of passes 1 / 2
constexpr int kHistWords = kBins0 + 2 * kBins12;  // per row, zeroed by the caller's first kernel (zero_hist)

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
// workgroups per row and pass: one per `points_per_workgroup` points of the store, at most `max_segments`
inline int segments(int64_t Ntot, int points_per_workgroup, int max_segments) {
  const int64_t g = cdiv(Ntot, points_per_workgroup);
  return (int)(g < 1 ? 1 : (g > max_segments ? max_segments : g));
}

struct SelectState {  // per row, written by select_init
  int64_t off;        // first point of the row's scene
  int32_t n;          // points of the scene
  int32_t seg;        // points per workgroup
  int32_t crop;       // members >= nb_pts
  uint32_t sb;        // s_b
  uint32_t prefix;    // radix select: the key bits fixed so far
  int32_t rank;       // ... and the rank wanted among the keys sharing them
  int32_t taken;      // collect_pairs' counter
  int32_t pad_;
};

struct Slice {
  int64_t off;
  int32_t n, seg;
};

// scene of row b; indices and offsets are clamped into the arrays, so wrong arguments give wrong results and never a stray access.
// seg is a multiple of the workgroup size; n < 2^31 and G <= 2^8, so the sum fits 32 unsigned bits.
__device__ __forceinline__ Slice scene_slice(const int64_t* __restrict__ scene_offsets, const int64_t* __restrict__ scene_of_row, int b,
                                             int S, int64_t Ntot, int G) {
  const int64_t s = clamp_index(scene_of_row[b], S);
  int64_t off = scene_offsets[s], end = scene_offsets[s + 1];
  clamp_slice(off, end, Ntot);
  Slice sc;
  sc.off = off;
  sc.n = (int32_t)(end - off);
  const int per = (int)(((uint32_t)sc.n + (uint32_t)G - 1u) / (uint32_t)G);
  sc.seg = (per + kSelThreads - 1) / kSelThreads * kSelThreads;
  return sc;
}

// points [begin, end) of the scene are segment g's
template <typename T>
__device__ __forceinline__ void segment_range(const T& sc, int g, int64_t& begin, int64_t& end) {
  begin = (int64_t)g * sc.seg;
  end = begin + sc.seg < sc.n ? begin + sc.seg : sc.n;
}

__device__ __forceinline__ void select_init(SelectState& st, const Slice& sc, int members, int nb_pts, const int64_t* __restrict__ seed_device,
                                            uint64_t seed, int b) {
  const uint64_t s64 = seed_device ? (uint64_t)seed_device[0] : seed;
  st.off = sc.off;
  st.n = sc.n;
  st.seg = sc.seg;
  st.crop = members >= nb_pts;
  st.sb = chunk_seed((uint32_t)(s64 ^ (s64 >> 32)), b);
  st.prefix = 0u;
  st.rank = nb_pts;
  st.taken = 0;
  st.pad_ = 0;
}

__device__ __forceinline__ void zero_hist(uint32_t* __restrict__ hist_all, int b) {
  for (int i = threadIdx.x; i < kHistWords; i += kSelThreads) hist_all[(size_t)b * kHistWords + i] = 0u;
}

// h is a bijection, so the keys of a row are distinct
__device__ __forceinline__ uint32_t select_key(int64_t j, uint32_t sb) { return lowbias32((uint32_t)j ^ sb); }

// One member's key in the histogram of key bits 31..24 (PASS 0, in the workgroup's s_hist[kBins0] between hist_begin and hist_end) or of
// bits 23..12 / 11..0 of the keys that share the bits fixed so far (PASS 1 / 2, in the row's `hist`).  Integer atomics: order-free.
template <int PASS>
__device__ __forceinline__ void hist_begin(uint32_t* s_hist) {
  if (PASS != 0) return;
  for (int i = threadIdx.x; i < kBins0; i += kSelThreads) s_hist[i] = 0u;
  __syncthreads();
}
template <int PASS>
__device__ __forceinline__ void hist_key(uint32_t key, uint32_t prefix, uint32_t* s_hist, uint32_t* __restrict__ hist) {
  if (PASS == 0) atomicAdd(&s_hist[key >> 24], 1u);
  if (PASS == 1 && (key >> 24) == (prefix >> 24)) atomicAdd(&hist[kBins0 + ((key >> 12) & 4095u)], 1u);
  if (PASS == 2 && (key >> 12) == (prefix >> 12)) atomicAdd(&hist[kBins0 + kBins12 + (key & 4095u)], 1u);
}
template <int PASS>
__device__ __forceinline__ void hist_end(const uint32_t* s_hist, uint32_t* __restrict__ hist) {
  if (PASS != 0) return;
  __syncthreads();
  for (int i = threadIdx.x; i < kBins0; i += kSelThreads) {
    const uint32_t v = s_hist[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

// the digit of pass PASS: the bin d with (keys in bins < d) < rank <= (keys in bins <= d).  One workgroup per row (blockIdx.x).
template <int PASS, typename State>
__device__ __forceinline__ void digit_search(State* __restrict__ state, const uint32_t* __restrict__ hist_all) {
  constexpr int BINS = PASS == 0 ? kBins0 : kBins12;
  constexpr int PER = BINS / kSelThreads;
  constexpr int SHIFT = PASS == 0 ? 24 : (PASS == 1 ? 12 : 0);
  __shared__ int s_wtot[kSelThreads / kWave];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  if (!state[b].crop) return;
  const int rank = state[b].rank;
  const uint32_t* hist = hist_all + (size_t)b * kHistWords + (PASS == 0 ? 0 : (PASS == 1 ? kBins0 : kBins0 + kBins12));
  int v[PER], local = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    v[i] = (int)hist[tid * PER + i];
    local += v[i];
  }
  int inc = local;
#pragma unroll
  for (int k = 1; k < kWave; k <<= 1) {
    const int o = __shfl_up(inc, k, kWave);
    if (lane >= k) inc += o;
  }
  if (lane == kWave - 1) s_wtot[wave] = inc;
  __syncthreads();  // (also: every thread has read `rank` before the one below rewrites it)
  int below = inc - local;
#pragma unroll
  for (int w = 0; w < kSelThreads / kWave; ++w) below += w < wave ? s_wtot[w] : 0;
  if (below < rank && rank <= below + local) {  // exactly one thread: 1 <= rank <= number of keys
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (below < rank && rank <= below + v[i]) {
        state[b].rank = rank - below;
        state[b].prefix |= (uint32_t)(tid * PER + i) << SHIFT;
      }
      below += v[i];
    }
  }
}

// Segment blockIdx.x of row blockIdx.y: the members (member(st, j)) with key <= prefix -- exactly nb_pts of a row, the keys are distinct --
// as pairs, in any order: one returning atomic per wave.  The tile loop is uniform over the wave: every lane takes part in the ballot.
template <typename State, typename Member>
__device__ __forceinline__ void collect_pairs(State* __restrict__ state, int nb_pts, unsigned long long* __restrict__ pairs, Member member) {
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1);
  const State st = state[b];
  if (!st.crop) return;
  int64_t begin, end;
  segment_range(st, blockIdx.x, begin, end);
  for (int64_t base = begin; base < end; base += kSelThreads) {
    const int64_t j = base + tid;
    const uint32_t key = select_key(j, st.sb);
    const bool take = j < end && member(st, j) && key <= st.prefix;
    const unsigned long long bal = __ballot(take);
    if (bal == 0ull) continue;
    const int leader = __ffsll((long long)bal) - 1;
    int at = 0;
    if (lane == leader) at = atomicAdd(&state[b].taken, __popcll(bal));
    at = __shfl(at, leader, kWave);
    const int pos = at + __popcll(bal & ((1ull << lane) - 1ull));
    if (take && pos < nb_pts) pairs[(size_t)b * nb_pts + pos] = ((unsigned long long)key << 32) | (uint32_t)j;
  }
}

// buf[0, P) = src[0, cnt) padded with ~0ull, sorted ascending by a workgroup of THREADS; P a power of two >= cnt, at most 8192 pairs (the
// 64 KiB of LDS a workgroup gets).  Every lane of the workgroup must arrive here; buf is readable by all on return.
template <int THREADS>
__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* buf, const unsigned long long* __restrict__ src, int cnt, int P) {
  const int tid = threadIdx.x;
  for (int i = tid; i < P; i += THREADS) buf[i] = i < cnt ? src[i] : ~0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const unsigned long long x = buf[i], y = buf[o];
          if ((x > y) == ((i & k) == 0)) {
            buf[i] = y;
            buf[o] = x;
          }
        }
      }
      __syncthreads();
    }
}

// a pair's (or a bare index's) point as the row's choice: inside the scene, 0 for a scene without points
__device__ __forceinline__ int64_t choice_of(unsigned long long pair, int n) {
  const int64_t idx = clamp_index((int64_t)(uint32_t)pair, n);
  return idx < 0 ? 0 : idx;
}

}  // namespace

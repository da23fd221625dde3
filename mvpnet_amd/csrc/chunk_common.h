// chunk_common.h -- what the two samplers (sample.hip, scene_sample.hip) and the whole-scene chunker (chunker.hip) share: the pad rule, the
// NaN-propagating min / max, the slice clamp and the base-point bit-row writer.  The rules are pinned in include/mvp_hip.h
// (mvp_sample_chunks_f32, mvp_sample_scenes_f32, mvp_scene_chunks_*, mvp_pack_chunks_f32); this is the one place that states them in
// code.  The crop half of the resampling rule, which only the samplers need, is keyed_select.h.
#pragma once
#include "common.h"   // kWave
#include "dropout.h"  // lowbias32

namespace {

// The pad rule: chunk c of a call draws from its own seed; slot s behind the m members (0 < m < 2^32) repeats member h(s ^ seed_c ^ K) * m >> 32.
__host__ __device__ __forceinline__ uint32_t chunk_seed(uint32_t seed32, int c) { return lowbias32(seed32 + 0x9E3779B9u * (uint32_t)(c + 1)); }
__host__ __device__ __forceinline__ int64_t pad_member(int64_t s, int64_t m, uint32_t seed_c) {
  return s < m ? s : (int64_t)(((unsigned long long)lowbias32((uint32_t)s ^ seed_c ^ 0x85EBCA6Bu) * (unsigned long long)m) >> 32);
}

// NaN-propagating min / max (numpy.min / numpy.max, torch.amin / amax)
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

// An index cut to its array of n >= 1 entries, a slice (off, end) to its array of `total`: wrong arguments give wrong results and never a
// stray access.
__host__ __device__ __forceinline__ int64_t clamp_index(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__host__ __device__ __forceinline__ void clamp_slice(int64_t& off, int64_t& end, int64_t total) {
  off = off < 0 ? 0 : (off > total ? total : off);
  end = end < off ? off : (end > total ? total : end);
}

// Bit row of a chunk over nb base points, by a workgroup of THREADS: bit j & 31 of word j >> 5 = member(j).  64 base points per wave and
// step, two words per ballot; member(j) is asked for j < nb only.  Every lane of the workgroup must arrive here.
template <int THREADS, typename Member>
__device__ __forceinline__ void write_base_bits(uint32_t* __restrict__ row, int nb, Member member) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), W = (nb + 31) >> 5;
  for (int j0 = (tid / kWave) * kWave; j0 < nb; j0 += THREADS) {
    const int j = j0 + lane;
    const unsigned long long bal = __ballot(j < nb && member(j));
    const int word = (j0 >> 5) + (lane >> 5);
    if ((lane & 31) == 0 && word < W) row[word] = (uint32_t)(bal >> (lane & 32));
  }
}

}  // namespace

// lift_vote.hip -- the whole-scene test of the 2D baseline (mvpnet/test_2d_chunks.py:119-157) behind the 2D network, in ONE launch for
// gfx950: per-pixel class logits are lifted to every chunk's points through the pixel k-NN, averaged over k and voted into the scene.
//
// The reference does this chunk by chunk: MVPNet2D gathers (1,C,n,k) logits, averages them, and the host adds the chunk's (n,C) means
// into the scene array.  Here the logits of every DISTINCT picked frame lie once in a store; a scene point walks the positions of the
// concatenated chunk lists that name it (the transposed index of mvp_vote_gather_f32), and from a position it is two indirections to the
// logit rows: position -> (chunk, row) -> k pixel ids -> (store frame through the chunk's frame table, pixel).  Neither the gathered
// (n,k,C) rows nor the per-chunk means exist in memory.  No atomics, a fixed order of additions: the same bits every run.
#include "common.h"

namespace {

constexpr int kLVThreads = 256;
constexpr int kLVMaxK = 8;

// A GROUP of G lanes (a power of two, G | 64) owns one scene point; lane g of it owns VEC consecutive classes from g*VEC (VEC = 4: one
// 16-byte load per neighbour row, for a channels-last store; VEC = 1: one dword at c*ld_c, any strides).  A position is resolved ONCE per
// (point, position): the group's first lane finds the next position in ascending order and its chunk and row, lane j of the group reads
// neighbour j's pixel id and the store frame of its view, and the row offsets go round the group by lane shuffles.  All lanes of a group
// run the same trip counts, so every shuffle reads a live lane.
template <int G, int VEC>
__global__ __launch_bounds__(kLVThreads) void lift_vote_kernel(const float* __restrict__ logit, int64_t ld_f, int64_t ld_p, int64_t ld_c, int U,
                                                               int hw, int P /* nv*hw */, int C, const int32_t* __restrict__ view_frame, int nv,
                                                               const int64_t* __restrict__ knn, int k, const int64_t* __restrict__ knn_base,
                                                               const int64_t* __restrict__ chunk_offsets, int num_chunks,
                                                               const int32_t* __restrict__ pt_offsets, const int32_t* __restrict__ pt_slots,
                                                               int64_t n_pts, float* __restrict__ sum, int32_t* __restrict__ cnt) {
  constexpr int kSlots = (kLVMaxK + G - 1) / G;  // neighbours whose offset one lane holds
  const int64_t t = (int64_t)blockIdx.x * kLVThreads + threadIdx.x;
  const int64_t p = t / G;
  if (p >= n_pts) return;  // (whole groups leave: G divides the workgroup)
  const int g = (int)threadIdx.x & (G - 1);
  const int lead = ((int)threadIdx.x & (kWave - 1)) & ~(G - 1);
  const int c0 = g * VEC;
  const bool mine = c0 < C;
  const float kf = (float)k;
  const int lo0 = pt_offsets[p], hi0 = pt_offsets[p + 1];
  float acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
  int prev = -1;
  for (int step = lo0; step < hi0; ++step) {
    int ci = 0, r = 0;
    if (g == 0) {
      int e = 0x7fffffff;
      for (int q = lo0; q < hi0; ++q) {  // smallest position above the previous one (a point's list is short and unordered)
        const int s = pt_slots[q];
        e = (s > prev && s < e) ? s : e;
      }
      prev = e;
      int lo = 0, hi = num_chunks;  // largest i with chunk_offsets[i] <= e
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_offsets[mid] <= (int64_t)e) lo = mid; else hi = mid;
      }
      ci = lo;
      r = (int)((int64_t)e - chunk_offsets[lo]);
    }
    if (G > 1) {
      ci = __shfl(ci, lead, kWave);
      r = __shfl(r, lead, kWave);
    }
    const int64_t row = knn_base[ci] + (int64_t)r;
    int off_lo[kSlots], off_hi[kSlots];  // the neighbour's row offset in the store, -1 = missing
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      const int j = s * G + g;
      int64_t off = -1;
      if (j < k) {
        const int64_t id = knn[row * k + j];
        if (id >= 0 && id < (int64_t)P) {
          const unsigned view = (unsigned)id / (unsigned)hw;
          const unsigned q = (unsigned)id - view * (unsigned)hw;
          const int u = view_frame[ci * nv + (int)view];
          if ((unsigned)u < (unsigned)U) off = (int64_t)u * ld_f + (int64_t)q * ld_p;
        }
      }
      off_lo[s] = (int)(uint32_t)(uint64_t)off;
      off_hi[s] = (int)(uint32_t)((uint64_t)off >> 32);
    }
    float m[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) m[v] = 0.f;
#pragma unroll
    for (int j = 0; j < kLVMaxK; ++j) {
      if (j < k) {
        int ol = off_lo[j / G], oh = off_hi[j / G];
        if (G > 1) {
          ol = __shfl(ol, lead + (j % G), kWave);
          oh = __shfl(oh, lead + (j % G), kWave);
        }
        const int64_t off = (int64_t)(((uint64_t)(uint32_t)oh << 32) | (uint64_t)(uint32_t)ol);
        float l[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) l[v] = 0.f;
        if (mine && off >= 0) {
          if constexpr (VEC == 4) {
            const float4 x = *reinterpret_cast<const float4*>(logit + off + c0);
            l[0] = x.x;
            l[1] = x.y;
            l[2] = x.z;
            l[3] = x.w;
          } else {
            l[0] = logit[off + (int64_t)c0 * ld_c];
          }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) m[v] = j == 0 ? l[v] : m[v] + l[v];
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] += __fdiv_rn(m[v], kf);
  }
  if (mine) {
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(sum + p * C + c0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
      sum[p * C + c0] = acc[0];
    }
  }
  if (g == 0) cnt[p] = hi0 - lo0;
}

}  // namespace

MVP_API int mvp_lift_vote_f32(const float* logit, int64_t ld_f, int64_t ld_p, int64_t ld_c, int64_t U, int64_t hw, int64_t C,
                              const int32_t* view_frame, int64_t nv, const int64_t* knn, int64_t k, const int64_t* knn_base,
                              const int64_t* chunk_offsets, int64_t num_chunks, const int32_t* point_offsets, const int32_t* point_slots,
                              int64_t n_pts, float* sum, int32_t* count, mvp_stream_t stream) {
  MVP_NONNULL(logit);
  MVP_NONNULL(view_frame);
  MVP_NONNULL(knn);
  MVP_NONNULL(knn_base);
  MVP_NONNULL(chunk_offsets);
  MVP_NONNULL(point_offsets);
  MVP_NONNULL(point_slots);
  MVP_NONNULL(sum);
  MVP_NONNULL(count);
  MVP_REQUIRE(k >= 1 && k <= kLVMaxK && C >= 1 && C <= 64 && nv >= 1 && U >= 1 && hw >= 1 && num_chunks >= 1 && n_pts >= 0);
  MVP_REQUIRE(ld_f >= 0 && ld_p >= 0 && ld_c >= 0);
  // what the kernel holds in 32 bits: a pixel id below nv*hw, a store frame below U, the frame table's index below num_chunks*nv, a
  // position and a point number (the transposed index is int32), and the grid's n_pts*G/256 workgroups with G <= 64
  const int64_t lim = 1ll << 31;
  if (hw >= lim || nv >= lim || nv * hw >= lim || U >= lim || num_chunks >= (1ll << 30) || num_chunks * nv >= lim || n_pts >= lim)
    return MVP_EUNSUPPORTED;
  if (n_pts == 0) return MVP_OK;
  const bool vec = C % 4 == 0 && ld_c == 1 && ld_p % 4 == 0 && ld_f % 4 == 0 && (uintptr_t)logit % 16 == 0 && (uintptr_t)sum % 16 == 0;
  const int lanes = (int)(vec ? C / 4 : C);
  int G = 1;
  while (G < lanes) G *= 2;
  const dim3 grid((unsigned)cdiv(n_pts * G, kLVThreads)), block(kLVThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define MVP_LV_LAUNCH(GG, VV)                                                                                                              \
  hipLaunchKernelGGL((lift_vote_kernel<GG, VV>), grid, block, 0, s, logit, ld_f, ld_p, ld_c, (int)U, (int)hw, (int)(nv * hw), (int)C,      \
                     view_frame, (int)nv, knn, (int)k, knn_base, chunk_offsets, (int)num_chunks, point_offsets, point_slots, n_pts, sum,   \
                     count)
  if (vec) {
    switch (G) {
      case 1: MVP_LV_LAUNCH(1, 4); break;
      case 2: MVP_LV_LAUNCH(2, 4); break;
      case 4: MVP_LV_LAUNCH(4, 4); break;
      case 8: MVP_LV_LAUNCH(8, 4); break;
      default: MVP_LV_LAUNCH(16, 4); break;
    }
  } else {
    switch (G) {
      case 1: MVP_LV_LAUNCH(1, 1); break;
      case 2: MVP_LV_LAUNCH(2, 1); break;
      case 4: MVP_LV_LAUNCH(4, 1); break;
      case 8: MVP_LV_LAUNCH(8, 1); break;
      case 16: MVP_LV_LAUNCH(16, 1); break;
      case 32: MVP_LV_LAUNCH(32, 1); break;
      default: MVP_LV_LAUNCH(64, 1); break;
    }
  }
#undef MVP_LV_LAUNCH
  return mvp_launch_status();
}

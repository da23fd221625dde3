// overlap.hip -- what frame selection needs, on the device for gfx950:
//
//   frame_overlap_kernel  : which base points does each RGB-D frame see?  Replaces the offline `compute_rgbd_knn`
//                           (mvpnet/data/preprocess/preprocess.py:99-170: un-project the frame, nearest base point of every pixel in an
//                           open3d KD-tree, mark it when closer than `radius`) by a brute-force scan: the ~2000 base points sit in LDS
//                           as three arrays (12 B per point), one pixel per lane, every lane reads the SAME LDS address per step
//                           (a broadcast, no bank conflict), two points per packed fp32 instruction (46 VALU per 8 pairs).  The workgroup collects
//                           its hits in an LDS bit row and merges the non-zero words into the frame's row with one atomic OR each.
//   select_frames_kernel  : `select_frames` (mvpnet/data/scannet_2d3d.py:20-30) for ALL chunks of a scene in one launch: one
//                           workgroup per chunk, the still-uncovered base points as a bit row in LDS, one frame per lane,
//                           score = sum of popcount(overlap row & uncovered), arg-max with the lowest frame index on ties.
//                           <true>: a training batch -- every chunk with the frame rows of its own scene (mvp_select_frames_ranges_u32).
//
// Measurements: DESIGN.md (scene preparation).
#include "unproject_core.h"
#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// LDS of frame_overlap_kernel: 3 * nbp floats (nbp = nb rounded up to 4) + nbp / 32 (rounded up) bit words.  MVP_OVERLAP_MAX_BASE
// points keep it under the 64 KiB a workgroup gets without opting in to more.
__host__ __device__ inline int overlap_pad4(int nb) { return (nb + 3) & ~3; }
inline size_t overlap_lds_bytes(int nb) { return (size_t)overlap_pad4(nb) * 12 + (size_t)((nb + 31) / 32) * 4; }

// One workgroup = T consecutive pixels of ONE frame (the last tile of a frame is partial), so a frame is spread over
// ceil(h*w / T) workgroups and a single frame still occupies many CUs.
template <typename DepthT, int T>
__global__ __launch_bounds__(T) void frame_overlap_kernel(const DepthT* __restrict__ depth, const float* __restrict__ kinv,
                                                          const float* __restrict__ pose, const float* __restrict__ base, int hw,
                                                          int w, int tiles, int nb, float r2, uint32_t* __restrict__ bits_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char overlap_smem[];
  const int nbp = overlap_pad4(nb);
  const int W = (nb + 31) >> 5;
  float* sx = reinterpret_cast<float*>(overlap_smem);
  float* sy = sx + nbp;
  float* sz = sy + nbp;
  uint32_t* sbits = reinterpret_cast<uint32_t*>(sz + nbp);
  const int f = blockIdx.x / tiles;
  const int tile = blockIdx.x - f * tiles;
  const int tid = threadIdx.x;
  const float* Pm = pose + (size_t)f * 16;
  // a frame whose pose has a non-finite entry is skipped, its row stays zero (preprocess.py:137-139); uniform over the workgroup
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) finite = finite && isfinite(Pm[i]);
  if (!finite) return;
  for (int j = tid; j < nbp; j += T) {  // padding points at +inf: their distance is +inf (or NaN), never below the running minimum
    const bool in = j < nb;
    sx[j] = in ? base[(size_t)j * 3 + 0] : INFINITY;
    sy[j] = in ? base[(size_t)j * 3 + 1] : INFINITY;
    sz[j] = in ? base[(size_t)j * 3 + 2] : INFINITY;
  }
  for (int j = tid; j < W; j += T) sbits[j] = 0u;
  const int pix = tile * T + tid;
  bool valid = pix < hw;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (valid) {
    const int v = pix / w, u = pix - v * w;
    const UnprojectCam cm = unproject_cam(kinv + (size_t)f * 9, Pm);
    double xw, yw, zw, zc;
    unproject_pixel(cm, depth_metres(depth, (size_t)f * hw + pix), u, v, xw, yw, zw, zc);  // = mvp_unproject_* with box = NULL
    px = (float)xw;
    py = (float)yw;
    pz = (float)zw;
    valid = zc > 0.0;
  }
  __syncthreads();
  // Nearest base point, lowest index on ties.  The scan keeps the minimum and the GROUP of four points it came from (v_min3 + v_min
  // + one compare and two selects per four pairs instead of a compare and two selects per pair); the point inside the group is found
  // afterwards by evaluating the group again -- the same instructions on the same operands give the same bits.
  float best = INFINITY;
  int bg = -1;
  if (__any(valid)) {  // a wave of invalid pixels (zero depth, the tail of the last tile) has nothing to search
    const f32x4* sx4 = reinterpret_cast<const f32x4*>(sx);
    const f32x4* sy4 = reinterpret_cast<const f32x4*>(sy);
    const f32x4* sz4 = reinterpret_cast<const f32x4*>(sz);
    const int groups = nbp >> 2;
    const f32x2 PX = {px, px}, PY = {py, py}, PZ = {pz, pz};
#pragma unroll 2
    for (int g = 0; g < groups; ++g) {
      const f32x4 X = sx4[g], Y = sy4[g], Z = sz4[g];
      // two points per instruction (v_pk_add / v_pk_mul: each half rounds like the scalar form, nothing fuses): the pixel's coordinate
      // sits in BOTH halves of a register pair, so no source swizzle (op_sel) is needed -- Makefile, NO_SLP
      const f32x2 a = dist2_3(PX, PY, PZ, f32x2{X.x, X.y}, f32x2{Y.x, Y.y}, f32x2{Z.x, Z.y});
      const f32x2 b = dist2_3(PX, PY, PZ, f32x2{X.z, X.w}, f32x2{Y.z, Y.w}, f32x2{Z.z, Z.w});
      const float d0 = a.x, d1 = a.y, d2 = b.x, d3 = b.y;
      const float m = fminf(fminf(fminf(d0, d1), d2), d3);
      const bool lt = m < best;  // strict: an equal later group does not replace an earlier one
      best = lt ? m : best;
      bg = lt ? g : bg;
    }
  }
  if (valid && bg >= 0 && best < r2) {  // strict, like the ball query: d2 < fl32(radius * radius)
    int j = bg << 2;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (dist2_3(px, py, pz, sx[j], sy[j], sz[j]) == best) break;
      ++j;
    }
    atomicOr(&sbits[j >> 5], 1u << (j & 31));
  }
  __syncthreads();
  uint32_t* row = bits_out + (size_t)f * W;
  for (int j = tid; j < W; j += T) {
    const uint32_t b = sbits[j];
    if (b) atomicOr(&row[j], b);
  }
}

// ---- greedy frame selection ---------------------------------------------------------------------------------------------------
constexpr int kSelThreads = 256;
constexpr int kSelMaxWords = 1024;  // 32768 base points

// RANGED: chunk c chooses among rows [frame_begin[c], frame_begin[c] + frame_count[c]) of a matrix that holds several scenes' frames
// (cut to [0, F); the lane's frame index is local to the range, so ties still go to the lowest row) and reports global rows.
template <bool RANGED>
__global__ __launch_bounds__(kSelThreads) void select_frames_kernel(const uint32_t* __restrict__ overlap,
                                                                   const uint32_t* __restrict__ chunk_bits, int F, int W, int n_pick,
                                                                   const int64_t* __restrict__ frame_begin,
                                                                   const int64_t* __restrict__ frame_count,
                                                                   int64_t* __restrict__ picked, int32_t* __restrict__ gain) {
  __shared__ uint32_t unc[kSelMaxWords];
  __shared__ unsigned long long wbest[kSelThreads / kWave];
  const int c = blockIdx.x, tid = threadIdx.x;
  int64_t f0 = 0;
  if (RANGED) {
    f0 = frame_begin[c];
    f0 = f0 < 0 ? 0 : (f0 > F ? F : f0);
    int64_t cnt = frame_count[c];
    cnt = cnt < 0 ? 0 : (cnt > F - f0 ? F - f0 : cnt);
    F = (int)cnt;
    overlap += (size_t)f0 * W;
    if (F < 1) {  // (uniform over the workgroup) no frame to choose from: the caller's error, answered without reading a row
      for (int pick = tid; pick < n_pick; pick += kSelThreads) {
        picked[(size_t)c * n_pick + pick] = -1;
        if (gain) gain[(size_t)c * n_pick + pick] = 0;
      }
      return;
    }
  }
  for (int j = tid; j < W; j += kSelThreads) unc[j] = chunk_bits[(size_t)c * W + j];
  __syncthreads();
  for (int pick = 0; pick < n_pick; ++pick) {
    // key = score in the high word, ~frame in the low one: the maximum key is the highest score and, among equal scores, the
    // LOWEST frame index (numpy.argmax; with all scores zero that is frame 0, pick after pick)
    unsigned long long key = 0ull;
    for (int f = tid; f < F; f += kSelThreads) {
      const uint32_t* row = overlap + (size_t)f * W;
      unsigned score = 0;
      for (int j = 0; j < W; ++j) score += __popc(row[j] & unc[j]);
      const unsigned long long k = ((unsigned long long)score << 32) | (unsigned)(~(unsigned)f);
      key = k > key ? k : key;
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      const unsigned long long o = __shfl_xor(key, m, kWave);
      key = o > key ? o : key;
    }
    if ((tid & (kWave - 1)) == 0) wbest[tid / kWave] = key;
    __syncthreads();
    key = wbest[0];
#pragma unroll
    for (int i = 1; i < kSelThreads / kWave; ++i) key = wbest[i] > key ? wbest[i] : key;
    const int fb = (int)(~(unsigned)key);
    if (tid == 0) {
      picked[(size_t)c * n_pick + pick] = f0 + fb;
      if (gain) gain[(size_t)c * n_pick + pick] = (int32_t)(key >> 32);
    }
    const uint32_t* row = overlap + (size_t)fb * W;
    for (int j = tid; j < W; j += kSelThreads) unc[j] &= ~row[j];
    __syncthreads();  // unc and wbest are rewritten by the next pick
  }
}

template <typename DepthT>
int frame_overlap_entry(const DepthT* depth, const float* kinv, const float* pose, const float* base, int64_t F, int64_t h, int64_t w,
                        int64_t nb, float radius, uint32_t* bits, mvp_stream_t stream) {
  MVP_NONNULL(depth);
  MVP_NONNULL(kinv);
  MVP_NONNULL(pose);
  MVP_NONNULL(base);
  MVP_NONNULL(bits);
  // each factor is bounded before it enters a product: no int64 product here can overflow
  MVP_REQUIRE(F >= 0 && F < (1ll << 31) && h > 0 && h < (1ll << 31) && w > 0 && w < (1ll << 31) && nb > 0);
  MVP_REQUIRE(h * w < (1ll << 31));
  MVP_REQUIRE(F * (h * w) < (1ll << 31));
  MVP_REQUIRE(radius >= 0.f);  // (false for NaN)
  if (nb > MVP_OVERLAP_MAX_BASE) return MVP_EUNSUPPORTED;
  if (F == 0) return MVP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t W = (nb + 31) / 32;
  hipError_t e = hipMemsetAsync(bits, 0, sizeof(uint32_t) * (size_t)(F * W), s);
  if (e != hipSuccess) return (int)e;
  const float r2 = radius * radius;  // fl32(fl32(radius) * fl32(radius))
  const int hw = (int)(h * w);
  const size_t lds = overlap_lds_bytes((int)nb);
  // 256 pixels per workgroup when that still gives every CU a few workgroups, 64 otherwise (few frames)
  if (F * cdiv(hw, 256) >= 1024) {
    const int tiles = (int)cdiv(hw, 256);
    hipLaunchKernelGGL((frame_overlap_kernel<DepthT, 256>), dim3((unsigned)(F * tiles)), dim3(256), lds, s, depth, kinv, pose, base, hw,
                       (int)w, tiles, (int)nb, r2, bits);
  } else {
    const int tiles = (int)cdiv(hw, 64);
    hipLaunchKernelGGL((frame_overlap_kernel<DepthT, 64>), dim3((unsigned)(F * tiles)), dim3(64), lds, s, depth, kinv, pose, base, hw,
                       (int)w, tiles, (int)nb, r2, bits);
  }
  return mvp_launch_status();
}

}  // namespace

MVP_API int mvp_frame_overlap_f32(const float* depth_m, const float* kinv, const float* pose, const float* base_points, int64_t F,
                                  int64_t h, int64_t w, int64_t nb, float radius, uint32_t* overlap_bits, mvp_stream_t stream) {
  return frame_overlap_entry<float>(depth_m, kinv, pose, base_points, F, h, w, nb, radius, overlap_bits, stream);
}
MVP_API int mvp_frame_overlap_u16(const uint16_t* depth_mm, const float* kinv, const float* pose, const float* base_points, int64_t F,
                                  int64_t h, int64_t w, int64_t nb, float radius, uint32_t* overlap_bits, mvp_stream_t stream) {
  return frame_overlap_entry<uint16_t>(depth_mm, kinv, pose, base_points, F, h, w, nb, radius, overlap_bits, stream);
}

MVP_API int mvp_select_frames_u32(const uint32_t* overlap_bits, const uint32_t* chunk_bits, int64_t F, int64_t C, int64_t W,
                                  int64_t n_pick, int64_t* picked, int32_t* gain, mvp_stream_t stream) {
  MVP_NONNULL(overlap_bits);
  MVP_NONNULL(chunk_bits);
  MVP_NONNULL(picked);
  MVP_REQUIRE(F >= 1 && F < (1ll << 31) && C >= 0 && C < (1ll << 31) && W >= 1 && n_pick >= 0 && n_pick < (1ll << 31));
  if (W > kSelMaxWords) return MVP_EUNSUPPORTED;
  if (C == 0 || n_pick == 0) return MVP_OK;
  hipLaunchKernelGGL(select_frames_kernel<false>, dim3((unsigned)C), dim3(kSelThreads), 0, static_cast<hipStream_t>(stream), overlap_bits,
                     chunk_bits, (int)F, (int)W, (int)n_pick, nullptr, nullptr, picked, gain);
  return mvp_launch_status();
}

MVP_API int mvp_select_frames_ranges_u32(const uint32_t* overlap_bits, const uint32_t* chunk_bits, const int64_t* frame_begin,
                                         const int64_t* frame_count, int64_t Ftot, int64_t C, int64_t W, int64_t n_pick, int64_t* picked,
                                         int32_t* gain, mvp_stream_t stream) {
  MVP_NONNULL(overlap_bits);
  MVP_NONNULL(chunk_bits);
  MVP_NONNULL(frame_begin);
  MVP_NONNULL(frame_count);
  MVP_NONNULL(picked);
  MVP_REQUIRE(Ftot >= 1 && Ftot < (1ll << 31) && C >= 0 && C < (1ll << 31) && W >= 1 && n_pick >= 0 && n_pick < (1ll << 31));
  if (W > kSelMaxWords) return MVP_EUNSUPPORTED;
  if (C == 0 || n_pick == 0) return MVP_OK;
  hipLaunchKernelGGL(select_frames_kernel<true>, dim3((unsigned)C), dim3(kSelThreads), 0, static_cast<hipStream_t>(stream), overlap_bits,
                     chunk_bits, (int)Ftot, (int)W, (int)n_pick, frame_begin, frame_count, picked, gain);
  return mvp_launch_status();
}

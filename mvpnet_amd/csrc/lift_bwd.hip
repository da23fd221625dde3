// lift_bwd.hip -- gradient of the 2D->3D lift with respect to the 2D feature map, as a gather (gfx950).
//
//   grad_feature[b,j,:] = (+0.0f) + grad_gfeature[b,e_1,:] + grad_gfeature[b,e_2,:] + ...   over the e (= n*k + slot) with index[b,e] == j,
//   e_1 < e_2 < ..., plain float32 additions, one rounding each.
//
// mvp_lift_gather_backward_f32 (lifting.hip) zero-fills the map and adds every element with a float atomic: the result depends on the
// order in which the adds arrive.  Here the index is transposed first -- for every pixel the ascending list of the positions that name it
// -- and the map is then written once, row by row, by lanes that walk their pixel's list: no fill, no float atomics, and the result is a
// function of the inputs.  Two launches:
//   lift_bwd_build_kernel   offsets (B,P+1) and slots (B,E) int32 in the workspace.  A chunk has P = nv*h*w pixels (57 600 at the
//                           workload shape, 384 000 at the dense one): more counters than one workgroup's LDS holds, so a chunk is cut
//                           into ranges of kRange pixels and one workgroup builds one range.  It reads ALL of the chunk's E indices (twice:
//                           count, fill; E is 24 576 at the workload shape, the reads come from L2), keeps the counters and cursors of its
//                           range in LDS, and finds where its lists start in the chunk's slot array by counting the valid indices below its
//                           range on the way -- so there is no pass over the whole chunk, no global counter and no zero fill of anything.
//                           The LDS atomics leave a list in arrival order; every list of more than four entries is then sorted ascending
//                           (below), the shorter ones are ordered by the gather in registers.
//   lift_bwd_gather_kernel  one lane per (2 pixels, 4 channels) -- or per (2 pixels, channel) when C % 4 != 0 --: the sums above, each stored once.
#include <type_traits>

#include "common.h"

namespace {

constexpr int kBT = 1024;        // threads of a build workgroup
constexpr int kRange = 8192;     // pixels (LDS counters) of a build workgroup
constexpr int kGatherList = 4;   // lists up to here stay in arrival order: the gather loads their positions at once and orders them itself
constexpr int kRegList = 16;     // lists up to here are sorted in registers by the lane that owns the pixel
constexpr int kWaveList = 128;   // lists up to here are rank-sorted by one wave through LDS; longer ones are rebuilt in order (below)
constexpr int kGT = 256;         // threads of a gather workgroup

__global__ __launch_bounds__(kBT) void lift_bwd_build_kernel(const int64_t* __restrict__ idx, int64_t E, int P, int* __restrict__ offsets,
                                                             int* __restrict__ slots) {
  __shared__ int cnt[kRange];                          // counts, then running cursors, then the lists' ends (relative to `base`)
  __shared__ int part[kBT / kWave];                    // the waves' scan totals; later their hit counts in the ordered rebuild
  __shared__ unsigned short queue[kRange];             // pixels (range-local) whose list is longer than kRegList
  __shared__ int wbuf[kBT / kWave][kWaveList];         // one list per wave
  __shared__ int s_below, s_queued;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int lo = blockIdx.x * kRange;                  // this workgroup's pixels: [lo, lo + R)
  const int R = min(kRange, P - lo);
  const int64_t* ix = idx + (size_t)b * E;
  int* o = offsets + (size_t)b * ((size_t)P + 1);
  int* sl = slots + (size_t)b * E;
  for (int i = tid; i < kRange; i += kBT) cnt[i] = 0;
  if (tid == 0) {
    s_below = 0;
    s_queued = 0;
  }
  __syncthreads();
  // a pass over the chunk's index: sixteen 16-byte loads (32 entries) in flight per lane -- a workgroup reads the whole chunk, 160
  // entries per lane and pass at the dense shape, and the passes are chains of load -> LDS atomic (cf. csr_build_lds_kernel, rows.hip)
  constexpr int kU = 16;
  const bool pairs = (E & 1) == 0 && (reinterpret_cast<uintptr_t>(ix) & 15) == 0;
  auto for_entries = [&](auto&& fn) {
    if (pairs) {
      const longlong2* ix2 = reinterpret_cast<const longlong2*>(ix);
      const int64_t E2 = E >> 1;
      for (int64_t e0 = tid; e0 < E2; e0 += kU * kBT) {
        longlong2 j[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) j[u] = e0 + u * kBT < E2 ? ix2[e0 + u * kBT] : longlong2{-1, -1};
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          fn((int64_t)j[u].x, 2 * (e0 + u * kBT));
          fn((int64_t)j[u].y, 2 * (e0 + u * kBT) + 1);
        }
      }
    } else {
      for (int64_t e0 = tid; e0 < E; e0 += 4 * kBT) {
        int64_t j[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) j[u] = e0 + u * kBT < E ? ix[e0 + u * kBT] : -1;
#pragma unroll
        for (int u = 0; u < 4; ++u) fn(j[u], e0 + u * kBT);
      }
    }
  };
  int below = 0;  // valid indices below this range: where the range's lists start in the chunk's slot array
  for_entries([&](int64_t j, int64_t) {
    if (j >= 0 && j < lo) ++below;
    if (j >= lo && j < (int64_t)lo + R) atomicAdd(&cnt[(int)(j - lo)], 1);
  });
  if (below) atomicAdd(&s_below, below);
  __syncthreads();
  const int base = s_below;
  // exclusive scan of cnt over contiguous runs of kRange / kBT pixels per thread: inside a wave by shuffles, across the waves through LDS
  constexpr int kPer = kRange / kBT;
  const int j0 = tid * kPer;
  int sum = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) sum += cnt[j0 + i];
  int incl = sum;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int v = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += v;
  }
  if (lane == kWave - 1) part[wave] = incl;
  __syncthreads();
  int run = incl - sum;  // exclusive inside the wave
  for (int w = 0; w < wave; ++w) run += part[w];
  if (lo == 0 && tid == 0) o[0] = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int c = cnt[j0 + i];
    cnt[j0 + i] = run;  // cursor = start of the list
    run += c;
    if (j0 + i < R) o[lo + j0 + i + 1] = base + run;
  }
  __syncthreads();
  for_entries([&](int64_t j, int64_t e) {
    if (j >= lo && j < (int64_t)lo + R) sl[base + atomicAdd(&cnt[(int)(j - lo)], 1)] = (int)e;
  });
  __syncthreads();  // (workgroup scope: the slots written above are read back below by other lanes of THIS workgroup)
  // ---- ascending positions inside every list ----
  // up to kGatherList entries (the usual case: a pixel is named once or twice): left as they are, the gather orders them; up to kRegList:
  // in registers, by the lane that owns the pixel; the others are queued
  for (int j = tid; j < R; j += kBT) {
    const int p1 = cnt[j];                                                                                // the cursor ended at the list's end
    const int p0 = j ? __hip_atomic_load(&cnt[j - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;  // = the end of the list before
    const int n = p1 - p0;
    if (n <= kGatherList) continue;
    if (n > kRegList) {
      queue[atomicAdd(&s_queued, 1)] = (unsigned short)j;
      continue;
    }
    int* l = sl + base + p0;
    int v[kRegList];
#pragma unroll
    for (int i = 0; i < kRegList; ++i) v[i] = i < n ? l[i] : 0x7fffffff;
#pragma unroll
    for (int r = 0; r < kRegList; ++r)  // odd-even transposition network
#pragma unroll
      for (int i = r & 1; i + 1 < kRegList; i += 2) {
        const int a = min(v[i], v[i + 1]), c = max(v[i], v[i + 1]);
        v[i] = a;
        v[i + 1] = c;
      }
#pragma unroll
    for (int i = 0; i < kRegList; ++i)
      if (i < n) l[i] = v[i];
  }
  __syncthreads();
  const int queued = s_queued;
  // lists of kRegList + 1 .. kWaveList entries: one wave per list.  The positions of a list are distinct, so an entry's place is the number
  // of entries below it.  (Every wave makes the same number of trips: the barriers are the workgroup's.)
  for (int q0 = 0; q0 < queued; q0 += kBT / kWave) {
    const int q = q0 + wave;
    int p0 = 0, n = 0;
    if (q < queued) {
      const int j = queue[q];
      p0 = j ? cnt[j - 1] : 0;
      n = cnt[j] - p0;
      if (n > kWaveList) n = 0;  // left to the rebuild below
    }
    int* l = sl + base + p0;
    int v[kWaveList / kWave];
#pragma unroll
    for (int u = 0; u < kWaveList / kWave; ++u) {
      v[u] = lane + u * kWave < n ? l[lane + u * kWave] : 0x7fffffff;
      wbuf[wave][lane + u * kWave] = v[u];
    }
    __syncthreads();
    int rank[kWaveList / kWave];
#pragma unroll
    for (int u = 0; u < kWaveList / kWave; ++u) rank[u] = 0;
    for (int i = 0; i < n; ++i) {
      const int x = wbuf[wave][i];
#pragma unroll
      for (int u = 0; u < kWaveList / kWave; ++u) rank[u] += x < v[u] ? 1 : 0;
    }
#pragma unroll
    for (int u = 0; u < kWaveList / kWave; ++u)
      if (lane + u * kWave < n) l[rank[u]] = v[u];  // rank < n: inside the list
    __syncthreads();
  }
  // longer lists, of any length (every edge of a chunk may name one pixel): the workgroup rebuilds the list in order from the index
  // itself -- a stable compaction of the positions e with index[e] == pixel, kBT positions per trip.
  for (int q = 0; q < queued; ++q) {
    const int j = queue[q];
    const int p0 = j ? cnt[j - 1] : 0;
    const int n = cnt[j] - p0;
    if (n <= kWaveList) continue;  // (uniform: every thread reads the same queue entry)
    int* l = sl + base + p0;
    const int64_t pixel = (int64_t)lo + j;
    int done = 0;
    for (int64_t e0 = 0; e0 < E && done < n; e0 += kBT) {
      const int64_t e = e0 + tid;
      const bool hit = e < E && ix[e] == pixel;
      const unsigned long long m = __ballot(hit);
      if (lane == 0) part[wave] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kBT / kWave; ++w) {
        const int c = part[w];
        before += w < wave ? c : 0;
        total += c;
      }
      if (hit) l[done + before + __popcll(m & ((1ull << lane) - 1ull))] = (int)e;  // done + before + rank < n: the list holds n hits in all
      done += total;
      __syncthreads();
    }
  }
}

// One lane per (kGU pixels, 4 channels) [VEC] or per (kGU pixels, channel); the kGU pixels lie half a map apart, so every load and
// store stream of a wave stays contiguous.  A list is a chain of three dependent loads (offsets -> positions -> rows) in front of one
// store, and the kernel mostly waits on it: a lane keeps the chains of kGU pixels, and the first kGatherList rows of each, in flight
// together (measured at the workload / dense shape, both launches: one pixel per lane 235 / 127 us, two 216 / 118, four 246 / 126).
// The first kGatherList positions are ordered here in registers (the build leaves such short lists in arrival order; of a longer,
// sorted list they are the first four and stay where they are), the additions run in list order, the rest of a longer list follows
// entry by entry.  E == 0: no list was built (offsets is not read), every row is +0.0f.
constexpr int kGU = 2;
__device__ __forceinline__ void add_row(float4& acc, const float4& a) {
  acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
}
__device__ __forceinline__ void add_row(float& acc, const float& a) { acc += a; }
__device__ __forceinline__ void zero_row(float4& acc) { acc = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void zero_row(float& acc) { acc = 0.f; }
__device__ __forceinline__ void order2(int& a, int& b) {
  const int lo = min(a, b), hi = max(a, b);
  a = lo;
  b = hi;
}

template <bool VEC>
__global__ __launch_bounds__(kGT) void lift_bwd_gather_kernel(const float* __restrict__ ggf, const int* __restrict__ offsets,
                                                              const int* __restrict__ slots, int P, int C, int64_t E,
                                                              float* __restrict__ gfeat) {
  static_assert(kGatherList == 4, "the ordering network below takes four positions");
  using Row = typename std::conditional<VEC, float4, float>::type;
  const int b = blockIdx.y;
  const int L = VEC ? C >> 2 : C;  // lanes per pixel
  const int Q = (P + kGU - 1) / kGU;  // pixels per part of the map
  const int64_t t = (int64_t)blockIdx.x * kGT + threadIdx.x;
  const int64_t q = t / L;
  const int c = (int)(t - q * L) * (VEC ? 4 : 1);
  if (q >= Q) return;
  const int* o = offsets + (size_t)b * ((size_t)P + 1);
  const int* sl = slots + (size_t)b * E;
  const float* g = ggf + (size_t)b * E * C + c;
  int p0[kGU], n[kGU];
#pragma unroll
  for (int u = 0; u < kGU; ++u) {
    const int64_t j = q + (int64_t)u * Q;
    const bool ok = j < P && E > 0;
    p0[u] = ok ? o[j] : 0;
    n[u] = ok ? o[j + 1] - p0[u] : 0;
  }
  int e[kGU][kGatherList];
#pragma unroll
  for (int u = 0; u < kGU; ++u)
#pragma unroll
    for (int i = 0; i < kGatherList; ++i) e[u][i] = i < n[u] ? sl[p0[u] + i] : 0x7fffffff;
#pragma unroll
  for (int u = 0; u < kGU; ++u) {
    order2(e[u][0], e[u][1]);
    order2(e[u][2], e[u][3]);
    order2(e[u][0], e[u][2]);
    order2(e[u][1], e[u][3]);
    order2(e[u][1], e[u][2]);
  }
  Row a[kGU][kGatherList];
#pragma unroll
  for (int u = 0; u < kGU; ++u)
#pragma unroll
    for (int i = 0; i < kGatherList; ++i)
      if (i < n[u]) a[u][i] = *reinterpret_cast<const Row*>(g + (size_t)e[u][i] * C);
#pragma unroll
  for (int u = 0; u < kGU; ++u) {
    const int64_t j = q + (int64_t)u * Q;
    if (j >= P) continue;
    Row acc;
    zero_row(acc);  // +0.0f
#pragma unroll
    for (int i = 0; i < kGatherList; ++i)
      if (i < n[u]) add_row(acc, a[u][i]);
    for (int p = p0[u] + kGatherList; p < p0[u] + n[u]; ++p) add_row(acc, *reinterpret_cast<const Row*>(g + (size_t)sl[p] * C));
    *reinterpret_cast<Row*>(gfeat + ((size_t)b * P + j) * C + c) = acc;
  }
}

}  // namespace

MVP_API int64_t mvp_lift_backward_workspace_bytes(int64_t B, int64_t P, int64_t N, int64_t k) {
  if (B < 0 || P < 0 || N < 0 || k < 0 || B >= 65536 || P >= (1ll << 31) || (k > 0 && N >= ((1ll << 31) + k - 1) / k)) return 0;
  // offsets (B,P+1) int32, slots (B,N*k) int32
  return (4 * B * (P + 1 + N * k) + 15) & ~(int64_t)15;
}

MVP_API int mvp_lift_backward_f32(const float* grad_gfeature, const int64_t* index, int64_t B, int64_t P, int64_t C, int64_t N, int64_t k,
                                  void* workspace, float* grad_feature, mvp_stream_t stream) {
  MVP_NONNULL(grad_gfeature);
  MVP_NONNULL(index);
  MVP_NONNULL(workspace);
  MVP_NONNULL(grad_feature);
  MVP_REQUIRE(B >= 0 && P > 0 && C >= 0 && N >= 0 && k >= 0 && C < (1ll << 20));
  MVP_REQUIRE(((uintptr_t)workspace % 16) == 0 && ((uintptr_t)grad_gfeature % 4) == 0 && ((uintptr_t)grad_feature % 4) == 0 &&
              ((uintptr_t)index % 8) == 0);
  // positions and pixels are 32-bit in the workspace and in the kernels; a chunk is blockIdx.y
  if (B >= 65536 || P >= (1ll << 31) || (k > 0 && N >= ((1ll << 31) + k - 1) / k)) return MVP_EUNSUPPORTED;
  const int64_t E = N * k;
  if (B == 0 || C == 0) return MVP_OK;
  const bool vec = (C % 4 == 0) && ((uintptr_t)grad_gfeature % 16 == 0) && ((uintptr_t)grad_feature % 16 == 0);
  const int64_t gather_blocks = cdiv(cdiv(P, kGU) * (vec ? C / 4 : C), kGT);
  if (gather_blocks >= (1ll << 31)) return MVP_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* offsets = static_cast<int*>(workspace);
  int* slots = offsets + B * (P + 1);
  if (E > 0) {
    hipLaunchKernelGGL(lift_bwd_build_kernel, dim3((unsigned)cdiv(P, kRange), (unsigned)B), dim3(kBT), 0, s, index, E, (int)P, offsets, slots);
    const int rc = mvp_launch_status();
    if (rc != MVP_OK) return rc;
  }
  const dim3 grid((unsigned)gather_blocks, (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(lift_bwd_gather_kernel<true>, grid, dim3(kGT), 0, s, grad_gfeature, offsets, slots, (int)P, (int)C, E, grad_feature);
  else
    hipLaunchKernelGGL(lift_bwd_gather_kernel<false>, grid, dim3(kGT), 0, s, grad_gfeature, offsets, slots, (int)P, (int)C, E, grad_feature);
  return mvp_launch_status();
}

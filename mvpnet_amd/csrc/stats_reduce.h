// stats_reduce.h -- reduction of per-workgroup partial column statistics (shared by mlp.hip and rows.hip).
#pragma once
#include "common.h"

namespace {

// Sum the per-row-tile partial statistics (nblk x 2*Cout, written by the producing kernel) into stat.
// With one atomic pair per (workgroup, column) up to 16 k workgroups queued on the same 2*Cout
// addresses (measured: 370 -> 215 us on a 2.1 M-row C=32 layer once that queue is gone).
//
// Two-dimensional grid: blockIdx.x = column slice, blockIdx.y = row group.  A workgroup owns kSrCols = 16 columns -- one 128-byte
// line of every partial row -- and one of G = gridDim.y row groups; its 256 lanes are 16 column-lanes x 16 row-lanes.  Every lane issues
// kSrDepth independent loads before its first add (a group of up to 16 * kSrDepth rows is ONE load round), the row-lanes are summed
// through LDS, and ONE fp64 atomic per column leaves the workgroup: G atomics queue per result address (~90 ns each, see
// colstats_kernel in rows.hip), where the one-dimensional split queued up to 128 and walked its rows in dependent 4-deep rounds.
constexpr int kSrCols = 16;      // columns per workgroup (16 doubles = one 128-byte line per partial row)
constexpr int kSrRowLanes = 16;  // row-lanes per column
constexpr int kSrDepth = 8;      // loads in flight per lane
constexpr int kSrMaxGroups = 16; // most row groups (= atomics per result address)
static_assert(kSrCols * kSrRowLanes == 256 && kSrCols == 16 && kSrRowLanes == 16, "lane layout of stats_reduce_slice");
static_assert(kSrDepth == 8, "the pairwise sum in stats_reduce_slice is written for 8 loads");

// One workgroup's share: columns 16 * blockIdx.x .., partial rows of row group blockIdx.y.  red: 4 x 16 doubles of LDS.
__device__ __forceinline__ void stats_reduce_slice(const double* __restrict__ partial, int64_t nblk, int C2, double* __restrict__ stat,
                                                   double (*red)[kSrCols]) {
  const int cl = threadIdx.x & (kSrCols - 1), rl = threadIdx.x >> 4;
  const int c = (int)blockIdx.x * kSrCols + cl;
  const int64_t per = (nblk + gridDim.y - 1) / gridDim.y;
  const int64_t t0 = (int64_t)blockIdx.y * per, t1 = min(nblk, t0 + per);
  double acc = 0.0;
  if (c < C2) {
    const double* p = partial + c;
    for (int64_t t = t0 + rl; t < t1; t += kSrRowLanes * kSrDepth) {
      double v[kSrDepth];
#pragma unroll
      for (int j = 0; j < kSrDepth; ++j) {  // rows past the end re-read the last row (in bounds) and count as zero: no branch between the loads
        const int64_t tj = t + (int64_t)j * kSrRowLanes;
        const double x = p[(size_t)min(tj, t1 - 1) * C2];
        v[j] = tj < t1 ? x : 0.0;
      }
      acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
  }
  // row-lanes: lanes 16 and 32 apart inside the wave, then the four waves through LDS
  acc += __shfl_xor(acc, 16, kWave);
  acc += __shfl_xor(acc, 32, kWave);
  if ((threadIdx.x & (kWave - 1)) < kSrCols) red[threadIdx.x >> 6][cl] = acc;
  __syncthreads();
  if (threadIdx.x < kSrCols && c < C2 && t1 > t0) atomicAdd(stat + c, (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]));
}

// Grid for nblk partial rows of C2 columns: (column slices, row groups), one row group per load round (16 row-lanes x kSrDepth rows) up to
// kSrMaxGroups (measured in the B = 32 step, profiles/small_reductions.txt: caps of 4 .. 16 give the same 5 - 7 us per launch, 32 and 64
// a little more for the finalize form, whose workgroups all draw their ticket on one address).  No rows (the producer added to `stat` itself and only the finalize is wanted):
// one workgroup.
static inline dim3 stats_reduce_grid(int64_t nblk, int C2) {
  if (nblk <= 0) return dim3(1, 1);
  const int64_t g = cdiv(nblk, kSrRowLanes * kSrDepth);
  return dim3((unsigned)cdiv(C2, kSrCols), (unsigned)(g > kSrMaxGroups ? kSrMaxGroups : g));
}

__global__ __launch_bounds__(256) void stats_reduce_kernel(const double* __restrict__ partial, int64_t nblk, int C2,
                                                           double* __restrict__ stat) {
  __shared__ double red[4][kSrCols];
  stats_reduce_slice(partial, nblk, C2, stat, red);
}


// BatchNorm "finalize" carried by the reduction itself: the LAST workgroup of stats_reduce_finalize_kernel (ticket counter) turns the
// completed sums into mean / invstd and moves the running statistics -- the separate bn_finalize launch (25 per training step, ~5 us
// each plus the launch gap) disappears.  Same arithmetic as bn_finalize_kernel (rows.hip).
struct BnFinalize {
  int64_t rows;        // R: statistics are over this many rows
  float eps, momentum;
  float* mean;         // (C) out
  float* invstd;       // (C) out
  float* running_mean; // (C) in/out or nullptr
  float* running_var;
  int64_t* num_batches_tracked;  // or nullptr
};

// The launch's completion counter lives in the CALLER's memory: stat[C2] (one extra float64 behind the 2*Cout sums, zero on entry like
// the sums, left zero again by the last workgroup).  No static device state, nothing shared between launches, streams, threads or graphs.
__global__ __launch_bounds__(256) void stats_reduce_finalize_kernel(const double* __restrict__ partial, int64_t nblk, int C2,
                                                                    double* __restrict__ stat, BnFinalize fin) {
  __shared__ double red[4][kSrCols];
  __shared__ unsigned last;
  stats_reduce_slice(partial, nblk, C2, stat, red);
  // ---- last workgroup: finalize.  No __threadfence(): at device scope it writes back and invalidates the XCD's whole L2, once per
  // workgroup here.  What crosses workgroups are the device-scope atomics on `stat` above and the device-scope loads below; every lane
  // waits for ITS atomics to have been performed (wait_vm_complete) before the barrier, so the ticket drawn after the barrier is
  // ordered behind all of this workgroup's adds whatever channel they went to.
  wait_vm_complete();
  __syncthreads();
  unsigned* ticket = reinterpret_cast<unsigned*>(stat + C2);
  if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x * gridDim.y - 1 ? 1u : 0u;
  __syncthreads();
  if (!last) return;
  const int C = C2 / 2;
  for (int c = threadIdx.x; c < C; c += 256) {
    const double s1 = __hip_atomic_load(stat + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double s2 = __hip_atomic_load(stat + C + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double m = s1 / (double)fin.rows;
    double var = s2 / (double)fin.rows - m * m;
    if (var < 0.0) var = 0.0;
    fin.mean[c] = (float)m;
    fin.invstd[c] = (float)(1.0 / sqrt(var + (double)fin.eps));
    if (fin.running_mean) {
      const double unbiased = fin.rows > 1 ? var * ((double)fin.rows / (double)(fin.rows - 1)) : var;
      fin.running_mean[c] = (float)((1.0 - fin.momentum) * (double)fin.running_mean[c] + fin.momentum * m);
      fin.running_var[c] = (float)((1.0 - fin.momentum) * (double)fin.running_var[c] + fin.momentum * unbiased);
    }
  }
  if (threadIdx.x == 0) {
    if (fin.num_batches_tracked) *fin.num_batches_tracked += 1;
    *ticket = 0u;  // the caller's buffer is all sums again
  }
}

static inline void launch_stats_reduce_finalize(const double* partial, int64_t nblk, int C2, double* stat, const BnFinalize& fin, hipStream_t s) {
  hipLaunchKernelGGL(stats_reduce_finalize_kernel, stats_reduce_grid(nblk, C2), dim3(256), 0, s, partial, nblk, C2, stat, fin);
}

static inline void launch_stats_reduce(const double* partial, int64_t nblk, int C2, double* stat, hipStream_t s) {
  hipLaunchKernelGGL(stats_reduce_kernel, stats_reduce_grid(nblk, C2), dim3(256), 0, s, partial, nblk, C2, stat);
}

}  // namespace

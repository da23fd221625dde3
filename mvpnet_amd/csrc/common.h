// common.h -- shared device helpers for libmvp_hip.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mvp_hip.h"

#define MVP_API extern "C" __attribute__((visibility("default")))

#define MVP_REQUIRE(cond)            \
  do {                               \
    if (!(cond)) return MVP_EINVAL;  \
  } while (0)
#define MVP_NONNULL(p)               \
  do {                               \
    if ((p) == nullptr) return MVP_ENULL; \
  } while (0)

static inline int mvp_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MVP_OK : (int)e;
}

constexpr int kWave = 64;  // CDNA wavefront

// Pinned squared distance: (dx*dx + dy*dy) + dz*dz, each op rounded once.
// The library is compiled with -ffp-contract=off, so these never fuse into FMA.
template <typename T>
__device__ __forceinline__ T dist2_3(T ax, T ay, T az, T bx, T by, T bz) {
  T dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}
template <typename T>
__device__ __forceinline__ T dist2_2(T ax, T ay, T bx, T by) {
  T dx = ax - bx, dy = ay - by;
  return dx * dx + dy * dy;
}

template <typename T>
__device__ __forceinline__ T shfl_xor_t(T v, int m) {
  return __shfl_xor(v, m, kWave);
}
template <>
__device__ __forceinline__ double shfl_xor_t<double>(double v, int m) {
  return __shfl_xor(v, m, kWave);
}

// Completion wait for everything this lane has issued to memory so far.  On gfx9-family ISAs stores and NON-returning atomics count in
// vmcnt like loads do, and the count drops when the operation has been performed at its coherence point (device-scope atomics: the
// memory side).  `s_waitcnt vmcnt(0)` is therefore what orders "my atomics have landed" before a following ticket atomic -- without the
// L2 write-back + invalidate that a device-scope release fence adds, and unlike a workgroup-scope fence, which emits no vm wait at all on
// gfx950 (back-off barriers: the ticket could otherwise be performed while another channel still queues this lane's adds).
__device__ __forceinline__ void wait_vm_complete() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// 16-bit feature rows (MVP_FEATURE_BF16 / MVP_FEATURE_F16) widened to float32 in registers.  Both widenings are exact for every value:
// bfloat16 is the upper half of the float32 pattern (an integer shift: no arithmetic touches the value, subnormals keep their bits);
// float16 goes through the hardware conversion, which takes subnormal halves as they are (f16 denormals are never flushed on gfx9) and
// whose results are all normal float32 numbers.  `lo` = the element in bits 0..15 of the word, `hi` = the one in bits 16..31.
template <bool F16>
__device__ __forceinline__ float widen_h16_lo(unsigned w) {
  if constexpr (F16) return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
  else return __uint_as_float(w << 16);
}
template <bool F16>
__device__ __forceinline__ float widen_h16_hi(unsigned w) {
  if constexpr (F16) return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
  else return __uint_as_float(w & 0xffff0000u);
}

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

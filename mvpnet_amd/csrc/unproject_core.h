// unproject_core.h -- the world point of a depth pixel, shared by every kernel that un-projects (unproject_kernel in lifting.hip,
// lift_prepare_kernel in lift_fused.hip, frame_overlap_kernel in overlap.hip) so that they agree bit for bit:
//   X_w = R.(Kinv.[u,v,1]^T * depth) + t  in float64, rounded to float32 ONCE by the caller
// (the reference is float64 "by accident": int64 uv1 promotes, scannet_2d3d.py:35-38, :262, :317).
#pragma once
#include "common.h"

struct UnprojectCam {
  double k[9];   // inverse intrinsics, row-major
  double p[12];  // first three rows of the camera-to-world pose, row-major
};

__device__ __forceinline__ UnprojectCam unproject_cam(const float* __restrict__ Ki, const float* __restrict__ Pm) {
  UnprojectCam c;
#pragma unroll
  for (int i = 0; i < 9; ++i) c.k[i] = (double)Ki[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) c.p[i] = (double)Pm[i];
  return c;
}

// depth of pixel p in metres: float32 as stored, or uint16 millimetres / 1000 (np.asarray(png, float32) / 1000., scannet_2d3d.py:255)
template <typename DepthT>
__device__ __forceinline__ float depth_metres(const DepthT* __restrict__ depth, size_t p) {
  if constexpr (sizeof(DepthT) == 2)
    return __fdiv_rn((float)depth[p], 1000.0f);
  else
    return depth[p];
}

// -> world coordinates (float64, not yet rounded) and the camera-frame depth zc (the pixel is valid when zc > 0, scannet_2d3d.py:260)
__device__ __forceinline__ void unproject_pixel(const UnprojectCam& c, float df, int u, int v, double& xw, double& yw, double& zw,
                                                double& zc) {
  const double d = (double)df, du = (double)u, dv = (double)v;
  const double rx = (c.k[0] * du + c.k[1] * dv) + c.k[2];
  const double ry = (c.k[3] * du + c.k[4] * dv) + c.k[5];
  const double rz = (c.k[6] * du + c.k[7] * dv) + c.k[8];
  const double xc = rx * d, yc = ry * d;
  zc = rz * d;
  xw = ((xc * c.p[0] + yc * c.p[1]) + zc * c.p[2]) + c.p[3];
  yw = ((xc * c.p[4] + yc * c.p[5]) + zc * c.p[6]) + c.p[7];
  zw = ((xc * c.p[8] + yc * c.p[9]) + zc * c.p[10]) + c.p[11];
}

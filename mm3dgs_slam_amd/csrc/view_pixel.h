// What pointcloud.hip and tsdf.hip share about one posed RGB-D view: the pixel validity test, the world->camera pose in double (also
// compact.hip's, for pose prediction), and the colour byte of a float32 channel.  One statement each, so cloud and mesh agree on which pixels are surface.
#pragma once
#include <math.h>
#include "mm3dgs_common.h"

struct Rigid { double R[3][3], t[3]; };      // [R | t; 0 1]

// world->camera 7-vector (qw,qx,qy,qz,tx,ty,tz): normalised quaternion -> R (utils/pose_utils.py:240-271,352-368), no contraction
__device__ __forceinline__ Rigid rigid_from_pose(const float* __restrict__ pose) {
#pragma clang fp contract(off)
  Rigid o;
  double w = pose[0], x = pose[1], y = pose[2], z = pose[3];
  const double n = sqrt(w * w + x * x + y * y + z * z);
  w /= n; x /= n; y /= n; z /= n;
  o.R[0][0] = 1.0 - 2.0 * (y * y + z * z); o.R[0][1] = 2.0 * (x * y - w * z); o.R[0][2] = 2.0 * (x * z + w * y);
  o.R[1][0] = 2.0 * (x * y + w * z); o.R[1][1] = 1.0 - 2.0 * (x * x + z * z); o.R[1][2] = 2.0 * (y * z - w * x);
  o.R[2][0] = 2.0 * (x * z - w * y); o.R[2][1] = 2.0 * (y * z + w * x); o.R[2][2] = 1.0 - 2.0 * (x * x + y * y);
  o.t[0] = pose[4]; o.t[1] = pose[5]; o.t[2] = pose[6];
  return o;
}

// strict float32 tests on the inputs: NaN fails every one of them
__device__ __forceinline__ bool view_pixel_valid(const float* __restrict__ depth, const float* __restrict__ sil, float sil_min, float depth_max, size_t i,
                                                 float& z) {
  z = depth[i];
  bool ok = z > 0.f && z < INFINITY && (depth_max <= 0.f || z <= depth_max);
  if (ok && sil) ok = sil[i] > sil_min;
  return ok;
}

__device__ __forceinline__ uint32_t pc_quant(float c) {
#pragma clang fp contract(off)
  c = c > 0.f ? c : 0.f;      // NaN -> 0
  c = c < 1.f ? c : 1.f;
  return (uint32_t)(uint8_t)(c * 255.0f + 0.5f);
}

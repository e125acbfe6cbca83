// One posed pinhole view (PinholeView: H, W, fx, fy, cx, cy and a world->camera 7-vector), stated once for every export and evaluation kernel
// that takes one -- pointcloud.hip, tsdf.hip / tsdf_sparse.hip (through tsdf_sample.h), cull.hip, meshdepth.hip: the pose in double (also
// compact.hip's, for pose prediction), world -> camera -> pixel, pixel -> world, the finite test of a float32 position (also geometry.hip's),
// the pixel validity test and the colour byte of a float32 channel.  Cloud, mesh, culling and mesh depth agree bit for bit on which pixel a
// point falls in because they call the same function.  Every function is compiled without contraction: the pragma holds per function body,
// and the host statements round alike.
#pragma once
#include <math.h>
#include "fused_api.h"

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

// the pose is the same for every lane: one lane normalises the quaternion into the workgroup's g (LDS); every lane of the workgroup calls
__device__ __forceinline__ void view_rigid_shared(const float* __restrict__ pose, Rigid& g) {
#pragma clang fp contract(off)
  if (threadIdx.x == 0) g = rigid_from_pose(pose);
  __syncthreads();
}

// a float32 position without NaN or infinity
__device__ __forceinline__ bool view_finite(float x, float y, float z) {
#pragma clang fp contract(off)
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// world -> camera: p_c = R p_w + t, each row summed left to right.  The callers test z and leave before they use x and y: the three rows are
// independent and without side effects, so the compiler moves the rows of x and y behind that branch (cull_mark_kernel, tsdf_sample_update:
// z, its test, then x, then y in the listing; profiles/r22_offloop_view.txt, section 3).  A listing that computes all three rows in front of
// the test of z has lost that early-out: look there first when one of these kernels gets slower
__device__ __forceinline__ void view_to_camera(const Rigid& g, double pw0, double pw1, double pw2, double& x, double& y, double& z) {
#pragma clang fp contract(off)
  x = g.R[0][0] * pw0 + g.R[0][1] * pw1 + g.R[0][2] * pw2 + g.t[0];
  y = g.R[1][0] * pw0 + g.R[1][1] * pw1 + g.R[1][2] * pw2 + g.t[1];
  z = g.R[2][0] * pw0 + g.R[2][1] * pw1 + g.R[2][2] * pw2 + g.t[2];
}

// camera -> pixel: the nearest pixel (floor(fx x / z + cx + 0.5), floor(fy y / z + cy + 0.5)) and its linear index; false outside the image
// (a NaN fails).  The caller has tested z: what depth counts as in front differs between the callers
__device__ __forceinline__ bool view_pixel_index(const PinholeView& v, double x, double y, double z, size_t& pix) {
#pragma clang fp contract(off)
  const double fu = floor(v.fx * x / z + v.cx + 0.5), fv = floor(v.fy * y / z + v.cy + 0.5);
  if (!(fu >= 0.0 && fu < (double)v.W && fv >= 0.0 && fv < (double)v.H)) return false;
  pix = (size_t)(int)fv * (size_t)v.W + (size_t)(int)fu;
  return true;
}

// pixel -> world at depth z: p_c = ((u - cx) / fx z, (v - cy) / fy z, z), P = R^T (p_c - t), in double and unrounded; no half-pixel offset
__device__ __forceinline__ void view_lift(const PinholeView& v, const Rigid& g, double u, double w, double z, double (&P)[3]) {
#pragma clang fp contract(off)
  const double c0 = (u - v.cx) / v.fx * z - g.t[0];
  const double c1 = (w - v.cy) / v.fy * z - g.t[1];
  const double c2 = z - g.t[2];
  for (int a = 0; a < 3; a++) P[a] = g.R[0][a] * c0 + g.R[1][a] * c1 + g.R[2][a] * c2;
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

// Frame ingest (mm3dgs_ingest_frame; host path: mm3dgs_slam_amd/dataset.py ingest_host): the raw sensor bytes of one frame -- uint8
// interleaved RGB [Hs,Ws,3] and uint16 depth [Hs,Ws], 5 bytes per source pixel -- become the two float32 images the SLAM loops consume,
// colour [3,H,W] in [0,1] and depth [H,W] in metres, in ONE launch.  It replaces the reference's per-frame host chain
// (gradslam_datasets/basedataset.py:238-285,324-377, slam/SLAM.py:384-390): cv2.resize of a float64 copy (INTER_LINEAR for colour,
// INTER_NEAREST for depth), the division by png_depth_scale, the cast to float32, the upload of 16 bytes per pixel, permute and / 255.
//
// Semantics (normative; include/mm3dgs.h states them in full).  With sx = (double)Ws / W, sy = (double)Hs / H:
//   colour  fx = (x + 0.5) sx - 0.5, x0 = floor(fx), a = fx - x0; x0 < 0 -> (0, 0); x0 >= Ws - 1 -> (Ws - 1, 0); x1 = min(x0 + 1, Ws - 1);
//           the same for y; v = (1 - b) ((1 - a) p00 + a p01) + b ((1 - a) p10 + a p11), here in double, rounded once to float32;
//           out = v / 255.0f, the correctly rounded float32 division.
//   depth   xs = min((int)floor(x sx), Ws - 1), ys likewise; out = (float)((double)d / png_depth_scale): the double quotient rounded once.
// This is meant to be what cv2.resize computes on float64 input.  cv2 was NOT available where this was written, so the match to cv2
// itself is unchecked: the kernel is held to the host path (bit-exact depth; bit-exact colour at integer ratios, where a and b are 0 or
// 0.5 and v is exact; 1e-6 elsewhere), and the host path to an independent float64 bilinear reference.
//
// Kernels.  The launch is ~6 MB of traffic at 640 x 480: bound by launch latency, not by anything inside it -- no LDS, no atomics, and
// nothing clever.  Lanes of a wave cover contiguous output pixels of one row, every store is at least a dword per lane.
//   ingest_native_kernel   Hs == H, Ws == W, W % 4 == 0 and aligned pointers: one lane per four pixels, three packed source dwords
//                          (12 bytes of RGB) and one 8-byte depth load in, four float4 out.
//   ingest_scalar_kernel   everything else (any ratio, any width, any byte alignment of rgb): one lane per output pixel, byte loads
//                          at clamped indices -- no lane reads outside [Hs,Ws] whatever the ratio.  Always correct; the native kernel
//                          gives the same bits where both apply (a = b = 0: v is the byte itself).
//
// Monocular depth estimate (mm3dgs_ingest_est; host path: dataset.py ingest_est_host): the depth network's raw output [Hs,Ws] as float32,
// float16 or uint16 becomes the float32 [H,W] estimate, the reference's last step (utils/depth_utils.py MiDaS.estimate_depth: F.interpolate,
// bilinear, align_corners=False) in ONE launch.  The colour rule above on one channel, then v * scale, the double product rounded once:
//   Hs == H and Ws == W   out = (float)((double)p * scale): the value itself, no blend, so a non-finite neighbour does not spread;
//   otherwise             out = (float)(((1 - b) ((1 - a) p00 + a p01) + b ((1 - a) p10 + a p11)) * scale), all in double.
//   ingest_est_packed_kernel   equal sizes, W % 4 == 0, source 16-byte (float32) / 8-byte (16-bit types) and output 16-byte aligned: one lane
//                              per four pixels, one vector load and one float4 store.
//   ingest_est_kernel          everything else: one lane per output pixel, four taps at clamped indices.  The same bits as the packed
//                              kernel where both apply.
// ~1.6 MB of traffic at 384 x 512 float16 -> 480 x 640: launch-latency bound like the frame kernels.  Not timed yet.
#include <math.h>
#include <hip/hip_fp16.h>
#include "mm3dgs_common.h"
#include "fused_api.h"

// the blend restates the host path's float64 operators one by one: no contraction to FMA (exact cases do not care, the rest stay closer)
#pragma clang fp contract(off)

#define INGEST_WG 256

// source coordinate of the bilinear rule along one axis: (i0, i1, weight of i1)
__device__ __forceinline__ void ingest_axis(int i, double scale, int n_src, int& i0, int& i1, double& w) {
  const double f = ((double)i + 0.5) * scale - 0.5;
  double fl = floor(f);
  w = f - fl;
  if (fl < 0.0) { fl = 0.0; w = 0.0; }
  if (fl >= (double)(n_src - 1)) { fl = (double)(n_src - 1); w = 0.0; }
  i0 = (int)fl;
  i1 = min(i0 + 1, n_src - 1);
}

__device__ __forceinline__ int ingest_nearest(int i, double scale, int n_src) {
  const double f = floor((double)i * scale);
  return f >= (double)(n_src - 1) ? n_src - 1 : (int)f;      // (i >= 0 and scale > 0: f >= 0)
}

__global__ void __launch_bounds__(INGEST_WG)
ingest_scalar_kernel(int Hs, int Ws, const uint8_t* __restrict__ rgb, const uint16_t* __restrict__ depth, double depth_scale, int H, int W,
                     int blocks_per_row, float* __restrict__ out_color, float* __restrict__ out_depth) {
  const int y = (int)(blockIdx.x / (unsigned)blocks_per_row);
  const int x = (int)(blockIdx.x % (unsigned)blocks_per_row) * INGEST_WG + (int)threadIdx.x;
  if (x >= W || y >= H) return;
  const double sx = (double)Ws / (double)W, sy = (double)Hs / (double)H;
  const size_t HW = (size_t)H * (size_t)W, o = (size_t)y * (size_t)W + (size_t)x;
  int x0, x1, y0, y1;
  double a, b;
  ingest_axis(x, sx, Ws, x0, x1, a);
  ingest_axis(y, sy, Hs, y0, y1, b);
  const size_t r0 = (size_t)y0 * (size_t)Ws, r1 = (size_t)y1 * (size_t)Ws;
  const uint8_t* p00 = rgb + (r0 + (size_t)x0) * 3;
  const uint8_t* p01 = rgb + (r0 + (size_t)x1) * 3;
  const uint8_t* p10 = rgb + (r1 + (size_t)x0) * 3;
  const uint8_t* p11 = rgb + (r1 + (size_t)x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double top = (1.0 - a) * (double)p00[c] + a * (double)p01[c];
    const double bot = (1.0 - a) * (double)p10[c] + a * (double)p11[c];
    const float v = (float)((1.0 - b) * top + b * bot);
    out_color[(size_t)c * HW + o] = v / 255.0f;
  }
  if (depth) {
    const int xs = ingest_nearest(x, sx, Ws), ys = ingest_nearest(y, sy, Hs);
    const double d = (double)depth[(size_t)ys * (size_t)Ws + (size_t)xs];
    out_depth[o] = (float)(d / depth_scale);
  }
}

// n_quads = H W / 4 groups of four pixels; a group never straddles a row (W % 4 == 0).  rgb is 4-byte, depth 8-byte, the outputs 16-byte aligned.
__global__ void __launch_bounds__(INGEST_WG)
ingest_native_kernel(size_t n_quads, const uint32_t* __restrict__ rgb, const uint2* __restrict__ depth, double depth_scale,
                     float4* __restrict__ out_color, float4* __restrict__ out_depth) {
  const size_t q = (size_t)blockIdx.x * INGEST_WG + threadIdx.x;
  if (q >= n_quads) return;
  const uint32_t w0 = rgb[q * 3], w1 = rgb[q * 3 + 1], w2 = rgb[q * 3 + 2];      // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian)
  const float4 r = make_float4((float)(w0 & 255u), (float)(w0 >> 24), (float)((w1 >> 16) & 255u), (float)((w2 >> 8) & 255u));
  const float4 g = make_float4((float)((w0 >> 8) & 255u), (float)(w1 & 255u), (float)(w1 >> 24), (float)((w2 >> 16) & 255u));
  const float4 bl = make_float4((float)((w0 >> 16) & 255u), (float)((w1 >> 8) & 255u), (float)(w2 & 255u), (float)(w2 >> 24));
  out_color[q] = make_float4(r.x / 255.0f, r.y / 255.0f, r.z / 255.0f, r.w / 255.0f);
  out_color[n_quads + q] = make_float4(g.x / 255.0f, g.y / 255.0f, g.z / 255.0f, g.w / 255.0f);
  out_color[2 * n_quads + q] = make_float4(bl.x / 255.0f, bl.y / 255.0f, bl.z / 255.0f, bl.w / 255.0f);
  if (depth) {
    const uint2 d = depth[q];
    out_depth[q] = make_float4((float)((double)(d.x & 0xffffu) / depth_scale), (float)((double)(d.x >> 16) / depth_scale),
                               (float)((double)(d.y & 0xffffu) / depth_scale), (float)((double)(d.y >> 16) / depth_scale));
  }
}

void launch_ingest_frame(int Hs, int Ws, const uint8_t* rgb, const uint16_t* depth, double depth_scale, int H, int W, float* out_color,
                         float* out_depth, hipStream_t s) {
  const bool native = Hs == H && Ws == W && (W & 3) == 0 && ((uintptr_t)rgb & 3) == 0 && ((uintptr_t)depth & 7) == 0 &&
                      ((uintptr_t)out_color & 15) == 0 && ((uintptr_t)out_depth & 15) == 0;
  if (native) {
    const size_t n_quads = (size_t)H * (size_t)W / 4;
    const size_t blocks = (n_quads + INGEST_WG - 1) / INGEST_WG;
    hipLaunchKernelGGL(ingest_native_kernel, dim3((unsigned)blocks), dim3(INGEST_WG), 0, s, n_quads, (const uint32_t*)rgb, (const uint2*)depth,
                       depth_scale, (float4*)out_color, (float4*)out_depth);
    return;
  }
  const int blocks_per_row = (W + INGEST_WG - 1) / INGEST_WG;
  const size_t blocks = (size_t)blocks_per_row * (size_t)H;
  hipLaunchKernelGGL(ingest_scalar_kernel, dim3((unsigned)blocks), dim3(INGEST_WG), 0, s, Hs, Ws, rgb, depth, depth_scale, H, W, blocks_per_row,
                     out_color, out_depth);
}

// ---- monocular depth estimate ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double est_value(float v) { return (double)v; }
__device__ __forceinline__ double est_value(__half v) { return (double)__half2float(v); }      // (exact: every float16 is a float32)
__device__ __forceinline__ double est_value(uint16_t v) { return (double)v; }

template <typename T>
__global__ void __launch_bounds__(INGEST_WG)
ingest_est_kernel(int Hs, int Ws, const T* __restrict__ est, double scale, int H, int W, int blocks_per_row, float* __restrict__ out) {
  const int y = (int)(blockIdx.x / (unsigned)blocks_per_row);
  const int x = (int)(blockIdx.x % (unsigned)blocks_per_row) * INGEST_WG + (int)threadIdx.x;
  if (x >= W || y >= H) return;
  const size_t o = (size_t)y * (size_t)W + (size_t)x;
  if (Hs == H && Ws == W) {
    out[o] = (float)(est_value(est[o]) * scale);
    return;
  }
  const double sx = (double)Ws / (double)W, sy = (double)Hs / (double)H;
  int x0, x1, y0, y1;
  double a, b;
  ingest_axis(x, sx, Ws, x0, x1, a);
  ingest_axis(y, sy, Hs, y0, y1, b);
  const size_t r0 = (size_t)y0 * (size_t)Ws, r1 = (size_t)y1 * (size_t)Ws;
  const double p00 = est_value(est[r0 + (size_t)x0]), p01 = est_value(est[r0 + (size_t)x1]);
  const double p10 = est_value(est[r1 + (size_t)x0]), p11 = est_value(est[r1 + (size_t)x1]);
  const double top = (1.0 - a) * p00 + a * p01;
  const double bot = (1.0 - a) * p10 + a * p11;
  const double v = (1.0 - b) * top + b * bot;
  out[o] = (float)(v * scale);
}

// four consecutive source values of one lane: a 16-byte load of float32, an 8-byte load of the 16-bit types
__device__ __forceinline__ void est_load4(const float* p, size_t q, double v[4]) {
  const float4 f = reinterpret_cast<const float4*>(p)[q];
  v[0] = (double)f.x; v[1] = (double)f.y; v[2] = (double)f.z; v[3] = (double)f.w;
}
__device__ __forceinline__ void est_load4(const uint16_t* p, size_t q, double v[4]) {
  const uint2 d = reinterpret_cast<const uint2*>(p)[q];      // little endian: the first value in the low half
  v[0] = (double)(d.x & 0xffffu); v[1] = (double)(d.x >> 16); v[2] = (double)(d.y & 0xffffu); v[3] = (double)(d.y >> 16);
}
__device__ __forceinline__ void est_load4(const __half* p, size_t q, double v[4]) {
  const uint2 d = reinterpret_cast<const uint2*>(p)[q];
  v[0] = est_value(__ushort_as_half((unsigned short)(d.x & 0xffffu))); v[1] = est_value(__ushort_as_half((unsigned short)(d.x >> 16)));
  v[2] = est_value(__ushort_as_half((unsigned short)(d.y & 0xffffu))); v[3] = est_value(__ushort_as_half((unsigned short)(d.y >> 16)));
}

// n_quads = H W / 4 groups of four pixels at equal sizes (W % 4 == 0)
template <typename T>
__global__ void __launch_bounds__(INGEST_WG)
ingest_est_packed_kernel(size_t n_quads, const T* __restrict__ est, double scale, float4* __restrict__ out) {
  const size_t q = (size_t)blockIdx.x * INGEST_WG + threadIdx.x;
  if (q >= n_quads) return;
  double v[4];
  est_load4(est, q, v);
  out[q] = make_float4((float)(v[0] * scale), (float)(v[1] * scale), (float)(v[2] * scale), (float)(v[3] * scale));
}

template <typename T>
static void launch_ingest_est_t(int Hs, int Ws, const T* est, double scale, int H, int W, float* out, hipStream_t s) {
  const uintptr_t src_mask = sizeof(T) == 4 ? 15 : 7;
  if (Hs == H && Ws == W && (W & 3) == 0 && ((uintptr_t)est & src_mask) == 0 && ((uintptr_t)out & 15) == 0) {
    const size_t n_quads = (size_t)H * (size_t)W / 4;
    const size_t blocks = (n_quads + INGEST_WG - 1) / INGEST_WG;
    hipLaunchKernelGGL(ingest_est_packed_kernel<T>, dim3((unsigned)blocks), dim3(INGEST_WG), 0, s, n_quads, est, scale, (float4*)out);
    return;
  }
  const int blocks_per_row = (W + INGEST_WG - 1) / INGEST_WG;
  const size_t blocks = (size_t)blocks_per_row * (size_t)H;
  hipLaunchKernelGGL(ingest_est_kernel<T>, dim3((unsigned)blocks), dim3(INGEST_WG), 0, s, Hs, Ws, est, scale, H, W, blocks_per_row, out);
}

void launch_ingest_est(int Hs, int Ws, const void* est, int dtype, double scale, int H, int W, float* out, hipStream_t s) {
  if (dtype == 0) launch_ingest_est_t(Hs, Ws, (const float*)est, scale, H, W, out, s);
  else if (dtype == 1) launch_ingest_est_t(Hs, Ws, (const __half*)est, scale, H, W, out, s);
  else launch_ingest_est_t(Hs, Ws, (const uint16_t*)est, scale, H, W, out, s);
}

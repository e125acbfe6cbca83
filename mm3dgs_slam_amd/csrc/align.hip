// Least-squares alignment of a monocular depth estimate to a depth image (mm3dgs_align_depth; reference slam/SLAM.py:411-448 with
// utils/depth_utils.py:44-99; host path: depth_utils.get_scale_shift_LS): fit  scale * est + shift ~ 1 / depth  over the valid pixels
// and write  out = 1 / (scale * est + shift)  for every pixel -- three image reads, five sums, one image write, in two launches instead
// of the ~30 torch launches and the float64 copies of the whole image that the host path takes.
//
// Pixel rule (the host path's, except for the corner named last):
//   considered  with a silhouette:  sil > sil_min && est > est_min   (strict, float32; the callers pass 0.99f and 1e-6f)
//               without one:        depth > 0                        (the UT-MM first frame, fitted to the sensor depth)
//   valid       considered && 0 < z < +inf,  z = the correctly rounded float32 quotient 1.0f / depth, widened to double -- the value the
//               host path sums.  NaN, zero, negative and +inf depth are therefore invalid, and a NaN / inf of est at a pixel that is
//               not considered never reaches the sums (selects, not products with a 0/1 mask).
//   DIFFERENCE from the host path: a considered pixel whose depth is so small (zero, subnormal) that 1 / depth overflows to +inf is
//   excluded here; the host path sums it and returns NaN, as the reference does.
//
// Kernels (the pattern of loss.hip: no atomics, no hand-off between the workgroups of a launch, bit-reproducible from call to call):
//   align_sums_kernel          fixed grid of at most ALIGN_MAX_ROWS workgroups, grid-stride loop, five double accumulators per lane
//                              (h = (double)est: a00 = sum h^2, a01 = sum h, n = sum 1, b0 = sum h z, b1 = sum z), DPP sum inside a wave,
//                              LDS across the four waves, one row of ALIGN_ROW doubles per workgroup with plain stores.
//   align_finish_apply_kernel  every workgroup adds the at most ALIGN_MAX_ROWS rows in the same fixed order (one row per lane, the same
//                              wave / LDS reduction), solves the 2 x 2 system as get_scale_shift_LS states it and applies the float32
//                              (scale, shift) to its pixels; workgroup 0 also writes the fit record.  A finishing launch of its own
//                              would save each workgroup 10 KB of L2 reads and cost a third launch in a chain that is all launch latency.
// Nothing here assumes more than the 4-byte alignment of a float: depth and silhouette are planes of a [6,H,W] image, which start on a
// 4-byte boundary only when H W is odd -- every image access is one dword per lane (256 contiguous bytes per wave instruction).
#include <math.h>
#include "mm3dgs_common.h"
#include "fused_api.h"
#include "block_ops.h"

// The solve restates the host path literally (det = a00 n - a01^2 from two rounded products) and the apply is float32 with an unfused
// multiply and add.  hipcc contracts a * b + c to an FMA by default, and the header's __fmul_rn / __fadd_rn do not stop it: they are the
// plain operators, compiled under the header's own contraction setting, and came out as one v_fma_f32 here.  So this file turns
// contraction off and writes the operators itself; `/` is the correctly rounded division (what __fdiv_rn expands to as well).
#pragma clang fp contract(off)

#define ALIGN_WG 256        // lanes per workgroup (four waves)
#define ALIGN_MAX_ROWS 256  // workgroups of the sums launch = rows of partial sums; <= ALIGN_WG: the finish reads one row per lane
#define ALIGN_ROW 8         // doubles per row: a00, a01, n, b0, b1, three unused (a 64-byte row)

static int align_rows(size_t HW) {
  const size_t r = (HW + ALIGN_WG - 1) / ALIGN_WG;
  return (int)(r < ALIGN_MAX_ROWS ? r : ALIGN_MAX_ROWS);
}
size_t align_depth_work_bytes(int H, int W) { return align_up((size_t)align_rows((size_t)H * (size_t)W) * ALIGN_ROW * sizeof(double), 256); }

__global__ void __launch_bounds__(ALIGN_WG)
align_sums_kernel(size_t HW, const float* __restrict__ est, const float* __restrict__ depth, const float* __restrict__ sil, float sil_min,
                  float est_min, double* __restrict__ rows) {
  __shared__ double sh[4][5];
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const size_t stride = (size_t)gridDim.x * ALIGN_WG;
  for (size_t i = (size_t)blockIdx.x * ALIGN_WG + threadIdx.x; i < HW; i += stride) {
    const float e = est[i], d = depth[i];
    const bool considered = sil ? (sil[i] > sil_min && e > est_min) : (d > 0.f);
    const float zf = 1.0f / d;
    const bool valid = considered && zf > 0.f && zf < INFINITY;
    const double h = (double)e, z = (double)zf;     // (products of two float32 values are exact in double)
    acc[0] += valid ? h * h : 0.0;
    acc[1] += valid ? h : 0.0;
    acc[2] += valid ? 1.0 : 0.0;
    acc[3] += valid ? h * z : 0.0;
    acc[4] += valid ? z : 0.0;
  }
  block_sums_f64<5, true>(acc, sh);      // fixed order; the totals in every lane
  if (threadIdx.x < ALIGN_ROW) {
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < 5; k++) r = (int)threadIdx.x == k ? acc[k] : r;
    rows[(size_t)blockIdx.x * ALIGN_ROW + threadIdx.x] = r;
  }
}

__global__ void __launch_bounds__(ALIGN_WG)
align_finish_apply_kernel(size_t HW, const float* __restrict__ est, const double* __restrict__ rows, int nrows, double* __restrict__ fit,
                          float* __restrict__ out) {
  __shared__ double sh[4][5];
  double tot[5];
  const bool has = (int)threadIdx.x < nrows;
#pragma unroll
  for (int k = 0; k < 5; k++) tot[k] = has ? rows[(size_t)threadIdx.x * ALIGN_ROW + k] : 0.0;
  block_sums_f64<5, true>(tot, sh);
  // get_scale_shift_LS, literally: a singular system (fewer than two valid pixels, or an estimate that is constant over them to its own
  // float32 rounding) has no fit and returns the identity
  const double a00 = tot[0], a01 = tot[1], n = tot[2], b0 = tot[3], b1 = tot[4];
  const double a00n = a00 * n;
  const double det = a00n - a01 * a01;
  const bool ok = n >= 2.0 && fabs(det) > 1e-9 * fmax(fabs(a00n), 1e-300) && isfinite(det);
  const double safe = ok ? det : 1.0;
  const float scale = ok ? (float)((n * b0 - a01 * b1) / safe) : 1.f;
  const float shift = ok ? (float)((a00 * b1 - a01 * b0) / safe) : 0.f;
  if (blockIdx.x == 0 && threadIdx.x < 16) {
    double r = 0.0;
    const double rec[8] = {(double)scale, (double)shift, ok ? 1.0 : 0.0, n, a00, a01, b0, b1};
#pragma unroll
    for (int k = 0; k < 8; k++) r = (int)threadIdx.x == k ? rec[k] : r;
    fit[threadIdx.x] = r;
  }
  if (!out) return;
  const size_t stride = (size_t)gridDim.x * ALIGN_WG;
  for (size_t i = (size_t)blockIdx.x * ALIGN_WG + threadIdx.x; i < HW; i += stride)
    out[i] = 1.0f / (scale * est[i] + shift);    // v_mul_f32, v_add_f32, the v_div_scale / v_div_fmas / v_div_fixup sequence
}

void launch_align_depth(int H, int W, const float* est, const float* depth, const float* sil, float sil_min, float est_min, double* rows,
                        double* fit, float* out, hipStream_t s) {
  const size_t HW = (size_t)H * (size_t)W;
  const int nrows = align_rows(HW);
  hipLaunchKernelGGL(align_sums_kernel, dim3(nrows), dim3(ALIGN_WG), 0, s, HW, est, depth, sil, sil_min, est_min, rows);
  hipLaunchKernelGGL(align_finish_apply_kernel, dim3(out ? nrows : 1), dim3(ALIGN_WG), 0, s, HW, est, (const double*)rows, nrows, fit, out);
}

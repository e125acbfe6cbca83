// Image evaluation of a finished run (mm3dgs_eval_image; reference slam/SLAM.py:197-231 with utils/image_utils.py:17-19 and
// utils/loss_utils.py:95-154; host path: eval_utils.image_metrics_host): PSNR, SSIM and the depth L1 / RMSE of one rendered frame against
// the recorded one, as one row of sixteen doubles on the device -- two launches instead of the five grouped 11x11 convolutions, the
// operators around them and the two host read-backs per frame of the torch chain.
//
// Kernels (the pattern of loss.hip: no atomics, no hand-off between the workgroups of a launch, bit-reproducible from call to call):
//   eval_tile_kernel    one 16x16-pixel tile per 256-lane workgroup.  The SSIM map is the one ssim_maps_kernel computes: the same staged
//                       26x26 halo regions and the same separable moment strips (loss_tile.h: ssim_moments_hpass / ssim_moments_vpass /
//                       ssim_px), float32 moments and map, the map's quotient as one IEEE division.  Every per-pixel term is widened to
//                       double before it is summed: the squared colour difference (subtracted in double), the map value, and over
//                       { 0 < gt_depth < +inf } the count, |depth - gt_depth| and its square.  One row of EVAL_ROW doubles per tile, plain stores, every column written.
//   eval_finish_kernel  one workgroup: the fixed-order double sum of the tile rows (reduce_rows_256, loss_tile.h), then the sixteen values.
// Nothing here assumes more than the 4-byte alignment of a float: the colour planes go through dword buffer loads, the depth images through
// one dword load per lane.
#include <math.h>
#include "loss_tile.h"
#include "block_ops.h"

#define EVAL_ROW 12     // doubles per tile row (the row width reduce_rows_256 reads): sse[3], ssim_sum[3], n, sum |d|, sum d^2, three zeros

struct EvalCfg { int H, W; float window[11]; };

static int eval_tiles_x(int W) { return (W + LT - 1) / LT; }
static int eval_tiles(int H, int W) { return eval_tiles_x(W) * ((H + LT - 1) / LT); }
size_t eval_image_work_bytes(int H, int W) { return align_up((size_t)eval_tiles(H, W) * EVAL_ROW * sizeof(double), 256); }

__global__ void __launch_bounds__(256)
eval_tile_kernel(EvalCfg cfg, const float* __restrict__ image, const float* __restrict__ gt, const float* __restrict__ depth,
                 const float* __restrict__ gt_depth, double* __restrict__ partial, int tiles_x) {
  __shared__ __align__(16) float sI[LW][SW], sG[LW][SW];
  __shared__ __align__(16) float hS[5][LW][HW_];
  __shared__ double red[4][9];
  const int tile = blockIdx.x;
  const int x0 = (tile % tiles_x) * LT, y0 = (tile / tiles_x) * LT;
  const uint32_t HW = (uint32_t)cfg.H * (uint32_t)cfg.W;   // H W <= 2^28 (checked by the API): the byte offset of every colour element fits 32 bits
  const int tid = threadIdx.x;
  const HaloIdx hx = halo_index(cfg.H, cfg.W, x0, y0);
  const Rsrc r_im = make_rsrc(image, HW * 12u), r_gt = make_rsrc(gt, HW * 12u);
  float va[3], vb[3];
#pragma unroll
  for (int e = 0; e < 3; e++) {
    va[e] = hx.off[e] >= 0 ? bld(r_im, (uint32_t)hx.off[e]) : 0.f;
    vb[e] = hx.off[e] >= 0 ? bld(r_gt, (uint32_t)hx.off[e]) : 0.f;
  }
  const int tx = tid & 15, ty = tid >> 4;      // this lane's pixel
  const int px = x0 + tx, py = y0 + ty;
  const bool inside = px < cfg.W && py < cfg.H;
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; k++) acc[k] = 0.0;
  if (inside && depth) {
    const size_t pix = (size_t)py * (size_t)cfg.W + (size_t)px;
    const float g = gt_depth[pix];
    if (g > 0.f && g < INFINITY) {      // strict float32 test: NaN, +-0, negative and +inf are invalid
      const double d = fabs((double)depth[pix] - (double)g);      // (a NaN of the rendered depth propagates)
      acc[6] = 1.0; acc[7] = d; acc[8] = d * d;
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
#pragma unroll
    for (int e = 0; e < 3; e++)
      if (hx.lds[e] >= 0) { (&sI[0][0])[hx.lds[e]] = va[e]; (&sG[0][0])[hx.lds[e]] = vb[e]; }
    __syncthreads();   // staging complete; also: every lane has finished the previous channel's vertical pass (hS is free)
    if (ch < 2) {
#pragma unroll
      for (int e = 0; e < 3; e++) {
        va[e] = hx.off[e] >= 0 ? bld(r_im, (uint32_t)(ch + 1) * HW + (uint32_t)hx.off[e]) : 0.f;
        vb[e] = hx.off[e] >= 0 ? bld(r_gt, (uint32_t)(ch + 1) * HW + (uint32_t)hx.off[e]) : 0.f;
      }
    }
    if (inside) {
      const double d = (double)sI[ty + HALO][tx + HALO] - (double)sG[ty + HALO][tx + HALO];
      acc[ch] = d * d;
    }
    ssim_moments_hpass(cfg.window, sI, sG, hS, tid);
    __syncthreads();
    float st[5];
    ssim_moments_vpass(cfg.window, hS, tx, ty, st);
    if (inside) {
      const SsimPx p = ssim_px(st);
      acc[3 + ch] = (double)((p.A1 * p.A2) / (p.B1 * p.B2));      // the correctly rounded float32 division, as the host chain's map
    }
  }
  block_sums_f64<9, false>(acc, red);      // fixed order; valid in lane 0
  if (tid == 0) {
    double* row = partial + (size_t)tile * EVAL_ROW;
#pragma unroll
    for (int k = 0; k < 9; k++) row[k] = acc[k];
    row[9] = 0.0; row[10] = 0.0; row[11] = 0.0;
  }
}

__global__ void __launch_bounds__(256)
eval_finish_kernel(int H, int W, const double* __restrict__ partial, int nrows, int has_depth, double* __restrict__ row) {
  __shared__ double part[16][16];
  __shared__ double tot[16];
  reduce_rows_256(partial, nrows, 0xfffu, part, tot);
  if (threadIdx.x < 16) {
    const double hw = (double)H * (double)W;
    double mse[3], psnr = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      mse[c] = tot[c] / hw;
      psnr += 20.0 * log10(1.0 / sqrt(mse[c]));      // mse == 0: +inf, as torch gives
    }
    const double n = has_depth ? tot[6] : 0.0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double v[16] = {psnr / 3.0, ((tot[3] + tot[4]) + tot[5]) / (3.0 * hw), n > 0.0 ? tot[7] / n : nan, n,
                          mse[0], mse[1], mse[2], tot[3] / hw, tot[4] / hw, tot[5] / hw, n > 0.0 ? sqrt(tot[8] / n) : nan,
                          0.0, 0.0, 0.0, 0.0, 0.0};
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < 16; k++) r = (int)threadIdx.x == k ? v[k] : r;
    row[threadIdx.x] = r;
  }
}

void launch_eval_image(int H, int W, const float* image, const float* gt, const float* depth, const float* gt_depth, const float* window,
                       double* rows, double* row, hipStream_t s) {
  EvalCfg cfg;
  cfg.H = H; cfg.W = W;
  for (int i = 0; i < 11; i++) cfg.window[i] = window[i];
  const int T = eval_tiles(H, W);
  hipLaunchKernelGGL(eval_tile_kernel, dim3(T), dim3(256), 0, s, cfg, image, gt, depth, gt_depth, rows, eval_tiles_x(W));
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(256), 0, s, H, W, (const double*)rows, T, depth ? 1 : 0, row);
}

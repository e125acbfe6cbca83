// Debug mosaic (mm3dgs_mosaic; host path: mm3dgs_slam_amd/debug_frames.py compose_host): rows x cols panels of H x W pixels -- float32 colour
// images, the absolute difference of two of them, depth images through a 256-entry colour table -- become ONE interleaved uint8 image
// [rows H, cols W, 3], the frame of the reference's debug video (slam/SLAM.py:233-276) and of SLAM.render() (:148-195).  The reference
// composes it on the host: a matplotlib colour-map call on a float64 copy of every depth image (device -> host -> device each), a chain of
// torch.cat and the cast of the float64 result.  Here only the finished bytes leave the device.
//
// Semantics (normative; include/mm3dgs.h states them in full):
//   kind 0  v = a[ch,y,x];  kind 1  v = fabsf(a[ch,y,x] - b[ch,y,x]), one float32 subtraction;  byte = Q(v):
//           p = (double)v * 255 (exact);  quant 0: NaN or p < 0 -> 0, p >= 255 -> 255, else trunc(p);
//                                         quant 1: NaN -> 0, else trunc(min(max(p + 0.5, 0), 255)), the sum rounded once in double.
//   kind 2  lo, hi = min, max over the panel (any NaN: both NaN);  t = (a[y,x] - lo) / (hi - lo) in float32, IEEE division, clamped to
//           [0,1] with a NaN kept;  byte = lut[min((int)(t * 256), 255)][ch];  a NaN t is (0,0,0) -- so a panel with a NaN, or with
//           hi == lo (0 / 0), is black throughout: nothing here special-cases it, the operators do it.
//
// Kernels.  A streaming job, 22 MB in (60 + 12 bytes per pixel) and 5.5 MB out for the 2 x 3 mosaic at 640 x 480: no atomics, no hand-off between the workgroups of a
// launch, the same bytes on every call (min and max are exact in any order).
//   mosaic_range_kernel     grid (parts, panels): workgroup (j, p) of a kind-2 panel folds its grid-stride share of the H W values into one
//                           (lo, hi, NaN flag) record of `work`; fminf / fmaxf drop a NaN, hence the flag.  One dword per lane per load:
//                           a depth image is a plane of a [6,H,W] render and has no more than a float's alignment.
//   mosaic_compose_kernel   one workgroup per 1 KB of one output row, one lane per ALIGNED output dword (the row stride 3 cols W and the
//                           row's first byte have no alignment: the dword grid is laid over the row from the dword that holds its first
//                           byte; a lane whose dword hangs over either end of the row stores its bytes one by one, since the rest of that
//                           dword belongs to the neighbouring row and another workgroup).  The four bytes of a lane are 4/3 of a pixel: per
//                           plane the lanes of a wave read one contiguous run of floats, every float of a colour plane exactly once.  The
//                           first wave folds the at most `parts` records of the kind-2 panels its workgroup touches (one or two) first.
#include <math.h>
#include "mm3dgs_common.h"
#include "fused_api.h"

// every operator below restates the host path's: no contraction, `/` is the correctly rounded division
#pragma clang fp contract(off)

#define MOSAIC_WG 256
#define MOSAIC_PARTS 64       // records per panel = workgroups per panel of the range launch; <= 64: the compose kernel folds one per lane of a wave

struct MosaicPart { float lo, hi; uint32_t nan, unused; };      // 16 bytes

static int mosaic_parts(size_t HW) {
  const size_t r = (HW + MOSAIC_WG - 1) / MOSAIC_WG;
  return (int)(r < MOSAIC_PARTS ? r : MOSAIC_PARTS);
}
size_t mosaic_work_bytes(int rows, int cols) { return (size_t)rows * (size_t)cols * MOSAIC_PARTS * sizeof(MosaicPart); }

// (lo, hi, flag) over the 64 lanes of a wave, to every lane
__device__ __forceinline__ void mosaic_wave_range(float& lo, float& hi, uint32_t& bad) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, m));
    hi = fmaxf(hi, __shfl_xor(hi, m));
    bad |= (uint32_t)__shfl_xor((int)bad, m);
  }
}

__global__ void __launch_bounds__(MOSAIC_WG)
mosaic_range_kernel(MosaicPanels P, size_t HW, MosaicPart* __restrict__ work) {
  __shared__ float sh_lo[4], sh_hi[4];
  __shared__ uint32_t sh_bad[4];
  const int p = (int)blockIdx.y;
  if (P.kind[p] != 2) return;
  const float* __restrict__ a = P.a[p];
  float lo = INFINITY, hi = -INFINITY;
  uint32_t bad = 0;
  const size_t stride = (size_t)gridDim.x * MOSAIC_WG;
  for (size_t i = (size_t)blockIdx.x * MOSAIC_WG + threadIdx.x; i < HW; i += stride) {
    const float v = a[i];
    bad |= v != v ? 1u : 0u;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  mosaic_wave_range(lo, hi, bad);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { sh_lo[wv] = lo; sh_hi[wv] = hi; sh_bad[wv] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    MosaicPart r;
    r.lo = fminf(fminf(sh_lo[0], sh_lo[1]), fminf(sh_lo[2], sh_lo[3]));
    r.hi = fmaxf(fmaxf(sh_hi[0], sh_hi[1]), fmaxf(sh_hi[2], sh_hi[3]));
    r.nan = sh_bad[0] | sh_bad[1] | sh_bad[2] | sh_bad[3];
    r.unused = 0;
    work[(size_t)p * MOSAIC_PARTS + blockIdx.x] = r;
  }
}

__device__ __forceinline__ uint32_t mosaic_quantise(float v, int quant) {
  const double p = (double)v * 255.0;      // exact: 24 + 8 significant bits
  if (v != v) return 0u;
  if (quant) return (uint32_t)fmin(fmax(p + 0.5, 0.0), 255.0);
  return p < 0.0 ? 0u : (p >= 255.0 ? 255u : (uint32_t)p);
}

__global__ void __launch_bounds__(MOSAIC_WG)
mosaic_compose_kernel(MosaicPanels P, int H, int W, int cols, int parts, int blocks_per_row, const MosaicPart* __restrict__ work,
                      const uint8_t* __restrict__ lut, int quant, int bgr, uint8_t* __restrict__ out) {
  __shared__ const float* s_a[MOSAIC_MAX_PANELS];
  __shared__ const float* s_b[MOSAIC_MAX_PANELS];
  __shared__ int s_kind[MOSAIC_MAX_PANELS];
  __shared__ float s_lo[MOSAIC_MAX_PANELS], s_hi[MOSAIC_MAX_PANELS];
  const unsigned Y = blockIdx.x / (unsigned)blocks_per_row, bx = blockIdx.x % (unsigned)blocks_per_row;      // output row, 1 KB block in it
  const int r = (int)(Y / (unsigned)H), y = (int)(Y - (unsigned)r * (unsigned)H);
  const size_t row_bytes = (size_t)3 * (size_t)cols * (size_t)W;
  const uintptr_t row0 = (uintptr_t)out + (size_t)Y * row_bytes, row1 = row0 + row_bytes;      // the row's bytes: [row0, row1)
  const uintptr_t blk0 = (row0 & ~(uintptr_t)3) + (size_t)bx * (MOSAIC_WG * 4);
  if (blk0 >= row1) return;      // (the whole workgroup: the dword grid of this row ends before this block)
  // panels of this output row that the block's bytes fall into (one, or two at a panel border)
  const size_t o_first = blk0 > row0 ? (size_t)(blk0 - row0) : 0;
  const size_t o_last = (size_t)((blk0 + MOSAIC_WG * 4 < row1 ? blk0 + MOSAIC_WG * 4 : row1) - row0) - 1;
  const int c_first = (int)(o_first / 3 / (size_t)W), c_last = (int)(o_last / 3 / (size_t)W);
  if ((int)threadIdx.x < cols) {
    const int p = r * cols + (int)threadIdx.x;
    s_a[threadIdx.x] = P.a[p];
    s_b[threadIdx.x] = P.b[p];
    s_kind[threadIdx.x] = P.kind[p];
  }
  if (threadIdx.x < 64) {
    for (int c = c_first; c <= c_last; c++) {
      const int p = r * cols + c;
      if (P.kind[p] != 2) continue;
      float lo = INFINITY, hi = -INFINITY;
      uint32_t bad = 0;
      if ((int)threadIdx.x < parts) {
        const MosaicPart q = work[(size_t)p * MOSAIC_PARTS + threadIdx.x];
        lo = q.lo; hi = q.hi; bad = q.nan;
      }
      mosaic_wave_range(lo, hi, bad);
      if (threadIdx.x == 0) {      // torch.min / torch.max return NaN when the image holds one
        s_lo[c] = bad ? NAN : lo;
        s_hi[c] = bad ? NAN : hi;
      }
    }
  }
  __syncthreads();
  const uintptr_t addr = blk0 + (size_t)threadIdx.x * 4;      // this lane's aligned dword
  if (addr >= row1) return;
  const size_t HW = (size_t)H * (size_t)W;
  // state of the lane's first byte inside the row: panel column c, pixel x, output channel oc
  const uintptr_t first = addr > row0 ? addr : row0;
  const size_t o = (size_t)(first - row0);
  const unsigned X = (unsigned)(o / 3);
  int oc = (int)(o - (size_t)X * 3);
  int c = (int)(X / (unsigned)W), x = (int)(X - (unsigned)c * (unsigned)W);
  uint32_t word = 0;
  bool full = true;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uintptr_t ba = addr + k;
    if (ba < row0 || ba >= row1) { full = false; continue; }
    const int ch = bgr ? 2 - oc : oc;
    const int kind = s_kind[c];
    const size_t px = (size_t)y * (size_t)W + (size_t)x;
    uint32_t byte;
    if (kind == 2) {
      const float lo = s_lo[c], hi = s_hi[c];
      float t = (s_a[c][px] - lo) / (hi - lo);
      t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);      // (a NaN fails both tests and stays)
      if (t != t) byte = 0u;
      else {
        const int idx = min((int)(t * 256.f), 255);
        byte = lut[idx * 3 + ch];
      }
    } else {
      const size_t i = (size_t)ch * HW + px;
      const float v = kind == 1 ? fabsf(s_a[c][i] - s_b[c][i]) : s_a[c][i];
      byte = mosaic_quantise(v, quant);
    }
    word |= byte << (8 * k);
    if (++oc == 3) {
      oc = 0;
      if (++x == W) { x = 0; c++; }
    }
  }
  if (full) *reinterpret_cast<uint32_t*>(addr) = word;
  else {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uintptr_t ba = addr + k;
      if (ba >= row0 && ba < row1) *reinterpret_cast<uint8_t*>(ba) = (uint8_t)(word >> (8 * k));
    }
  }
}

void launch_mosaic(int H, int W, int rows, int cols, const MosaicPanels& panels, const uint8_t* lut, int quant, int bgr, void* work, uint8_t* out,
                   hipStream_t s) {
  const size_t HW = (size_t)H * (size_t)W;
  const int parts = mosaic_parts(HW);
  bool any_depth = false;
  for (int p = 0; p < rows * cols; p++) any_depth = any_depth || panels.kind[p] == 2;
  if (any_depth)      // (without a depth panel nobody reads `work`: the launch would do nothing)
    hipLaunchKernelGGL(mosaic_range_kernel, dim3(parts, rows * cols), dim3(MOSAIC_WG), 0, s, panels, HW, (MosaicPart*)work);
  // dwords that can hold a row's bytes at the worst alignment of its first byte: ceil((3 + row_bytes) / 4)
  const size_t row_bytes = (size_t)3 * (size_t)cols * (size_t)W;
  const size_t row_dwords = (row_bytes + 3 + 3) / 4;
  const int blocks_per_row = (int)((row_dwords + MOSAIC_WG - 1) / MOSAIC_WG);
  const size_t blocks = (size_t)blocks_per_row * (size_t)rows * (size_t)H;
  hipLaunchKernelGGL(mosaic_compose_kernel, dim3((unsigned)blocks), dim3(MOSAIC_WG), 0, s, panels, H, W, cols, parts, blocks_per_row,
                     (const MosaicPart*)work, lut, quant, bgr, out);
}

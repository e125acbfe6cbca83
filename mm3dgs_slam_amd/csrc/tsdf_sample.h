// What the dense volume (tsdf.hip) and the voxel-block volume (tsdf_sparse.hip) share, each stated once so that the two cannot drift: the
// update of one sample by one view, the marching-tetrahedra case tables, and the layout of the extraction's work buffer over a flat run of
// samples.  The kernels that only see that flat run (state, scan, base) stay in tsdf.hip and are launched through the two helpers below.
#pragma once
#include <math.h>
#include "block_ops.h"
#include "fused_api.h"
#include "view_pixel.h"

// ---- one sample, one view ----------------------------------------------------------------------------------------------------------
// The sample at the world point (pw0, pw1, pw2) with its two volume words at tw / rw.  In double from the float32 inputs, no contraction
// (the host statement rounds alike); z <= 0, a pixel outside the image or one that fails the point cloud's validity test, or sdf < -trunc
// end the sample before anything is loaded from the volume.  Running means, rounded to float32 once at the 8- and 16-byte stores.
__device__ __forceinline__ void tsdf_sample_update(const TsdfView& v, const Rigid& g, size_t hw, double pw0, double pw1, double pw2, float2* __restrict__ tw,
                                                   float4* __restrict__ rw, uint32_t& nupd, uint32_t& ncup) {
#pragma clang fp contract(off)
  const double z = g.R[2][0] * pw0 + g.R[2][1] * pw1 + g.R[2][2] * pw2 + g.t[2];
  if (!(z > 0.0)) return;
  const double x = g.R[0][0] * pw0 + g.R[0][1] * pw1 + g.R[0][2] * pw2 + g.t[0];
  const double y = g.R[1][0] * pw0 + g.R[1][1] * pw1 + g.R[1][2] * pw2 + g.t[1];
  const double fu = floor(v.fx * x / z + v.cx + 0.5), fv = floor(v.fy * y / z + v.cy + 0.5);
  if (!(fu >= 0.0 && fu < (double)v.W && fv >= 0.0 && fv < (double)v.H)) return;      // (a NaN fails)
  const size_t pix = (size_t)(int)fv * (size_t)v.W + (size_t)(int)fu;
  float d;
  if (!view_pixel_valid(v.depth, v.sil, v.sil_min, v.depth_max, pix, d)) return;
  const double sdf = (double)d - z;
  if (sdf < -v.trunc) return;
  // the sample is seen: from here on the volume is read and written
  double s = sdf / v.trunc;
  s = s < 1.0 ? s : 1.0;
  const float2 t = *tw;
  const double T = (double)t.x, W = (double)t.y;
  *tw = make_float2((float)((T * W + s) / (W + 1.0)), (float)(W + 1.0));      // one 8-byte store
  nupd++;
  if (sdf <= v.trunc) {
    const float4 c = *rw;
    const double Cw = (double)c.w;
    *rw = make_float4((float)(((double)c.x * Cw + (double)v.color[pix]) / (Cw + 1.0)), (float)(((double)c.y * Cw + (double)v.color[hw + pix]) / (Cw + 1.0)),
                      (float)(((double)c.z * Cw + (double)v.color[2 * hw + pix]) / (Cw + 1.0)), (float)(Cw + 1.0));      // one 16-byte store
    ncup++;
  }
}

// ---- marching tetrahedra: the work buffer over n samples -------------------------------------------------------------------------------
#define TM_TB 256
// work = [256 B header: uint64 vertices, triangles][state byte per sample: bit 0 known, bit 1 inside][cube byte per sample: 0x80 valid | triangles]
//        [edge mask byte per sample: bit d][uint32 vertex base per sample][uint32 triangle base per cube][per-256 vertex counts][per-256 triangle counts]
struct TmWork { unsigned long long* hdr; uint8_t* state; uint8_t* cube; uint8_t* vmask; uint32_t* vbase; uint32_t* tbase; uint32_t* vcounts; uint32_t* tcounts; };
static inline size_t tm_nb(size_t n) { return (n + TM_TB - 1) / TM_TB; }
static inline TmWork tm_work(void* base, size_t n, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  TmWork w;
  w.hdr = c.take<unsigned long long>(2);
  w.state = c.take<uint8_t>(n);
  w.cube = c.take<uint8_t>(n);
  w.vmask = c.take<uint8_t>(n);
  w.vbase = c.take<uint32_t>(n);
  w.tbase = c.take<uint32_t>(n);
  w.vcounts = c.take<uint32_t>(tm_nb(n));
  w.tcounts = c.take<uint32_t>(tm_nb(n));
  if (bytes) *bytes = c.at;
  return w;
}
struct TmEmit { double o[3], voxel; unsigned long long vcap, tcap; };

// the two ends of a plan that see only the flat run of n samples (tsdf.hip): the state bytes before the cubes and edges are counted, and
// the scan of both per-256 counts with the per-sample bases behind them
void launch_tm_state(size_t n, const void* tsdf_w, float min_weight, const TmWork& w, hipStream_t s);
void launch_tm_scan_base(size_t n, const TmWork& w, uint64_t* counters, hipStream_t s);

// ---- marching tetrahedra: the case tables ------------------------------------------------------------------------------------------
// The triangles of a positively oriented tetrahedron by its 4-bit inside mask (bit v: vertex v of the path is inside), as
// count | six 3-bit edge ids << 2; edges 0..5 = the vertex pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  One vertex apart: the triangle of its
// three edges; two and two: the quadrilateral (a,c) (a,d) (b,d) (b,c) as two triangles; wound so that the normal points from the inside
// vertices to the outside ones (mesh.py derives the same table by rule and checks the winding numerically).
#define TM1(a, b, c) (1u | (a##u << 2) | (b##u << 5) | (c##u << 8))
#define TM2(a, b, c, d, e, f) (2u | (a##u << 2) | (b##u << 5) | (c##u << 8) | (d##u << 11) | (e##u << 14) | (f##u << 17))
static __device__ const uint32_t TM_CASES[16] = {0u, TM1(0, 1, 2), TM1(0, 4, 3), TM2(1, 2, 4, 1, 4, 3), TM1(1, 3, 5), TM2(0, 5, 2, 0, 3, 5), TM2(0, 4, 5, 0, 5, 1),
                                                 TM1(2, 4, 5), TM1(2, 5, 4), TM2(0, 1, 5, 0, 5, 4), TM2(0, 5, 3, 0, 2, 5), TM1(1, 5, 3), TM2(1, 3, 4, 1, 4, 2),
                                                 TM1(0, 3, 4), TM1(0, 2, 1), 0u};
// cube corners (bit 0 x, bit 1 y, bit 2 z) of the path's two middle vertices, by tetrahedron = axis permutation in lexicographic order:
// (x,y,z) (x,z,y) (y,x,z) (y,z,x) (z,x,y) (z,y,x); the odd permutations (1, 2, 5) mirror the tetrahedron: their triangles swap two corners
static __device__ const uint8_t TM_MID1[6] = {1, 1, 2, 2, 4, 4};
static __device__ const uint8_t TM_MID2[6] = {3, 5, 3, 6, 5, 6};
#define TM_ODD 0x26u
static __device__ const uint8_t TM_EDGE_LO[6] = {0, 0, 0, 1, 1, 2};
static __device__ const uint8_t TM_EDGE_HI[6] = {1, 2, 3, 2, 3, 3};

__device__ __forceinline__ unsigned tm_tet_mask(unsigned inside, int k) {
  return (inside & 1u) | (((inside >> TM_MID1[k]) & 1u) << 1) | (((inside >> TM_MID2[k]) & 1u) << 2) | (((inside >> 7) & 1u) << 3);
}

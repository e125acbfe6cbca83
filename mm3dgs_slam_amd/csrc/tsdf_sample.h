// What the dense volume (tsdf.hip) and the voxel-block volume (tsdf_sparse.hip) share about integration, stated once so that the two cannot
// drift: the update of one sample by one view.  What they share about extraction is tsdf_march.h.
#pragma once
#include <math.h>
#include "block_ops.h"
#include "fused_api.h"
#include "view_pixel.h"

// ---- one sample, one view ----------------------------------------------------------------------------------------------------------
// The sample at the world point (pw0, pw1, pw2) with its two volume words at tw / rw.  In double from the float32 inputs, no contraction
// (the host statement rounds alike), the projection through view_pixel.h's statements (culling's too); z <= 0, a pixel outside the image or
// one that fails the point cloud's validity test, or sdf < -trunc end the sample before anything is loaded from the volume.  Running means,
// rounded to float32 once at the 8- and 16-byte stores.
__device__ __forceinline__ void tsdf_sample_update(const TsdfView& v, const Rigid& g, size_t hw, double pw0, double pw1, double pw2, float2* __restrict__ tw,
                                                   float4* __restrict__ rw, uint32_t& nupd, uint32_t& ncup) {
#pragma clang fp contract(off)
  double x, y, z;
  size_t pix;
  view_to_camera(g, pw0, pw1, pw2, x, y, z);      // (x and y are needed only behind the test of z)
  if (!(z > 0.0) || !view_pixel_index(v, x, y, z, pix)) return;
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

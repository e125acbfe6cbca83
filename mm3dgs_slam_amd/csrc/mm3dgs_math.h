// Device-side maths shared by the per-Gaussian kernels (preprocess.hip, fused.hip): SH basis, quaternion -> rotation,
// 3D covariance, EWA projection to a 2D conic, and the pieces of its chain rule and of the Adam update that several kernels must evaluate
// bit-identically.  Conventions: see preprocess.hip's header.
// Floating-point contraction: every helper here is inlined into its caller and INHERITS THE INCLUDING FILE'S CONTRACTION MODE (fused.hip sets
// `#pragma clang fp contract(on)` before this include: a product and a sum inside one source expression fuse, nothing else does;
// preprocess.hip compiles under hipcc's default).  Each expression below is therefore one rounding recipe: do not split or merge them, and
// keep the temporaries where they are.
#pragma once
#include "mm3dgs_common.h"

#define PP_BLOCK 256

#define SH_C0 0.28209479177387814f
#define SH_C1 0.4886025119029199f
#define SH_C2_0 1.0925484305920792f
#define SH_C2_1 -1.0925484305920792f
#define SH_C2_2 0.31539156525252005f
#define SH_C2_3 -1.0925484305920792f
#define SH_C2_4 0.5462742152960396f
#define SH_C3_0 -0.5900435899266435f
#define SH_C3_1 2.890611442640554f
#define SH_C3_2 -0.4570457994644658f
#define SH_C3_3 0.3731763325901154f
#define SH_C3_4 -0.4570457994644658f
#define SH_C3_5 1.445305721320277f
#define SH_C3_6 -0.5900435899266435f

// Real SH basis values b[0..(deg+1)^2) at unit direction (x,y,z).
__device__ __forceinline__ void sh_basis(int deg, float x, float y, float z, float* b) {
  b[0] = SH_C0;
  if (deg > 0) {
    b[1] = -SH_C1 * y; b[2] = SH_C1 * z; b[3] = -SH_C1 * x;
    if (deg > 1) {
      float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      b[4] = SH_C2_0 * xy; b[5] = SH_C2_1 * yz; b[6] = SH_C2_2 * (2.f * zz - xx - yy);
      b[7] = SH_C2_3 * xz; b[8] = SH_C2_4 * (xx - yy);
      if (deg > 2) {
        b[9] = SH_C3_0 * y * (3.f * xx - yy);
        b[10] = SH_C3_1 * xy * z;
        b[11] = SH_C3_2 * y * (4.f * zz - xx - yy);
        b[12] = SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy);
        b[13] = SH_C3_4 * x * (4.f * zz - xx - yy);
        b[14] = SH_C3_5 * z * (xx - yy);
        b[15] = SH_C3_6 * x * (xx - 3.f * yy);
      }
    }
  }
}
// d b[k] / d(x,y,z)
__device__ __forceinline__ void sh_basis_grad(int deg, float x, float y, float z, float* gx, float* gy, float* gz) {
  gx[0] = gy[0] = gz[0] = 0.f;
  if (deg > 0) {
    gx[1] = 0.f; gy[1] = -SH_C1; gz[1] = 0.f;
    gx[2] = 0.f; gy[2] = 0.f; gz[2] = SH_C1;
    gx[3] = -SH_C1; gy[3] = 0.f; gz[3] = 0.f;
    if (deg > 1) {
      float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      gx[4] = SH_C2_0 * y; gy[4] = SH_C2_0 * x; gz[4] = 0.f;
      gx[5] = 0.f; gy[5] = SH_C2_1 * z; gz[5] = SH_C2_1 * y;
      gx[6] = SH_C2_2 * -2.f * x; gy[6] = SH_C2_2 * -2.f * y; gz[6] = SH_C2_2 * 4.f * z;
      gx[7] = SH_C2_3 * z; gy[7] = 0.f; gz[7] = SH_C2_3 * x;
      gx[8] = SH_C2_4 * 2.f * x; gy[8] = SH_C2_4 * -2.f * y; gz[8] = 0.f;
      if (deg > 2) {
        gx[9] = SH_C3_0 * 6.f * xy; gy[9] = SH_C3_0 * (3.f * xx - 3.f * yy); gz[9] = 0.f;
        gx[10] = SH_C3_1 * yz; gy[10] = SH_C3_1 * xz; gz[10] = SH_C3_1 * xy;
        gx[11] = SH_C3_2 * -2.f * xy; gy[11] = SH_C3_2 * (4.f * zz - xx - 3.f * yy); gz[11] = SH_C3_2 * 8.f * yz;
        gx[12] = SH_C3_3 * -6.f * xz; gy[12] = SH_C3_3 * -6.f * yz; gz[12] = SH_C3_3 * (6.f * zz - 3.f * xx - 3.f * yy);
        gx[13] = SH_C3_4 * (4.f * zz - 3.f * xx - yy); gy[13] = SH_C3_4 * -2.f * xy; gz[13] = SH_C3_4 * 8.f * xz;
        gx[14] = SH_C3_5 * 2.f * xz; gy[14] = SH_C3_5 * -2.f * yz; gz[14] = SH_C3_5 * (xx - yy);
        gx[15] = SH_C3_6 * (3.f * xx - 3.f * yy); gy[15] = SH_C3_6 * -6.f * xy; gz[15] = 0.f;
      }
    }
  }
}

__device__ __forceinline__ void quat_to_R(const float* q, float R[3][3]) {
  float r = q[0], x = q[1], y = q[2], z = q[3];
  R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z); R[0][2] = 2.f * (x * z + r * y);
  R[1][0] = 2.f * (x * y + r * z); R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
  R[2][0] = 2.f * (x * z - r * y); R[2][1] = 2.f * (y * z + r * x); R[2][2] = 1.f - 2.f * (x * x + y * y);
}

// Sigma3 = Mx Mx^T with Mx = R diag(sm)
__device__ __forceinline__ void cov3d_from_scaled_R(const float R[3][3], const float sm[3], float S3[3][3]) {
  float Mx[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) Mx[i][k] = R[i][k] * sm[k];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) S3[i][j] = Mx[i][0] * Mx[j][0] + Mx[i][1] * Mx[j][1] + Mx[i][2] * Mx[j][2];
}

// Sigma3 (symmetric, full 3x3) from scale/rotation or from the 6 upper-triangular values.
__device__ __forceinline__ void load_cov3d(int idx, const float* scales, const float* rots, const float* cov3d,
                                           float mod, float S3[3][3], float R[3][3], float sm[3]) {
  if (cov3d) {
    const float* c = cov3d + (size_t)idx * 6;
    S3[0][0] = c[0]; S3[0][1] = c[1]; S3[0][2] = c[2];
    S3[1][0] = c[1]; S3[1][1] = c[3]; S3[1][2] = c[4];
    S3[2][0] = c[2]; S3[2][1] = c[4]; S3[2][2] = c[5];
  } else {
    float q[4] = {rots[(size_t)idx * 4], rots[(size_t)idx * 4 + 1], rots[(size_t)idx * 4 + 2], rots[(size_t)idx * 4 + 3]};
    quat_to_R(q, R);
    sm[0] = mod * scales[(size_t)idx * 3]; sm[1] = mod * scales[(size_t)idx * 3 + 1]; sm[2] = mod * scales[(size_t)idx * 3 + 2];
    cov3d_from_scaled_R(R, sm, S3);
  }
}

struct Ewa {
  float t[3];      // view-space mean
  float txc, tyc;  // clamped-frustum x,y used inside the Jacobian
  bool in_x, in_y;
  float A[2][3];   // J * Wr
  float J00, J02, J11, J12;
  float a, b, c;   // 2D covariance (+0.3 on the diagonal)
};

__device__ __forceinline__ void ewa_project(const CamDev& cam, const float* V, const float p[3], const float S3[3][3], Ewa& e) {
#pragma unroll
  for (int j = 0; j < 3; j++) e.t[j] = p[0] * V[0 * 4 + j] + p[1] * V[1 * 4 + j] + p[2] * V[2 * 4 + j] + V[3 * 4 + j];
  float tz = e.t[2];
  float limx = 1.3f * cam.tanfovx, limy = 1.3f * cam.tanfovy;
  float txtz = e.t[0] / tz, tytz = e.t[1] / tz;
  e.in_x = (txtz >= -limx) && (txtz <= limx);
  e.in_y = (tytz >= -limy) && (tytz <= limy);
  e.txc = fminf(limx, fmaxf(-limx, txtz)) * tz;
  e.tyc = fminf(limy, fmaxf(-limy, tytz)) * tz;
  if (e.in_x) e.txc = e.t[0];
  if (e.in_y) e.tyc = e.t[1];
  float itz = 1.f / tz, itz2 = itz * itz;
  e.J00 = cam.focal_x * itz; e.J02 = -cam.focal_x * e.txc * itz2;
  e.J11 = cam.focal_y * itz; e.J12 = -cam.focal_y * e.tyc * itz2;
  // Wr[j][i] = V[i][j]  (world->view rotation for column vectors);  A = J * Wr
#pragma unroll
  for (int i = 0; i < 3; i++) {
    e.A[0][i] = e.J00 * V[i * 4 + 0] + e.J02 * V[i * 4 + 2];
    e.A[1][i] = e.J11 * V[i * 4 + 1] + e.J12 * V[i * 4 + 2];
  }
  float AS[2][3];
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int j = 0; j < 3; j++) AS[r][j] = e.A[r][0] * S3[0][j] + e.A[r][1] * S3[1][j] + e.A[r][2] * S3[2][j];
  e.a = AS[0][0] * e.A[0][0] + AS[0][1] * e.A[0][1] + AS[0][2] * e.A[0][2] + 0.3f;
  e.b = AS[0][0] * e.A[1][0] + AS[0][1] * e.A[1][1] + AS[0][2] * e.A[1][2];
  e.c = AS[1][0] * e.A[1][0] + AS[1][1] * e.A[1][1] + AS[1][2] * e.A[1][2] + 0.3f;
}

// Radius and tile rectangle of a splat at pixel (px, py) with 2D covariance diagonal (a, c) and determinant det: 3 sigma of the larger
// eigenvalue, clipped to the tile grid.  r0 = minx | miny << 16, r1 = maxx | maxy << 16 (GeomView.rect); hit: the rectangle holds a tile.
struct TileRect { uint32_t r0, r1; int32_t rad; bool hit; };
__device__ __forceinline__ TileRect splat_tile_rect(const CamDev& cam, float px, float py, float a, float c, float det) {
  TileRect t = {0u, 0u, 0, false};
  float mid = 0.5f * (a + c);
  float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
  float rf = ceilf(3.f * sqrtf(lam));
  float gxf = (float)cam.gx + 1.f, gyf = (float)cam.gy + 1.f;
  int minx = min(cam.gx, max(0, (int)fminf(fmaxf((px - rf) / TILE, -1.f), gxf)));
  int miny = min(cam.gy, max(0, (int)fminf(fmaxf((py - rf) / TILE, -1.f), gyf)));
  int maxx = min(cam.gx, max(0, (int)fminf(fmaxf((px + rf + (TILE - 1)) / TILE, -1.f), gxf)));
  int maxy = min(cam.gy, max(0, (int)fminf(fmaxf((py + rf + (TILE - 1)) / TILE, -1.f), gyf)));
  t.hit = (maxx - minx) * (maxy - miny) > 0;
  if (t.hit) {
    t.rad = (int32_t)fminf(rf, 2.0e9f);
    t.r0 = (uint32_t)minx | ((uint32_t)miny << 16);
    t.r1 = (uint32_t)maxx | ((uint32_t)maxy << 16);
  }
  return t;
}

// Homogeneous projection of a point p under the row-vector matrix PV: clip x, y, w and pw = 1 / (w + 1e-7).
struct HomPoint { float hx, hy, hw, pw; };
__device__ __forceinline__ HomPoint hom_project(const float* PV, const float p[3]) {
  HomPoint h;
  h.hx = p[0] * PV[0] + p[1] * PV[4] + p[2] * PV[8] + PV[12];
  h.hy = p[0] * PV[1] + p[1] * PV[5] + p[2] * PV[9] + PV[13];
  h.hw = p[0] * PV[3] + p[1] * PV[7] + p[2] * PV[11] + PV[15];
  h.pw = 1.f / (h.hw + 1e-7f);
  return h;
}

// d/d(conic) (gA, gB, gC) -> d/d(2D covariance) (da, db, dcc) of Sigma2 = [[a, b], [b, c]], conic = (c, -b, a) / det.
// G2 = dL/dSigma2 is formed as 1/det [[gC, -gB/2], [-gB/2, gA]] + kappa adj(Sigma2), kappa = -(c gA - b gB + a gC) / det^2 -- NOT the expanded
// closed form (-c^2 gA + b c gB - b^2 gC) / det^2 etc.: for a thin rotated ellipse (a c / det ~ 50) each expanded entry cancels ~75-fold on its
// own, and the log-scale gradient of the long axis is v^T G2 v along the axis where G2 cancels ~50-fold again: independent 2e-6 errors of the
// entries came out as 2e-4 (measured with a float32 numpy probe: tools/cov_chain_probe.py).  In this form the cancelling part is ONE scalar
// times adj(Sigma2), whose quadratic form along the long axis is small by construction: 2e-4 -> 1.5e-5 on the same splat.
struct Cov2dGrad { float da, db, dcc; };
__device__ __forceinline__ Cov2dGrad conic_grad_to_cov2d(float a, float b, float c, float gA, float gB, float gC) {
  const float det = a * c - b * b, idet = 1.f / det;
  const float kappa = -(c * gA - b * gB + a * gC) * idet * idet;
  Cov2dGrad g;
  g.da = gC * idet + kappa * c;
  g.db = -gB * idet - 2.f * (kappa * b);
  g.dcc = gA * idet + kappa * a;
  return g;
}

// d/d(2D covariance) -> GA = G2 A (2x3) and dA = 2 G2 A Sigma3, with A = J Wr of ewa_project (Sigma2 = A Sigma3 A^T)
// (preprocess.hip, compiled under hipcc's default contraction, keeps its own copy of this one and of dcov3d_to_scale_rot: through the helpers its
//  gradients moved in their last bits -- preprocess_bwd_kernel says which and by how much.  Every other helper here serves both files bit for bit.)
__device__ __forceinline__ void cov2d_grad_to_dA(const Ewa& e, const float S3[3][3], const Cov2dGrad& g, float GA[2][3], float dA[2][3]) {
  const float G2[2][2] = {{g.da, 0.5f * g.db}, {0.5f * g.db, g.dcc}};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    GA[0][i] = G2[0][0] * e.A[0][i] + G2[0][1] * e.A[1][i];
    GA[1][i] = G2[1][0] * e.A[0][i] + G2[1][1] * e.A[1][i];
  }
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int r = 0; r < 2; r++) dA[r][j] = 2.f * (GA[r][0] * S3[0][j] + GA[r][1] * S3[1][j] + GA[r][2] * S3[2][j]);
}

// dSigma3 = A^T G2 A from A and GA = G2 A.
// dSigma3 is symmetric in exact arithmetic; in float32 the two triangles round differently, and their difference IS the rotation
// gradient of an isotropic Gaussian with identity rotation (every freshly seeded one, slam/mapper.py:644-668): rounding noise that
// Adam(eps=1e-15) turns into full +-lr steps of the quaternion.  torch's autograd of Sigma = L L^T forms (dSigma + dSigma^T) L and
// is exactly zero there; so is this once the triangles are averaged (found with the G9 runs of the reference's own classes:
// pose error to the reference 1.4e-5 -> 8e-8 after the first tracked frame).
__device__ __forceinline__ void cov2d_grad_to_dcov3d(const float A[2][3], const float GA[2][3], float dS[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) dS[i][j] = A[0][i] * GA[0][j] + A[1][i] * GA[1][j];
  const float s01 = 0.5f * (dS[0][1] + dS[1][0]), s02 = 0.5f * (dS[0][2] + dS[2][0]), s12 = 0.5f * (dS[1][2] + dS[2][1]);
  dS[0][1] = s01; dS[1][0] = s01; dS[0][2] = s02; dS[2][0] = s02; dS[1][2] = s12; dS[2][1] = s12;
}

// dSigma3 -> d/d(scales) and dL/dR through Sigma3 = Mx Mx^T, Mx = R diag(sm), sm = mod * scales:  dMx = 2 dSigma3 Mx
__device__ __forceinline__ void dcov3d_to_scale_rot(const float dS[3][3], const float R[3][3], const float sm[3], float mod, float ds[3],
                                                    float dR[3][3]) {
  float dM[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) dM[i][k] = 2.f * (dS[i][0] * R[0][k] + dS[i][1] * R[1][k] + dS[i][2] * R[2][k]) * sm[k];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    ds[k] = mod * (dM[0][k] * R[0][k] + dM[1][k] * R[1][k] + dM[2][k] * R[2][k]);
#pragma unroll
    for (int i = 0; i < 3; i++) dR[i][k] = dM[i][k] * sm[k];
  }
}

// d/d(pixel position) (gpx, gpy) -> d/d(NDC) (gnx, gny) -> d/d(clip x, y, w) -> added to dm, the gradient of the point h was projected from:
// pix = ((ndc + 1) S - 1) / 2, ndc = hom.xy / (hom.w + 1e-7)
struct ScreenGrad { float gnx, gny, dhx, dhy, dhw; };
__device__ __forceinline__ ScreenGrad pixel_grad_to_dmean(const CamDev& cam, const float* PV, const HomPoint& h, float gpx, float gpy, float dm[3]) {
  ScreenGrad s;
  s.gnx = gpx * 0.5f * cam.W;
  s.gny = gpy * 0.5f * cam.H;
  s.dhx = s.gnx * h.pw; s.dhy = s.gny * h.pw; s.dhw = -(s.gnx * h.hx + s.gny * h.hy) * h.pw * h.pw;
#pragma unroll
  for (int i = 0; i < 3; i++) dm[i] += PV[i * 4 + 0] * s.dhx + PV[i * 4 + 1] * s.dhy + PV[i * 4 + 3] * s.dhw;
  return s;
}

// d/dJ (the four non-zero entries of the perspective Jacobian) -> d/d(view-space mean), the +-1.3 tan-fov clamp of ewa_project included
__device__ __forceinline__ void dJ_to_dmean(const CamDev& cam, const Ewa& e, float dJ00, float dJ02, float dJ11, float dJ12, float dm[3]) {
  const float tz = e.t[2], itz = 1.f / tz, itz2 = itz * itz, itz3 = itz2 * itz;
  dm[0] = e.in_x ? -cam.focal_x * itz2 * dJ02 : 0.f;
  dm[1] = e.in_y ? -cam.focal_y * itz2 * dJ12 : 0.f;
  dm[2] = -cam.focal_x * itz2 * dJ00 - cam.focal_y * itz2 * dJ11 + 2.f * cam.focal_x * e.txc * itz3 * dJ02 +
          2.f * cam.focal_y * e.tyc * itz3 * dJ12;
}

// dL/dR -> dL/dq through quat_to_R at the quaternion q = (r, x, y, z)
__device__ __forceinline__ void dR_to_dq(const float q[4], const float dR[3][3], float dq[4]) {
  const float r = q[0], x = q[1], y = q[2], z = q[3];
  dq[0] = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
  dq[1] = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r * dR[1][2] + z * dR[2][0] +
                 r * dR[2][1] - 2.f * x * dR[2][2]);
  dq[2] = 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] +
                 z * dR[2][1] - 2.f * y * dR[2][2]);
  dq[3] = 2.f * (-2.f * z * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - 2.f * z * dR[1][1] +
                 y * dR[1][2] + x * dR[2][0] + y * dR[2][1]);
}
// the same for R(q / |q|): qn = q / |q|, inv = 1 / |q|; the normalisation projects the gradient onto qn's tangent space
__device__ __forceinline__ void dR_to_dq_raw(const float qn[4], float inv, const float dR[3][3], float dq_raw[4]) {
  float dq[4];
  dR_to_dq(qn, dR, dq);
  const float dot = qn[0] * dq[0] + qn[1] * dq[1] + qn[2] * dq[2] + qn[3] * dq[3];
#pragma unroll
  for (int k = 0; k < 4; k++) dq_raw[k] = (dq[k] - qn[k] * dot) * inv;
}

// One element of torch.optim.Adam's update (slam/gaussian_model.py:143-195, slam/tracker.py:233-246): omb1 = 1 - beta1, omb2 = 1 - beta2,
// bc2s = sqrt(1 - beta2^t), step = lr / (1 - beta1^t).  With eps = 1e-15 a one-ulp disagreement between two evaluations of this is a full
// +-lr step: every kernel that steps a parameter calls this.
struct AdamElem { float p, m, v; };
__device__ __forceinline__ void adam_moments(float m, float v, float g, float omb1, float beta2, float omb2, AdamElem& r) {
  r.m = m + (g - m) * omb1;                 // exp_avg.lerp_(grad, 1 - beta1)
  r.v = v * beta2 + g * g * omb2;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
}
// (the two halves are separate for the kernels that load p only after the moments are stored: requesting it earlier cost
//  slam_adam_project_kernel<true, true, 2> four VGPRs and a wave of occupancy)
__device__ __forceinline__ float adam_param(float p, const AdamElem& r, float bc2s, float eps, float step) {
  return p - step * (r.m / (sqrtf(r.v) / bc2s + eps));
}
__device__ __forceinline__ AdamElem adam_elem(float p, float m, float v, float g, float omb1, float beta2, float omb2, float bc2s, float eps,
                                              float step) {
  AdamElem r;
  adam_moments(m, v, g, omb1, beta2, omb2, r);
  r.p = adam_param(p, r, bc2s, eps, step);
  return r;
}

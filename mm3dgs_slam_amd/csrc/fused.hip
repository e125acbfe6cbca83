// Fused SLAM render path (section 7 step 6): one projection kernel that folds in
//   * the pose transform the reference does in torch in `transform_means_python` mode (slam/renderer.py:142-153):
//       means_cam = R(q/|q|) x + t, viewmatrix = I  -- and, in the backward, the P -> 12 float reduction that is the
//       pose gradient (dR = sum dmeans_cam (x) x, dt = sum dmeans_cam) followed by the chain rule to (q, t);
//   * the depth bundle [z, 1, z^2] of slam/renderer.py:26-43 (only z is stored; the compositor channels are derived);
//   * the GaussianModel activations of slam/gaussian_model.py:108-137 (exp, normalize, sigmoid, SH degree 0 -> RGB
//     with the +0.5 / clamp of renderer.py:188-189) and their chain rule in the backward;
//   * in the backward: the densification statistics of slam/mapper.py:887-899 / gaussian_model.py:594-598.
// Reference quirk kept: the Gaussians' rotations are NOT composed with the camera rotation in this mode
// (slam/renderer.py:152,171-173), i.e. the covariance stays in world orientation while the mean is in camera space.
// Everything downstream (scan, scatter, sort, compositors) is the generic pipeline with C = 6.
//
// Floating-point contraction in this translation unit follows the SOURCE (a * b + c inside one expression is an fma, nothing else is):
// hipcc's default lets the optimiser fuse across statements, and what it fuses then depends on the code around an inlined function --
// the projection inlined behind the optimiser step (slam_bwd_project_kernel) rounded the conics of ~9 % of the splats one bit away from
// the standalone projection kernel's, which Adam(eps = 1e-15) amplifies into visibly different maps within a few frames.
#pragma clang fp contract(on)
#include "mm3dgs_math.h"
#include "fused_api.h"
#include "composite_common.h"
#include "tile_mask.h"

#define FB 256
// workgroup size of the backward projection (= its rows of pose partials): independent of the projection kernels' 256.  With the per-block
// gather (its wave-level work lists, 28 KB of LDS) 128 lanes spread better over the CUs (mapping 33.1 -> 30.8 us); with one record per
// (tile, splat) pair the kernel is two short rounds of loads and 256 lanes win again (mapping 19.1 -> 18.6 us, and the pose-finish
// kernel reads half the rows: 8.4 -> 7.3 us).  The partial-row region of the scratch holds (P / 256 + 1) * 64 floats: 64-lane groups would not fit.
#define SLAM_BWD_FB 256
#define SH_C0F 0.28209479177387814f

struct PoseDev { float R[3][3]; float t[3]; float qn[4]; float inv_norm; };

__device__ __forceinline__ PoseDev load_pose(const float* __restrict__ pose) {
  PoseDev p;
  float w = pose[0], x = pose[1], y = pose[2], z = pose[3];
  float n = sqrtf(w * w + x * x + y * y + z * z);
  p.inv_norm = 1.f / n;
  p.qn[0] = w * p.inv_norm; p.qn[1] = x * p.inv_norm; p.qn[2] = y * p.inv_norm; p.qn[3] = z * p.inv_norm;
  quat_to_R(p.qn, p.R);
  p.t[0] = pose[4]; p.t[1] = pose[5]; p.t[2] = pose[6];
  return p;
}

// A launch's uniform inputs -- a pose (7 floats) and the 16 floats of cam.proj -- read ONCE, as the kernel's first instructions, into
// registers: before the first store of the kernel they are scalar loads that share the round trip of the kernel arguments.  Dereferenced
// where they are used, behind stores the pointers may alias, each is a memory round trip of its own that every wave of the one-round grid
// waits for alone (the next view's pose behind the Adam stores, cam.proj -- as vector loads -- behind the splat record).  The helpers below
// take `pose` and `PV` as pointers and never go back to cam.proj or SlamIn::pose: the kernels built on slam_bwd_body hand them these arrays.
struct PoseProj { float pose[7]; float PV[16]; };
__device__ __forceinline__ PoseProj load_pose_proj(const float* __restrict__ pose, const float* __restrict__ proj) {
  PoseProj u;
#pragma unroll
  for (int k = 0; k < 7; k++) u.pose[k] = pose[k];
#pragma unroll
  for (int k = 0; k < 16; k++) u.PV[k] = proj[k];
  return u;
}

// raw rotation quaternion q[4] and log-scales ls[3] -> normalised quaternion, R, scales, Sigma = (R S)(R S)^T
__device__ __forceinline__ void slam_cov3d_vals(const float q[4], const float ls[3], bool isotropic, float mod, float S3[3][3],
                                                float R[3][3], float sm[3], float qn[4], float& qinv) {
  float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  n = fmaxf(n, 1e-12f);  // torch.nn.functional.normalize eps
  qinv = 1.f / n;
  qn[0] = q[0] * qinv; qn[1] = q[1] * qinv; qn[2] = q[2] * qinv; qn[3] = q[3] * qinv;
  quat_to_R(qn, R);
  // accurate exp: the activations are inputs of everything downstream and there are 3 per Gaussian, so the fast v_exp path buys
  // nothing here (measured: pose gradients a little closer to the oracle, d/d(log-scale) unchanged)
  sm[0] = mod * expf(ls[0]);
  sm[1] = isotropic ? sm[0] : mod * expf(ls[1]);
  sm[2] = isotropic ? sm[0] : mod * expf(ls[2]);
  cov3d_from_scaled_R(R, sm, S3);
}

__device__ __forceinline__ void slam_cov3d(const SlamIn& in, int idx, float mod, float S3[3][3], float R[3][3], float sm[3],
                                           float qn[4], float& qinv) {
  const float* qp = in.rotation + (size_t)idx * 4;
  const float* lp = in.scaling + (size_t)idx * 3;
  const float q[4] = {qp[0], qp[1], qp[2], qp[3]}, ls[3] = {lp[0], lp[1], lp[2]};
  slam_cov3d_vals(q, ls, in.isotropic != 0, mod, S3, R, sm, qn, qinv);
}

// Projection of one Gaussian (lane): pose transform, activations, EWA, SH degree 0 -> RGB, [z, 1, z^2], tile rectangle, block
// rectangle.  Writes the splat record, depth, clamp bits, radii and rect; returns what the binning half of the kernels needs.
struct Projected { uint32_t r0, r1; float4 sA, sB; BlkRect br; float z; int32_t rad; uint32_t cl; };
// raw parameters of one Gaussian, as the projection consumes them
struct RawGaussian { float x[3], q[4], ls[3], fd[3], op; };

// projection of a Gaussian whose raw parameters are already in registers (loaded by slam_project_one, or just stepped by the map's
// in-kernel Adam: slam_bwd_project_kernel)
// world: Mm3dgsSlamInputs.world_means (transform_means_python: false): the same camera-space mean p = R x + t, but the EWA projection runs
// under the full view matrix (covariance rotated by R) and the depth bundle carries the reference's literal z' (third column of R . x)
__device__ __forceinline__ void pose_view_matrix(const PoseDev& ps, float V[16]) {      // row-vector convention: V = w2c^T
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) V[i * 4 + j] = ps.R[j][i];
    V[i * 4 + 3] = 0.f;
    V[12 + i] = ps.t[i];
  }
  V[15] = 1.f;
}
// The tracking compositor's pose chain.  With the map frozen and the means pre-transformed (the shipped mode), dL/d(camera-space mean) of a
// splat is LINEAR in the moments its gradient records hold:   dm = Kp (Mx, My) + Kq (Mxx, Mxy, Myy) + e_z cz   -- Kp = the screen-position
// chain (pixel centre <- homogeneous point <- p, times the conic: gpx = -(qa Mx + qb My), gpy = -(qc My + qb Mx)), Kq = the covariance chain
// (conic <- 2D covariance <- J(p) S3 J(p)^T, the +-1.3 tanfov clamp included), both the helpers slam_bwd_body calls, evaluated on unit
// inputs.  The projection stage writes { Kp, Kq, x } per visible Gaussian; the compositor applies it per (block, splat) and sums dm (x) [x; 1]
// straight into the tile's pose-gradient row: no gradient record leaves the compositor, no per-tile combine, no backward projection launch.
__device__ __forceinline__ void pose_chain_record(const CamDev& cam, const float PV[16], const float p[3], const float x[3], const Ewa& e,
                                                  const float S3[3][3], float qa, float qb, float qc, float pw, float hx, float hy,
                                                  float* __restrict__ rec) {
  // covariance chain: (gA, gB, gC) = d/d(conic) -> dm, column by column
  float Kq[3][3];
#pragma unroll
  for (int col = 0; col < 3; col++) {
    // Kq's columns act on (Mxx, Mxy, Myy): gA = -1/2 Mxx, gB = -Mxy, gC = -1/2 Myy
    const float gA = col == 0 ? -0.5f : 0.f, gB = col == 1 ? -1.f : 0.f, gC = col == 2 ? -0.5f : 0.f;
    float GA[2][3], dA[2][3], dm[3];
    cov2d_grad_to_dA(e, S3, conic_grad_to_cov2d(e.a, e.b, e.c, gA, gB, gC), GA, dA);
    dJ_to_dmean(cam, e, dA[0][0], dA[0][2], dA[1][1], dA[1][2], dm);      // (view = identity: dJ = dA)
    Kq[0][col] = dm[0]; Kq[1][col] = dm[1]; Kq[2][col] = dm[2];
  }
  // screen-position chain: (gpx, gpy) -> dm, then gpx = -(qa Mx + qb My), gpy = -(qc My + qb Mx)
  float Jp[3][2];
  const float sx = 0.5f * cam.W, sy = 0.5f * cam.H;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    // d(px)/dp_i = sx pw (PV[i][0] - hx pw PV[i][3]),  d(py)/dp_i = sy pw (PV[i][1] - hy pw PV[i][3])
    Jp[i][0] = PV[i * 4 + 0] * (sx * pw) - PV[i * 4 + 3] * (sx * hx * pw * pw);
    Jp[i][1] = PV[i * 4 + 1] * (sy * pw) - PV[i * 4 + 3] * (sy * hy * pw * pw);
  }
  float4* o = (float4*)rec;
  float Kp[3][2];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    Kp[i][0] = -(Jp[i][0] * qa + Jp[i][1] * qb);      // coefficient of Mx
    Kp[i][1] = -(Jp[i][0] * qb + Jp[i][1] * qc);      // coefficient of My
  }
  o[0] = make_float4(Kp[0][0], Kp[0][1], Kp[1][0], Kp[1][1]);
  o[1] = make_float4(Kp[2][0], Kp[2][1], Kq[0][0], Kq[0][1]);
  o[2] = make_float4(Kq[0][2], Kq[1][0], Kq[1][1], Kq[1][2]);
  o[3] = make_float4(Kq[2][0], Kq[2][1], Kq[2][2], x[0]);
  o[4] = make_float4(x[1], x[2], 0.f, 0.f);
}

// The (unnormalised) SH viewing direction v of the three sources, Mm3dgsSlamInputs.sh_dir (ABI 211; slam/renderer.py:117-124,179-193):
//   0  p = R x + t, the camera-space mean: the shipped mode hands the rasterizer pre-transformed means and campos = 0
//   1  x, the world mean about the ORIGIN: convert_SHs_python evaluates SH on pc.get_xyz - camera_pos with the shipped mode's camera_pos = 0
//   2  x - c = x + R^T t, the world mean seen from the camera centre c = -R^T t (world-frame means, campos = w2c^-1[3, :3])
template <int SHDIR>
__device__ __forceinline__ void sh_dir_vec(const PoseDev& ps, const float x[3], const float p[3], float v[3]) {
  static_assert(SHDIR >= 0 && SHDIR <= 2, "sh_dir is 0, 1 or 2");
#pragma unroll
  for (int j = 0; j < 3; j++) {
    if constexpr (SHDIR == 0) v[j] = p[j];
    else if constexpr (SHDIR == 1) v[j] = x[j];
    else v[j] = x[j] + ps.R[0][j] * ps.t[0] + ps.R[1][j] * ps.t[1] + ps.R[2][j] * ps.t[2];
  }
}

// SH (ABI 209): an active degree above 0 -- colour = sum_k basis_k(dir) sh_k + 0.5, clamped at 0, with dir = v / |v| of sh_dir_vec<SHDIR> (ABI 211:
// SHDIR 1 and 2; SHDIR 0 is the instance of ABI 209); rest = this Gaussian's f_rest rows
template <bool SH = false, int SHDIR = 0>
__device__ __forceinline__ Projected slam_project_vals(const CamDev& cam, bool live, int idx, const float* __restrict__ pose, const float* PV, bool isotropic,
                                                       const RawGaussian& rg, int32_t* __restrict__ radii, const GeomView& g, bool world = false,
                                                       bool want_poserec = false, const float* __restrict__ rest = nullptr, int sh_deg = 0) {
  const float Vi[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  const PoseDev ps = load_pose(pose);
  float p[3] = {0.f, 0.f, 0.f};
  const float* q_raw = rg.q; const float* ls_raw = rg.ls; const float* fd_raw = rg.fd;
  const float op_raw = rg.op;
  if (live) {
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = ps.R[i][0] * rg.x[0] + ps.R[i][1] * rg.x[1] + ps.R[i][2] * rg.x[2] + ps.t[i];
  }
  Projected o;
  o.r0 = 0; o.r1 = 0; o.rad = 0; o.z = 0.f; o.cl = 0;
  o.sA = make_float4(0.f, 0.f, 0.f, 0.f); o.sB = o.sA;
  o.br.bx0 = 0; o.br.by0 = 0; o.br.bw = 0; o.br.bh = 0;
  if (live && p[2] > 0.2f) {
    const HomPoint h = hom_project(PV, p);
    float S3[3][3], R[3][3], sm[3], qn[4], qinv;
    slam_cov3d_vals(q_raw, ls_raw, isotropic, cam.scale_modifier, S3, R, sm, qn, qinv);
    Ewa e;
    if (world) {
      float V[16];
      pose_view_matrix(ps, V);
      ewa_project(cam, V, rg.x, S3, e);
    } else {
      ewa_project(cam, Vi, p, S3, e);
    }
    float det = e.a * e.c - e.b * e.b;
    float px = ((h.hx * h.pw + 1.f) * cam.W - 1.f) * 0.5f;
    float py = ((h.hy * h.pw + 1.f) * cam.H - 1.f) * 0.5f;
    if (det != 0.f && isfinite(px) && isfinite(py)) {
      float dinv = 1.f / det;
      const TileRect tr = splat_tile_rect(cam, px, py, e.a, e.c, det);
      if (tr.hit) {
        o.rad = tr.rad; o.r0 = tr.r0; o.r1 = tr.r1;
        const float* fd = fd_raw;
        float c0 = SH_C0F * fd[0] + 0.5f, c1 = SH_C0F * fd[1] + 0.5f, c2 = SH_C0F * fd[2] + 0.5f;
        if constexpr (SH) {
          float v[3];
          sh_dir_vec<SHDIR>(ps, rg.x, p, v);
          const float inv = 1.f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
          float bb[16];
          sh_basis(sh_deg, v[0] * inv, v[1] * inv, v[2] * inv, bb);
          const int nb = (sh_deg + 1) * (sh_deg + 1);
          c0 = bb[0] * fd[0]; c1 = bb[0] * fd[1]; c2 = bb[0] * fd[2];
#pragma unroll
          for (int k = 1; k < 16; k++)
            if (k < nb) { c0 += bb[k] * rest[(k - 1) * 3]; c1 += bb[k] * rest[(k - 1) * 3 + 1]; c2 += bb[k] * rest[(k - 1) * 3 + 2]; }
          c0 += 0.5f; c1 += 0.5f; c2 += 0.5f;
        }
        o.cl = (c0 < 0.f ? 1u : 0u) | (c1 < 0.f ? 2u : 0u) | (c2 < 0.f ? 4u : 0u);
        g.clamped[idx] = (uint8_t)o.cl;
        // (the depth the tiles are SORTED by is the view depth p[2] in both modes; zc is the value the depth bundle composites)
        const float z = p[2];
        const float zc = world ? ps.R[0][2] * rg.x[0] + ps.R[1][2] * rg.x[1] + ps.R[2][2] * rg.x[2] : p[2];
        const float op = 1.f / (1.f + expf(-op_raw));
        float4* sp = (float4*)(g.splat + (size_t)idx * SPLAT_F);
        o.sA = make_float4(px, py, e.c * dinv, -e.b * dinv); o.sB = make_float4(e.a * dinv, op, fmaxf(c0, 0.f), fmaxf(c1, 0.f));
        sp[0] = o.sA;
        sp[1] = o.sB;
        o.br = block_rect(o.sA, o.sB, o.r0, o.r1);
        sp[2] = make_float4(fmaxf(c2, 0.f), zc, 1.f, zc * zc);
        g.depth[idx] = z;
        o.z = z;
        if (want_poserec && !world)
          pose_chain_record(cam, PV, p, rg.x, e, S3, e.c * dinv, -e.b * dinv, e.a * dinv, h.pw, h.hx, h.hy, g.poserec + (size_t)idx * POSEREC_F);
      }
    }
  }
  if (live) {
    radii[idx] = o.rad;
    g.rect[(size_t)idx * 2] = o.r0;
    g.rect[(size_t)idx * 2 + 1] = o.r1;
  }
  return o;
}

template <bool SH = false, int SHDIR = 0>
__device__ __forceinline__ Projected slam_project_one(const CamDev& cam, int P, int idx, const SlamIn& in, int32_t* __restrict__ radii,
                                                      const GeomView& g, bool want_poserec = false) {
  const bool live = idx < P;
  // every parameter of this Gaussian is requested up front (one memory latency for the kernel, not two: the map is
  // almost entirely in view in a SLAM iteration, so nothing is wasted on culled splats)
  RawGaussian rg = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.f};
  if (live) {
#pragma unroll
    for (int k = 0; k < 3; k++) rg.x[k] = in.xyz[(size_t)idx * 3 + k];
#pragma unroll
    for (int k = 0; k < 4; k++) rg.q[k] = in.rotation[(size_t)idx * 4 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) { rg.ls[k] = in.scaling[(size_t)idx * 3 + k]; rg.fd[k] = in.f_dc[(size_t)idx * 3 + k]; }
    rg.op = in.opacity[idx];
  }
  // (the pose and cam.proj are read from memory where they are used here: hoisting them to the kernel's entry, as slam_bwd_project_kernel does,
  //  gained slam_project_bin_kernel 0.1 .. 0.15 us of 20 -- inside its run-to-run spread, profiles/r11_ab_per_gaussian_loads.txt)
  return slam_project_vals<SH, SHDIR>(cam, live, idx, in.pose, cam.proj, in.isotropic != 0, rg, radii, g, in.world != 0, want_poserec,
                               SH ? in.f_rest + (size_t)(live ? idx : 0) * (size_t)in.n_rest * 3 : nullptr, in.sh_deg);
}

template <bool SH, int SHDIR = 0>
__global__ void __launch_bounds__(FB)
slam_preprocess_fwd_kernel(CamDev cam, int P, SlamIn in, int32_t* __restrict__ radii, GeomView g, ImageView iv, int lds_tiles,
                           int vis_only, uint32_t* __restrict__ seen, int want_poserec) {
  extern __shared__ uint32_t hist[];
  const int T = cam.gx * cam.gy;
  for (int t = threadIdx.x; t < lds_tiles; t += FB) hist[t] = 0;
  if (lds_tiles) __syncthreads();
  const int idx = blockIdx.x * FB + threadIdx.x;
  const bool live = idx < P;
  const Projected pr = slam_project_one<SH, SHDIR>(cam, P, idx, in, radii, g, want_poserec != 0);
  const uint32_t r0 = pr.r0, r1 = pr.r1;
  const int32_t rad = pr.rad;
  if (vis_only) {      // mm3dgs_slam_visibility: the projection stage alone (workgroup-uniform): no tile counting, no scans
    if (live && seen && rad > 0) seen[idx] += 1u;
    return;
  }
  count_rect_tiles<FB>(cam.gx, T, lds_tiles, hist, live, idx, r0, r1, g, iv);
}

// runtime (sh_deg, sh_dir) -> instantiation of a projection kernel family K<SH, SHDIR>
#define SLAM_PICK_SH(K, in) ((in).sh_deg <= 0 ? K<false, 0> : (in).sh_dir == 2 ? K<true, 2> : (in).sh_dir == 1 ? K<true, 1> : K<true, 0>)

void launch_slam_preprocess_fwd(const CamDev& cam, int P, const SlamIn& in, int32_t* radii, GeomView g, ImageView iv, hipStream_t s,
                                uint32_t* seen, bool visibility_only, bool want_poserec) {
  if (P <= 0) return;
  const int T = cam.gx * cam.gy;
  const int lds_tiles = (T <= MAX_LDS_TILES && !visibility_only) ? T : 0;
  // (the pose-chain records exist at SH degree 0 only)
  hipLaunchKernelGGL(SLAM_PICK_SH(slam_preprocess_fwd_kernel, in), dim3((P + FB - 1) / FB), dim3(FB), (size_t)lds_tiles * 4, s, cam, P, in, radii, g, iv,
                     lds_tiles, visibility_only ? 1 : 0, seen, want_poserec && in.sh_deg <= 0 ? 1 : 0);
}

// ---- projection + binning in ONE launch (direct bins) -----------------------------------------------------------------------------
// Every tile owns a fixed span of `cap` pairs at tile * cap (the host sized the binning state as T x cap from the longest
// list it has seen), so a pair's slot does not depend on a global prefix: no tile-count pass, no scan, no second kernel.  One
// lane per Gaussian, two sweeps over its tile rectangle around a per-workgroup LDS histogram: sweep 1 counts the workgroup's
// pairs per tile, one returning global atomic per *touched tile* reserves slots in the tile's span, sweep 2 hands them out
// with LDS atomics and writes, per pair, the key (depth bits | id | slot) and the payload the sort needs to emit the block
// lists without touching the splat again: the 16-bit block mask (tile_mask.h) and the pair's per-tile gradient record.  The
// per-tile records (one per pair, BwdView.dtile) need no global prefix either: projection workgroup w owns records
// [w * trec_cap, (w + 1) * trec_cap) with trec_cap = N_capacity / ceil(P / 256) (CamDev.trec_cap), a Gaussian's pairs
// contiguous inside the span at g.tileoff[idx].  The block records are addressed by list position (composite.hip) and have
// no span of their own.  A tile with more than `cap` pairs drops the excess and the sort flags the overflow; a workgroup
// with more than trec_cap pairs flags it here, and its splats that do not fit get no per-tile record (~0u).  Both set the
// sticky Mm3dgsHeader.overflow, like a packed bin that runs out of capacity.
struct PairCtx {           // what a lane needs to emit the pairs of ITS Gaussian (broadcast lane by lane for huge splats)
  MaskConsts mc; BlkRect br; uint32_t khi, idbits; int minx, miny, w, area;
  uint32_t trec0;            // per-tile record of the splat's first pair (absolute; pair k of the tile rectangle, row-major: trec0 + k); ~0u: none
};
__device__ __forceinline__ uint32_t emit_pair(const PairCtx& c, int k, int ttx, int tty, uint32_t* hist, int gx, uint32_t cap, const BinView& b,
                                              bool have_mask = false, uint32_t mask_in = 0u) {
  const int t = tty * gx + ttx;
  const uint32_t slot = atomicAdd(&hist[t], 1u);
  uint32_t mask = 0;
  if (slot < cap) {
    mask = have_mask ? mask_in : tile_block_mask_in_rect(c.mc, ttx, tty, c.br);
    const size_t at = (size_t)t * cap + slot;
    b.keys[at] = ((unsigned long long)c.khi << 32) | (unsigned long long)(c.idbits | slot);
    // payload (round 6): block mask | the pair's per-tile gradient record << 32 -- the block records themselves are addressed by list position
    // (composite.hip), so neither the block rectangle's width nor a first block record travels any more
    b.payload[at] = (unsigned long long)mask | ((unsigned long long)(c.trec0 == 0xffffffffu ? 0xffffffffu : c.trec0 + (uint32_t)k) << 32);
  }
  return mask;
}

// The binning half of the projection kernels: every lane hands in the projection of ITS Gaussian (slam_project_one / _vals); hist = the
// workgroup's [T] words of LDS, cleared by the caller before (the first barrier inside orders the clear).
__device__ __forceinline__ void slam_bin_pairs(const CamDev& cam, int P, int idx, const Projected& pr, const GeomView& g, const ImageView& iv,
                                               const BinView& b, uint32_t cap, int slot_bits, uint32_t* hist) {
  const int T = cam.gx * cam.gy;
  const int tid = threadIdx.x, lane = tid & 63, wvi = tid >> 6;
  const bool live = idx < P;
  PairCtx c;
  c.mc = mask_consts(pr.sA, pr.sB);
  c.br = pr.br;
  c.minx = pr.r0 & 0xffff; c.miny = pr.r0 >> 16;
  c.w = (int)(pr.r1 & 0xffff) - c.minx;
  c.area = c.w * ((int)(pr.r1 >> 16) - c.miny);
  c.khi = __float_as_uint(pr.z);
  c.idbits = (uint32_t)idx << slot_bits;
  {   // workgroup-local exclusive scan of the workgroup's pairs (round 6: the block records are addressed by list position, composite.hip -- the scan
      // of the splats' 4x4 blocks, the per-workgroup record spans and their overflow case are gone)
    __shared__ uint32_t wtot2[FB / 64];
    const uint32_t x2 = wave_scan_incl((uint32_t)c.area);
    if (lane == 63) wtot2[wvi] = x2;
    __syncthreads();                      // (also orders the histogram clear before sweep 1)
    uint32_t pre2 = 0;
    for (int q = 0; q < wvi; q++) pre2 += wtot2[q];
    // per-tile records: this workgroup's pairs own [w * trec_cap, (w + 1) * trec_cap); a Gaussian's pairs are contiguous in it
    const uint32_t plocal = pre2 + x2 - (uint32_t)c.area;
    if (live) g.tileoff[idx] = plocal;
    c.trec0 = plocal + (uint32_t)c.area <= cam.trec_cap ? (uint32_t)blockIdx.x * cam.trec_cap + plocal : 0xffffffffu;
    if (tid == FB - 1) {
      g.block_tiles[blockIdx.x] = pre2 + x2;  // pairs of this workgroup (summed into num_rendered by the sort)
      if (pre2 + x2 > cam.trec_cap) iv.hdr->overflow = 1u;
    }
  }
  // sweep 1: count (a rectangle of more than 32 tiles is spread over the wave).  Round 4: the block masks of a lane's OWN pairs (the first
  // four of its splat: all the pairs of nearly every splat of a SLAM map) are evaluated here already, and a pair whose mask is EMPTY -- the
  // 3-sigma tile rectangle the reference prescribes for `radii` / tiles touched reaches further than the { alpha >= 1/255 } region that can
  // contribute: 15 % of the pairs at frame 8 of the benchmark run, 18 % after 100 frames -- takes no slot in its tile's bin: no key to sort,
  // no payload, no per-tile gradient record.  Bit k of `empty4` marks it; the backward projection finds the bits in clamped[idx] >> 4 and
  // skips the record (it would be all zeros).  Splats of more than 32 tiles and the pairs beyond the fourth are listed as before.
  constexpr int OWN = 4;
  unsigned long long big = __ballot(c.area > 32);
  unsigned long long m64 = 0ull;
  uint32_t empty4 = 0u;
  const bool droppable = c.area > 0 && c.area <= 32;
  if (droppable) {
    int ttx = c.minx, tty = c.miny;
    const int kmax = PROBE(cam, 7) ? min(c.area, OWN) : c.area;      // (probe builds, bit 7: only the own pairs counted)
    for (int k = 0; k < kmax; k++) {
      bool count = true;
      if (k < OWN) {
        const uint32_t mk = tile_block_mask_in_rect(c.mc, ttx, tty, c.br);
        m64 |= (unsigned long long)mk << (16 * k);
        count = mk != 0u;
        empty4 |= count ? 0u : (1u << k);
      }
      if (count) atomicAdd(&hist[tty * cam.gx + ttx], 1u);
      if (++ttx == c.minx + c.w) { ttx = c.minx; tty++; }
    }
  }
  if (live) g.clamped[idx] = (uint8_t)(pr.cl | (empty4 << 4));
  if (PROBE(cam, 8)) big = 0ull;      // (probe builds, bit 8: without the > 32-tile splats' counting)
  for (unsigned long long bb = big; bb; bb &= bb - 1) {
    const int src = __ffsll((long long)bb) - 1;
    const int sminx = __builtin_amdgcn_readlane(c.minx, src), sminy = __builtin_amdgcn_readlane(c.miny, src);
    const int sw = __builtin_amdgcn_readlane(c.w, src), sarea = __builtin_amdgcn_readlane(c.area, src);
    for (int k = lane; k < sarea; k += 64) atomicAdd(&hist[(sminy + k / sw) * cam.gx + sminx + k % sw], 1u);
  }
  __syncthreads();
  for (int t = tid; t < T; t += FB) {
    const uint32_t n = hist[t];
    if (n) hist[t] = atomicAdd(&iv.cursor[t], n);
  }
  __syncthreads();
  // sweep 2: slots, keys, payloads (~200 instructions per pair).  Every lane emits the first four pairs of its own splat --
  // all the pairs of nearly every splat of a SLAM map (their block masks were formed above, m64: pair k = bits 16k..16k+15).  The pairs beyond the fourth form the wave's flat work list, cut into equal shares: the few 20-90 pixel
  // splats that grow in a map would otherwise keep one lane busy for dozens of iterations while its wave waits (this kernel
  // went from 19 to 44 us over 100 frames of a run before).
  {   // (running tile coordinates: no division per pair)
    int ttx = c.minx, tty = c.miny;
    for (int k = 0; k < min(c.area, OWN); k++) {
      if (!((empty4 >> k) & 1u)) emit_pair(c, k, ttx, tty, hist, cam.gx, cap, b, droppable, (uint32_t)(m64 >> (16 * k)) & 0xffffu);
      if (++ttx == c.minx + c.w) { ttx = c.minx; tty++; }
    }
  }
  const uint32_t incl = wave_scan_incl((uint32_t)max(c.area - OWN, 0));
  const uint32_t S = PROBE(cam, 6) ? 0u : (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);     // (probe builds, bit 6: without the shared list)
  if (S) {   // wave-uniform
    // (a raised issue priority for these waves -- the launch's tail on a grown map -- changes nothing: 36.0 / 19.0 us either way on the hand-held sweep,
    //  round 5; the per-Gaussian kernels run 2.4 waves per SIMD and wait on memory, not on issue slots)
    __shared__ uint32_t s_pref[FB / 64][64];
    __shared__ PairCtx s_ctx[FB / 64][64];
    s_pref[wvi][lane] = incl;
    s_ctx[wvi][lane] = c;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = (uint32_t)lane; i < S; i += 64u) {
      int lo = 0, hi = 63;     // owner: smallest o with pref[o] > i
#pragma unroll
      for (int st = 0; st < 6; st++) {
        const int mid = (lo + hi) >> 1;
        if (s_pref[wvi][mid] > i) hi = mid; else lo = mid + 1;
      }
      const int o = min(lo, 63);
      const uint32_t excl = o ? s_pref[wvi][o - 1] : 0u;
      const PairCtx oc = s_ctx[wvi][o];
      const int k = OWN + (int)(i - excl);
      emit_pair(oc, k, oc.minx + k % oc.w, oc.miny + k / oc.w, hist, cam.gx, cap, b);
    }
  }
}

// prologue of the projection + binning kernels: clear the workgroup's tile histogram, publish the bin capacity, return the lane's Gaussian
__device__ __forceinline__ int slam_bin_prologue(const CamDev& cam, const ImageView& iv, uint32_t cap, uint32_t* hist) {
  const int T = cam.gx * cam.gy;
  const int tid = threadIdx.x;
  for (int t = tid; t < T; t += FB) hist[t] = 0;
  if (blockIdx.x == 0 && tid == 0) iv.hdr->bin_cap = cap;
  return blockIdx.x * FB + tid;
}

template <bool SH, int SHDIR = 0>
__global__ void __launch_bounds__(FB)
slam_project_bin_kernel(CamDev cam, int P, SlamIn in, int32_t* __restrict__ radii, GeomView g, ImageView iv, BinView b, uint32_t cap,
                        int slot_bits, int want_poserec) {
  extern __shared__ uint32_t hist[];     // [T]: pairs of this workgroup per tile, then the next slot of each touched tile
  const int idx = slam_bin_prologue(cam, iv, cap, hist);
  const Projected pr = slam_project_one<SH, SHDIR>(cam, P, idx, in, radii, g, want_poserec != 0);
  slam_bin_pairs(cam, P, idx, pr, g, iv, b, cap, slot_bits, hist);
}

void launch_slam_project_bin(const CamDev& cam, int P, const SlamIn& in, int32_t* radii, GeomView g, ImageView iv, BinView b, uint32_t bin_cap,
                             int slot_bits, hipStream_t s, bool want_poserec) {
  if (P <= 0) return;
  const int T = cam.gx * cam.gy;
  hipLaunchKernelGGL(SLAM_PICK_SH(slam_project_bin_kernel, in), dim3((P + FB - 1) / FB), dim3(FB), (size_t)T * 4, s, cam, P, in, radii, g, iv, b, bin_cap,
                     slot_bits, want_poserec && in.sh_deg <= 0 ? 1 : 0);
}

// One Gaussian's row of N (1, 3 or 4) floats of an Adam group, stepped: ONE store per array -- parameters, first and second moments -- of the
// row's width (dword / dwordx3 / dwordx4; rows are 4-byte aligned, which is all a global store needs).  A [P, 3] array's last row ends
// the allocation: its store is 12 bytes, never 16.  Element by element with the three arrays interleaved -- the arrays may alias as far as
// the compiler knows -- the 14 parameters left as 42 single-dword stores, each strided by 12 or 16 bytes across the wave.
// (n: a constant of the unrolled loop over the groups)
__device__ __forceinline__ void store_row(float* dst, const float* v, int n) {
  if (n == 4) { const f4u w = {v[0], v[1], v[2], v[3]}; *(f4u*)dst = w; }
  else if (n == 3) { const float w[3] = {v[0], v[1], v[2]}; __builtin_memcpy(dst, w, 12); }
  else dst[0] = v[0];
}
__device__ __forceinline__ void store_adam_rows(int n, float* p, float* m, float* v, int idx, const float* rp, const float* rm, const float* rv) {
  const size_t off = (size_t)idx * n;
  store_row(p + off, rp, n); store_row(m + off, rm, n); store_row(v + off, rv, n);
}

// ---------------------------------------------------------------------------------------------------------------------
#define NPOSE 12  // dR (9, row-major) | dt (3)
// stepped: (the map's in-kernel Adam, ma.on) the lane's parameters AFTER the step -- what the next iteration's projection reads
// SH (ABI 209, active degree > 0; mapping-layout records -- the colour sums -- also when only the pose gradient is wanted): d/d(f_rest), the
// direction's share of d/d(mean), the sixth Adam group.  SHDIR (ABI 211) = the direction's source, sh_dir_vec: 0 -- its share goes into dm (the
// camera-space mean: the means and the pose); 1 and 2 -- straight into d/d(xyz), and for 2 (world-frame means only) the camera centre's terms into
// the pose rows: v = x + R^T t, so dL/dR_ij += t_i g_j and dL/dt += R g (g = dL/dv)
// FUSED: the instance of slam_bwd_project_kernel -- api.hip launches it only with the in-kernel Adam on and without gradient output, and as
// constants the two leave the first round of loads one straight path (a wait behind a join of paths is sized for the path with the fewest loads)
template <bool TRACK, bool DIRECT, bool WORLD = false, bool SH = false, int SHDIR = 0, bool FUSED = false>
__device__ __forceinline__ void slam_bwd_body(const CamDev& cam, int P, const SlamIn& in, const PoseProj& u, const int32_t* __restrict__ radii, const GeomView& g,
                                              uint32_t N_cap, const float* __restrict__ dsub, float* __restrict__ posepartial, const SlamGrads& out,
                                              const MapAdam& ma, RawGaussian* stepped, const uint32_t* __restrict__ ovf) {
  const int idx = blockIdx.x * SLAM_BWD_FB + threadIdx.x;
  // A forward that ran out of capacity (sticky header word, set by this iteration's binning / sort or by any earlier one of the loop)
  // dropped pairs WITHOUT writing their per-tile records: the sums below would read stale scratch.  Such an iteration is void -- no
  // gradient, no statistics, no optimiser step (zero gradients would still move the parameters by their momentum) -- so a loop whose
  // header is only read at a later drained point (fused.py: lazy checks) leaves the map exactly as the last complete iteration left it.
  // (requested here, consumed only after the gather below: nothing waits for it)
  const uint32_t ovf_word = ovf != nullptr ? __builtin_nontemporal_load(ovf) : 0u;
  const float* PV = u.PV;
  const float Vi[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  const PoseDev ps = load_pose(u.pose);
  // (kernel arguments the late phases used to fetch -- and wait for -- where they are used: read here, with the rest)
  const uint8_t* const opt_mask = ma.opt_mask;
  const bool adam_on = FUSED || ma.on != 0;
  const bool grads_out = !FUSED && out.d_xyz != nullptr;
  float* const st_radii = out.max_radii2D; float* const st_grad = out.grad_accum; float* const st_denom = out.denom;
  float cg[NPOSE];
#pragma unroll
  for (int k = 0; k < NPOSE; k++) cg[k] = 0.f;
  float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0, acc2 = acc0;
  int rad = 0;
  uint32_t cl_bits = 0;     // clamped[idx]: SH clamp bits 0-2 | (direct bins) empty-pair bits 4-7
  float4 sA = make_float4(0.f, 0.f, 0.f, 0.f), sB = sA;   // first 32 bytes of this Gaussian's splat record (xy, conic, opacity)
  float px3[3] = {0.f, 0.f, 0.f}, q_raw[4] = {1.f, 0.f, 0.f, 0.f}, ls_raw[3] = {0.f, 0.f, 0.f}, op_raw = 0.f;
  // Adam state of this Gaussian's 14 parameters, its three densification statistics and its opt_mask byte: they depend on idx and on
  // kernel arguments only, so they belong to the FIRST round of loads (below) and are held in registers across the gather -- ~45 VGPRs,
  // DESIGN.md section 4.  Requested behind the gather, as they were, the state was a round trip of its own (9 of its 15 loads had to land
  // before the chain rule started), each statistic a load - wait - store of its own, the mask byte one more.
  constexpr int AG_OFF[5] = {0, 3, 6, 7, 10}, AG_N[5] = {3, 3, 1, 3, 4};
  float ap[14], am[14], av[14];
  float st_r, st_g, st_d;      // (like the state: set and read under the same uniform conditions, no value on the other path to merge with)
  uint32_t maskb;
  {
    uint32_t first = 0;
    int area = 0;
    // one round of independent loads for everything this lane reads but the gradient records (this kernel is a chain of memory
    // latencies: every dependent step costs ~2 us).  A culled Gaussian has rect = 0 (and an unwritten splat record, read but never used).
    // The lanes past the map's end (the last workgroup's) read Gaussian P - 1 and use nothing of it (their rectangle is emptied below): loads
    // under a divergent branch come out of it through a merge of registers, whose copies of the wide loads' results were waits for the
    // state in front of the gather.
    uint32_t r0 = 0, r1 = 0, toff = 0, btile = 0, clb = 0;
    {
      const int li = idx < P ? idx : P - 1;
      // (what the gather's addresses are formed from comes first: the loads return in order, so the gather starts when these four have
      //  landed and everything requested behind them lands while the records are summed)
      clb = g.clamped[li];
      r0 = g.rect[(size_t)li * 2]; r1 = g.rect[(size_t)li * 2 + 1];
      toff = g.tileoff[li];
      if (!DIRECT) btile = g.block_tiles[li >> 8];
      __builtin_amdgcn_sched_barrier(0);      // (the scheduler orders independent loads by register pressure: without this, tileoff is the 13th)
      rad = radii[li];
      // the Gaussian's own parameters depend on nothing but li: requested with the first round, they land while the records are
      // gathered (the chain rule below used to start with a memory round trip of its own)
#pragma unroll
      for (int k = 0; k < 3; k++) { px3[k] = in.xyz[(size_t)li * 3 + k]; ls_raw[k] = in.scaling[(size_t)li * 3 + k]; }
#pragma unroll
      for (int k = 0; k < 4; k++) q_raw[k] = in.rotation[(size_t)li * 4 + k];
      op_raw = in.opacity[li];
      const float4* spl = (const float4*)(g.splat + (size_t)li * SPLAT_F);
      sA = spl[0]; sB = spl[1];
      if (adam_on) {
#pragma unroll
        for (int gq = 0; gq < 5; gq++)
#pragma unroll
          for (int c = 0; c < AG_N[gq]; c++) {
            const size_t off = (size_t)li * AG_N[gq] + c;
            ap[AG_OFF[gq] + c] = ma.p[gq][off]; am[AG_OFF[gq] + c] = ma.m[gq][off]; av[AG_OFF[gq] + c] = ma.v[gq][off];
          }
        if (opt_mask) maskb = opt_mask[li];
      }
      if (st_radii) { st_r = st_radii[li]; st_g = st_grad[li]; st_d = st_denom[li]; }
    }
    if (idx >= P) { r0 = 0; r1 = 0; }
    if (r1 != r0) {   // <=> radii > 0
      area = ((int)(r1 & 0xffff) - (int)(r0 & 0xffff)) * ((int)(r1 >> 16) - (int)(r0 >> 16));
      // first per-tile record of this Gaussian's pairs (contiguous, row-major over its tile rectangle): direct bins -- inside its
      // projection workgroup's span; packed bins -- its Gaussian-major pair index
      first = DIRECT ? (uint32_t)(idx >> 8) * cam.trec_cap + toff : btile + toff;
      const bool fits = DIRECT ? (toff + (uint32_t)area <= cam.trec_cap) : true;
      if (!fits || (size_t)first + (size_t)area > (size_t)N_cap) area = 0;      // beyond the capacity (flagged by the forward): nothing was written
    }
    constexpr int RECF = TRACK ? REC_TRACK_F : REC_MAP_F;      // (composite_common.h; the records are packed: stride = size)
    gather_records<RECF>(area, first, dsub + (size_t)NLIST * (size_t)N_cap * SPLAT_F, RECF, acc0, acc1, acc2, DIRECT ? (clb >> 4) : 0u);
    cl_bits = clb;
  }
  const bool skip = ovf_word != 0u;
  if (skip) rad = 0;        // void iteration: whatever the gather read (stale records of dropped pairs) is never used
  if (idx < P) {
    float dxyz[3] = {0.f, 0.f, 0.f}, dfd[3] = {0.f, 0.f, 0.f}, dls[3] = {0.f, 0.f, 0.f}, dqr[4] = {0.f, 0.f, 0.f, 0.f};
    float dlogit = 0.f, gnorm = 0.f;
    float shb[16], shg[3] = {0.f, 0.f, 0.f};      // (SH) basis values at this Gaussian's direction, clamp-masked colour gradient: zero for an invisible Gaussian
    float shw[3] = {0.f, 0.f, 0.f};               // (SH, SHDIR 1 / 2) dL/dv of the world-frame direction vector: the direction's share of d/d(xyz)
    if constexpr (SH) {
#pragma unroll
      for (int k = 0; k < 16; k++) shb[k] = 0.f;
    }
    if (rad > 0) {
      // moments -> d/dxy (pixel units) and d/dconic, with this splat's conic (composite.hip record layout)
      const float4 sp0 = sA, sp1 = sB;
      const float qa = sp0.z, qb = sp0.w, qc = sp1.x;
      // record layouts of composite.hip's SepReduce:  mapping [M0 Mx Mxx c0 | c1 c2 cz My | Mxy Myy],  tracking [M0 Mx Mxx cz | My Mxy Myy]
      const float M0 = acc0.x, m_x = acc0.y, m_xx = acc0.z;
      const float m_y = TRACK ? acc1.x : acc1.w, m_xy = TRACK ? acc1.y : acc2.x, m_yy = TRACK ? acc1.z : acc2.y;
      const float dc0 = acc0.w, dc1 = acc1.x, dc2 = acc1.y;        // mapping only
      const float dz_tot = TRACK ? acc0.w : acc1.z;               // d/dz of the [z, 1, z^2] bundle, already chained by the compositor
      const float gpx = -(qa * m_x + qb * m_y), gpy = -(qc * m_y + qb * m_x);
      const float gA = -0.5f * m_xx, gB = -m_xy, gC = -0.5f * m_yy;
      const float x0 = px3[0], x1 = px3[1], x2 = px3[2];
      float p[3];
#pragma unroll
      for (int i = 0; i < 3; i++) p[i] = ps.R[i][0] * x0 + ps.R[i][1] * x1 + ps.R[i][2] * x2 + ps.t[i];
      float S3[3][3], R[3][3], sm[3], qn[4], qinv;
      slam_cov3d_vals(q_raw, ls_raw, in.isotropic != 0, cam.scale_modifier, S3, R, sm, qn, qinv);
      Ewa e;
      constexpr bool world = WORLD;       // (a template parameter: the shipped configurations' instantiations keep their registers)
      if (world) {
        float V[16];
        pose_view_matrix(ps, V);
        const float xw[3] = {x0, x1, x2};
        ewa_project(cam, V, xw, S3, e);
      } else {
        ewa_project(cam, Vi, p, S3, e);
      }
      float GA[2][3], dS[3][3], dA[2][3];
      cov2d_grad_to_dA(e, S3, conic_grad_to_cov2d(e.a, e.b, e.c, gA, gB, gC), GA, dA);
      cov2d_grad_to_dcov3d(e.A, GA, dS);
      // transform mode: view = identity, dJ[r][k] = dA[r][k].  World mode: A = J R  ->  dJ = dA R^T, and the pose's rotation receives
      // dR[k][i] += sum_r J[r][k] dA[r][i]  (J = [[J00, 0, J02], [0, J11, J12]]) -- the "-w-pose" gradient through the view matrix
      float dJ00 = dA[0][0], dJ02 = dA[0][2], dJ11 = dA[1][1], dJ12 = dA[1][2];
      float dRc[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
      if (world) {
        dJ00 = dA[0][0] * ps.R[0][0] + dA[0][1] * ps.R[0][1] + dA[0][2] * ps.R[0][2];
        dJ02 = dA[0][0] * ps.R[2][0] + dA[0][1] * ps.R[2][1] + dA[0][2] * ps.R[2][2];
        dJ11 = dA[1][0] * ps.R[1][0] + dA[1][1] * ps.R[1][1] + dA[1][2] * ps.R[1][2];
        dJ12 = dA[1][0] * ps.R[2][0] + dA[1][1] * ps.R[2][1] + dA[1][2] * ps.R[2][2];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          dRc[0][i] = e.J00 * dA[0][i];
          dRc[1][i] = e.J11 * dA[1][i];
          dRc[2][i] = e.J02 * dA[0][i] + e.J12 * dA[1][i];
        }
      }
      float dm[3];
      dJ_to_dmean(cam, e, dJ00, dJ02, dJ11, dJ12, dm);
      const ScreenGrad sg = pixel_grad_to_dmean(cam, PV, hom_project(PV, p), gpx, gpy, dm);
      gnorm = sqrtf(sg.gnx * sg.gnx + sg.gny * sg.gny);
      if (!world) dm[2] += dz_tot;          // transform mode: the depth bundle's z IS the camera-space z
      if constexpr (SH) {
        // colour = clamp(sum_k b_k(dir) sh_k + 0.5), dir = p / |p|: the basis values weight the coefficient gradients, the basis' direction
        // derivative runs through the normalisation into dm (and from there into the means and the pose)
        static_assert(!TRACK, "the SH path runs on mapping-layout records");
        static_assert(WORLD == (SHDIR == 2), "world-frame means take the direction from the camera centre, pre-transformed ones from the mean or the origin");
        float v[3];
        {
          const float xw[3] = {x0, x1, x2};
          sh_dir_vec<SHDIR>(ps, xw, p, v);
        }
        const float pinv = 1.f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const float ux = v[0] * pinv, uy = v[1] * pinv, uz = v[2] * pinv;
        sh_basis(in.sh_deg, ux, uy, uz, shb);
        float gbx[16], gby[16], gbz[16];
        sh_basis_grad(in.sh_deg, ux, uy, uz, gbx, gby, gbz);
        const int nb = (in.sh_deg + 1) * (in.sh_deg + 1);
        shg[0] = (cl_bits & 1) ? 0.f : dc0; shg[1] = (cl_bits & 2) ? 0.f : dc1; shg[2] = (cl_bits & 4) ? 0.f : dc2;
        const float* rest = in.f_rest + (size_t)idx * (size_t)in.n_rest * 3;
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;
#pragma unroll
        for (int k = 1; k < 16; k++)
          if (k < nb) {
            const float tk = rest[(k - 1) * 3] * shg[0] + rest[(k - 1) * 3 + 1] * shg[1] + rest[(k - 1) * 3 + 2] * shg[2];
            ddx += gbx[k] * tk; ddy += gby[k] * tk; ddz += gbz[k] * tk;
          }
        const float dot = ux * ddx + uy * ddy + uz * ddz;
        if constexpr (SHDIR == 0) {
          dm[0] += (ddx - ux * dot) * pinv; dm[1] += (ddy - uy * dot) * pinv; dm[2] += (ddz - uz * dot) * pinv;
        } else {
          shw[0] = (ddx - ux * dot) * pinv; shw[1] = (ddy - uy * dot) * pinv; shw[2] = (ddz - uz * dot) * pinv;
        }
      }
      // pose: means_cam = R x + t
      cg[0] = dm[0] * x0; cg[1] = dm[0] * x1; cg[2] = dm[0] * x2;
      cg[3] = dm[1] * x0; cg[4] = dm[1] * x1; cg[5] = dm[1] * x2;
      cg[6] = dm[2] * x0; cg[7] = dm[2] * x1; cg[8] = dm[2] * x2;
      cg[9] = dm[0]; cg[10] = dm[1]; cg[11] = dm[2];
      if (world) {
        // + the covariance's rotation, + the depth bundle's z' = R[0][2] x0 + R[1][2] x1 + R[2][2] x2
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
          for (int i = 0; i < 3; i++) cg[k * 3 + i] += dRc[k][i];
        cg[2] += dz_tot * x0; cg[5] += dz_tot * x1; cg[8] += dz_tot * x2;
      }
      if constexpr (SH && SHDIR == 2) {
        // the camera centre: v = x + R^T t  ->  dL/dR_ij += t_i shw_j,  dL/dt_i += (R shw)_i
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
          for (int j = 0; j < 3; j++) cg[i * 3 + j] += ps.t[i] * shw[j];
          cg[9 + i] += ps.R[i][0] * shw[0] + ps.R[i][1] * shw[1] + ps.R[i][2] * shw[2];
        }
      }
      if (grads_out || adam_on) {
#pragma unroll
        for (int j = 0; j < 3; j++) dxyz[j] = ps.R[0][j] * dm[0] + ps.R[1][j] * dm[1] + ps.R[2][j] * dm[2] + (world ? dz_tot * ps.R[j][2] : 0.f);
        if constexpr (SH && SHDIR != 0) {
#pragma unroll
          for (int j = 0; j < 3; j++) dxyz[j] += shw[j];
        }
        const uint32_t cl = cl_bits;
        dfd[0] = (cl & 1) ? 0.f : SH_C0F * dc0;      // (SH_C0 = the degree-0 basis value)
        dfd[1] = (cl & 2) ? 0.f : SH_C0F * dc1;
        dfd[2] = (cl & 4) ? 0.f : SH_C0F * dc2;
        const float o = 1.f / (1.f + expf(-op_raw));
        dlogit = M0 * (1.f - o);   // sum G dL/dalpha = M0 / o, times d sigmoid = o (1 - o)
        float dR[3][3], ds[3];
        dcov3d_to_scale_rot(dS, R, sm, cam.scale_modifier, ds, dR);
        // scales = exp(log-scales): d/dlog = ds * s (sm already carries scale_modifier, ds carries the other factor)
        const float inv_mod = 1.f / cam.scale_modifier;
        if (in.isotropic) {
          dls[0] = (ds[0] * sm[0] + ds[1] * sm[1] + ds[2] * sm[2]) * inv_mod;
        } else {
          dls[0] = ds[0] * sm[0] * inv_mod; dls[1] = ds[1] * sm[1] * inv_mod; dls[2] = ds[2] * sm[2] * inv_mod;
        }
        dR_to_dq_raw(qn, qinv, dR, dqr);
      }
      if (st_radii) {      // (the old values came with the first round; a Gaussian with rad == 0 keeps its three words untouched)
        // (opaque up to here: the compiler would otherwise do the first arithmetic on each right behind its load -- and wait for it there)
        asm volatile("" : "+v"(st_r), "+v"(st_g), "+v"(st_d));
        st_radii[idx] = fmaxf(st_r, (float)rad);
        st_grad[idx] = st_g + gnorm;
        st_denom[idx] = st_d + 1.f;
      }
    }
    if (grads_out) {
      out.d_xyz[(size_t)idx * 3] = dxyz[0]; out.d_xyz[(size_t)idx * 3 + 1] = dxyz[1]; out.d_xyz[(size_t)idx * 3 + 2] = dxyz[2];
      out.d_f_dc[(size_t)idx * 3] = dfd[0]; out.d_f_dc[(size_t)idx * 3 + 1] = dfd[1]; out.d_f_dc[(size_t)idx * 3 + 2] = dfd[2];
      out.d_opacity[idx] = dlogit;
      out.d_scaling[(size_t)idx * 3] = dls[0]; out.d_scaling[(size_t)idx * 3 + 1] = dls[1]; out.d_scaling[(size_t)idx * 3 + 2] = dls[2];
      out.d_rotation[(size_t)idx * 4] = dqr[0]; out.d_rotation[(size_t)idx * 4 + 1] = dqr[1];
      out.d_rotation[(size_t)idx * 4 + 2] = dqr[2]; out.d_rotation[(size_t)idx * 4 + 3] = dqr[3];
      if constexpr (SH) {
        if (out.d_f_rest) {
          float* o = out.d_f_rest + (size_t)idx * (size_t)in.n_rest * 3;
          const int nb = (in.sh_deg + 1) * (in.sh_deg + 1);
#pragma unroll
          for (int k = 1; k < 16; k++)
            if (k - 1 < in.n_rest) {
              const float bk = k < nb ? shb[k] : 0.f;
              o[(k - 1) * 3] = bk * shg[0]; o[(k - 1) * 3 + 1] = bk * shg[1]; o[(k - 1) * 3 + 2] = bk * shg[2];
            }
        }
      }
    }
    if (adam_on) {
      // the map's Adam step for this Gaussian (every Gaussian, visible or not: zero gradients still decay the moments)
      if (opt_mask) asm volatile("" : "+v"(maskb));      // (as the statistics: the compare stays here, not behind the byte's load)
      const float keepg = (opt_mask && maskb == 0u) ? 0.f : 1.f;     // bundle adjustment: masked-out Gaussians get a zero gradient
      const float gr14[14] = {keepg * dxyz[0], keepg * dxyz[1], keepg * dxyz[2], keepg * dfd[0], keepg * dfd[1], keepg * dfd[2], keepg * dlogit,
                              keepg * dls[0], keepg * dls[1], keepg * dls[2], keepg * dqr[0], keepg * dqr[1], keepg * dqr[2], keepg * dqr[3]};
      if (!skip) {
#pragma unroll
      for (int gq = 0; gq < 5; gq++) {
#pragma unroll
        for (int c = 0; c < AG_N[gq]; c++) {
          const int q = AG_OFF[gq] + c;
          const AdamElem r = adam_elem(ap[q], am[q], av[q], gr14[q], ma.omb1, ma.beta2, ma.omb2, ma.bc2s, ma.eps, ma.step_size[gq]);
          am[q] = r.m; av[q] = r.v; ap[q] = r.p;
        }
        store_adam_rows(AG_N[gq], ma.p[gq], ma.m[gq], ma.v[gq], idx, ap + AG_OFF[gq], am + AG_OFF[gq], av + AG_OFF[gq]);
      }
      if constexpr (SH) {
        if (ma.rp) {      // the sixth group: every f_rest row steps (zero gradient beyond the active degree / for an invisible Gaussian: the moments decay)
          const int nb = (in.sh_deg + 1) * (in.sh_deg + 1);
          const size_t base = (size_t)idx * (size_t)in.n_rest * 3;
#pragma unroll
          for (int k = 1; k < 16; k++)
            if (k - 1 < in.n_rest) {
              const float bk = k < nb ? keepg * shb[k] : 0.f;
#pragma unroll
              for (int ch = 0; ch < 3; ch++) {
                const size_t off = base + (size_t)(k - 1) * 3 + ch;
                const float gr = bk * shg[ch];
                const float m0 = ma.rm[off], v0 = ma.rv[off];
                AdamElem r;
                adam_moments(m0, v0, gr, ma.omb1, ma.beta2, ma.omb2, r);
                ma.rm[off] = r.m; ma.rv[off] = r.v;
                ma.rp[off] = adam_param(ma.rp[off], r, ma.bc2s, ma.eps, ma.rest_step_size);
              }
            }
        }
      }
      }
      if (stepped) {      // AG layout: xyz 0-2 | f_dc 3-5 | opacity 6 | scaling 7-9 | rotation 10-13
#pragma unroll
        for (int k = 0; k < 3; k++) { stepped->x[k] = ap[k]; stepped->fd[k] = ap[3 + k]; stepped->ls[k] = ap[7 + k]; }
        stepped->op = ap[6];
#pragma unroll
        for (int k = 0; k < 4; k++) stepped->q[k] = ap[10 + k];
      }
    }
  }
  if (posepartial) {   // mapping without pose optimisation never consumes the pose gradient
    __shared__ float red[SLAM_BWD_FB / 64][NPOSE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NPOSE; k++) {
      float v = wave_sum_to_lane63(cg[k]);
      if (lane == 63) red[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NPOSE) {
      const int k = threadIdx.x;
      float t = red[0][k];
#pragma unroll
      for (int w = 1; w < SLAM_BWD_FB / 64; w++) t += red[w][k];
      posepartial[(size_t)blockIdx.x * 32 + k] = t;
    }
  }
}

// A mapping iteration's backward projection + Adam step and the NEXT iteration's projection + binning in one launch (direct bins, in-kernel
// Adam, no per-view pose step): both are one lane per Gaussian over the same index space, the stepped parameters go from the optimiser
// to the projection in registers (no second read of the map), and one launch with its ramp disappears from every mapping iteration.
// The lane reads the geometry of iteration k (its own rect / pair offset / splat record) before the projection half overwrites it for
// iteration k + 1; the bins and cursors were released by iteration k's sort; the per-tile records it sums were written by iteration k's
// compositor and are not touched again before iteration k + 1's.
static_assert(SLAM_BWD_FB == FB, "the fused backward + projection kernel uses one lane per Gaussian in both halves");
template <bool WORLD>
__global__ void __launch_bounds__(FB)
slam_bwd_project_kernel(CamDev cam, int P, SlamIn in, int32_t* __restrict__ radii, GeomView g, ImageView iv, BinView b, uint32_t N_cap,
                        const float* __restrict__ dsub, SlamGrads out, MapAdam ma, const float* __restrict__ next_pose, uint32_t cap,
                        int slot_bits) {
  extern __shared__ uint32_t hist[];
  // both views' uniforms before the first store of the kernel: the projection half used to fetch next_pose behind the Adam stores
  const PoseProj u = load_pose_proj(in.pose, cam.proj), un = load_pose_proj(next_pose, cam.proj);
  const int idx = slam_bin_prologue(cam, iv, cap, hist);
  RawGaussian rg = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.f};
  // (the overflow word as the backward compositor of this iteration found it: the binning half below may set the live word while
  //  workgroups of this half are still starting, and a partially stepped map is worse than either outcome)
  slam_bwd_body<false, true, WORLD, false, 0, true>(cam, P, in, u, radii, g, N_cap, dsub, nullptr, out, ma, &rg, &iv.hdr->overflow_seen);
  const Projected pr = slam_project_vals(cam, idx < P, idx, un.pose, un.PV, in.isotropic != 0, rg, radii, g, WORLD);
  slam_bin_pairs(cam, P, idx, pr, g, iv, b, cap, slot_bits, hist);
}

void launch_slam_bwd_project(const CamDev& cam, int P, const SlamIn& in, int32_t* radii, GeomView g, ImageView iv, BinView b, size_t N_cap,
                             BwdView bw, const SlamGrads& out, const MapAdam& ma, const float* next_pose, uint32_t bin_cap,
                             int slot_bits, hipStream_t s) {
  if (P <= 0) return;
  const uint32_t ncap = (uint32_t)(N_cap > 0xffffffffull ? 0xffffffffull : N_cap);
  const int T = cam.gx * cam.gy;
  hipLaunchKernelGGL(in.world ? slam_bwd_project_kernel<true> : slam_bwd_project_kernel<false>, dim3((P + FB - 1) / FB), dim3(FB), (size_t)T * 4, s, cam, P, in,
                     radii, g, iv, b, ncap, bw.dsub, out, ma, next_pose, bin_cap, slot_bits);
}

// The multi-GPU window's optimiser step (slam/mapper.py:931-948 on all-reduced gradients) and the NEXT view's projection + binning in one launch: what
// fused_adam_kernel + slam_project_bin_kernel do in two, with the stepped parameters going from the optimiser to the projection in
// registers (the second half of slam_bwd_project_kernel, fed by gradient arrays instead of the record gather).  The update is adam_elem, as
// in slam_bwd_body's in-kernel Adam; opt_mask as there.
// SH (ABI 212): an active degree above 0 -- the sixth group (f_rest from gr.d_f_rest, every one of the n_rest rows stepped: zero gradient beyond
// the active degree, the moments decay) and the projection's SH colour from the STEPPED rows, handed over in registers like the other
// parameters (the kernel never reads f_rest through `in`: in.f_rest and ma.rp are the same memory).  SHDIR as slam_project_bin_kernel's.
template <bool WORLD, bool SH = false, int SHDIR = 0>
__global__ void __launch_bounds__(FB)
slam_adam_project_kernel(CamDev cam, int P, SlamIn in, int32_t* __restrict__ radii, GeomView g, ImageView iv, BinView b, SlamGrads gr, MapAdam ma,
                         const float* __restrict__ next_pose, uint32_t cap, int slot_bits) {
  static_assert(!SH || WORLD == (SHDIR == 2), "world-frame means take the direction from the camera centre, pre-transformed ones from the mean or the origin");
  extern __shared__ uint32_t hist[];
  const PoseProj un = load_pose_proj(next_pose, cam.proj);      // (before the first store of the kernel)
  const int idx = slam_bin_prologue(cam, iv, cap, hist);
  RawGaussian rg = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.f};
  float rs[SH ? 45 : 1];      // (SH) the stepped f_rest rows the colour reads: [k - 1][3] for k < (sh_deg + 1)^2, compile-time indices only
  if (idx < P) {
    constexpr int AG_OFF[5] = {0, 3, 6, 7, 10}, AG_N[5] = {3, 3, 1, 3, 4};     // xyz | f_dc | opacity | scaling | rotation
    const float* gsrc[5] = {gr.d_xyz, gr.d_f_dc, gr.d_opacity, gr.d_scaling, gr.d_rotation};
    float ap[14], am[14], av[14], g14[14];
#pragma unroll
    for (int gq = 0; gq < 5; gq++)
#pragma unroll
      for (int c = 0; c < AG_N[gq]; c++) {
        const size_t off = (size_t)idx * AG_N[gq] + c;
        ap[AG_OFF[gq] + c] = ma.p[gq][off]; am[AG_OFF[gq] + c] = ma.m[gq][off]; av[AG_OFF[gq] + c] = ma.v[gq][off];
        g14[AG_OFF[gq] + c] = gsrc[gq][off];
      }
    const float keepg = (ma.opt_mask && ma.opt_mask[idx] == 0) ? 0.f : 1.f;
#pragma unroll
    for (int gq = 0; gq < 5; gq++)
#pragma unroll
      for (int c = 0; c < AG_N[gq]; c++) {
        const int q = AG_OFF[gq] + c;
        const float grd = keepg * g14[q];
        AdamElem r;
        adam_moments(am[q], av[q], grd, ma.omb1, ma.beta2, ma.omb2, r);
        am[q] = r.m; av[q] = r.v;
        ap[q] = adam_param(ap[q], r, ma.bc2s, ma.eps, ma.step_size[gq]);
      }
#pragma unroll
    for (int gq = 0; gq < 5; gq++)
      store_adam_rows(AG_N[gq], ma.p[gq], ma.m[gq], ma.v[gq], idx, ap + AG_OFF[gq], am + AG_OFF[gq], av + AG_OFF[gq]);
    if constexpr (SH) {
      // the sixth group, row by row (slam_bwd_body's arithmetic): rows the active degree does not reach take a zero gradient
      const int nb = (in.sh_deg + 1) * (in.sh_deg + 1);
      const size_t base = (size_t)idx * (size_t)in.n_rest * 3;
#pragma unroll
      for (int k = 1; k < 16; k++)
        if (k - 1 < in.n_rest) {
#pragma unroll
          for (int ch = 0; ch < 3; ch++) {
            const size_t off = base + (size_t)(k - 1) * 3 + ch;
            const float grd = k < nb ? keepg * gr.d_f_rest[off] : 0.f;
            const float m0 = ma.rm[off], v0 = ma.rv[off];
            AdamElem r;
            adam_moments(m0, v0, grd, ma.omb1, ma.beta2, ma.omb2, r);
            ma.rm[off] = r.m; ma.rv[off] = r.v;
            const float pn = adam_param(ma.rp[off], r, ma.bc2s, ma.eps, ma.rest_step_size);
            ma.rp[off] = pn;
            rs[(k - 1) * 3 + ch] = pn;
          }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) { rg.x[k] = ap[k]; rg.fd[k] = ap[3 + k]; rg.ls[k] = ap[7 + k]; }
    rg.op = ap[6];
#pragma unroll
    for (int k = 0; k < 4; k++) rg.q[k] = ap[10 + k];
  }
  if constexpr (SH) {
    const Projected pr = slam_project_vals<true, SHDIR>(cam, idx < P, idx, un.pose, un.PV, in.isotropic != 0, rg, radii, g, WORLD, false, rs, in.sh_deg);
    slam_bin_pairs(cam, P, idx, pr, g, iv, b, cap, slot_bits, hist);
  } else {
    const Projected pr = slam_project_vals(cam, idx < P, idx, un.pose, un.PV, in.isotropic != 0, rg, radii, g, WORLD);
    slam_bin_pairs(cam, P, idx, pr, g, iv, b, cap, slot_bits, hist);
  }
}

void launch_slam_adam_project(const CamDev& cam, int P, const SlamIn& in, int32_t* radii, GeomView g, ImageView iv, BinView b, const SlamGrads& gr,
                              const MapAdam& ma, const float* next_pose, uint32_t bin_cap, int slot_bits, hipStream_t s) {
  if (P <= 0) return;
  const int T = cam.gx * cam.gy;
  // (ABI 212; api.hip admits world_means = 1 with sh_dir = 2 only, and sh_dir = 2 with world_means = 1 only)
  auto k = in.sh_deg <= 0 ? (in.world ? slam_adam_project_kernel<true> : slam_adam_project_kernel<false>)
         : in.sh_dir == 2 ? slam_adam_project_kernel<true, true, 2> : in.sh_dir == 1 ? slam_adam_project_kernel<false, true, 1> : slam_adam_project_kernel<false, true, 0>;
  hipLaunchKernelGGL(k, dim3((P + FB - 1) / FB), dim3(FB), (size_t)T * 4, s, cam, P, in, radii, g, iv, b, gr, ma, next_pose, bin_cap, slot_bits);
}

// b^t for a step counter t >= 1 by squaring, in double (pow() costs this one-lane code ~60 registers of the whole kernel it is inlined into)
__device__ __forceinline__ double pow_int(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1) { if (t & 1) r *= b; b *= b; }
  return r;
}

// Fixed-order double-precision sum of the workgroup rows, chain rule (dR, dt) -> (dq, dt) through R(q/|q|), then (optionally) the pose
// Adam step of slam/tracker.py:233-246,160-162 (torch.optim.Adam defaults: betas (0.9, 0.999), eps 1e-8) -- entirely on the device, so
// a tracking iteration needs no host round trip.  One workgroup of 16 * NG lanes: lane = 16 * rowgroup + column; NG row groups keep the
// dependent-load chains short, then the groups are added in a fixed order (deterministic, double precision).
template <int NG>
__device__ __forceinline__ void pose_finish_body(const float* __restrict__ posepartial, int nrows, const float* __restrict__ pose_in,
                                                 float* __restrict__ dpose, const PoseAdam& ad, const PoseLossScale& pls, float* __restrict__ ad_loss4,
                                                 const uint32_t* __restrict__ ovf) {
  static_assert(NG % 8 == 0, "row groups are folded eight at a time");
  __shared__ double part[NG][16];
  __shared__ double part8[NG / 8][16];
  __shared__ double tot[16];
  const int k = threadIdx.x;
  // lane 0's pose / Adam state: requested first, lands while the rows are summed (this kernel is pure latency)
  float pin[4] = {1.f, 0.f, 0.f, 0.f}, pcur[7], am[7], av[7], prior[7], ptr_in[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 7; i++) { pcur[i] = 0.f; am[i] = 0.f; av[i] = 0.f; prior[i] = 0.f; }
  int step0 = 0;
  uint32_t ovf_word = 0u;
  if (k == 0) {
    if (ovf) ovf_word = *ovf;                           // (requested with the rest of lane 0's state: nothing waits for it)
#pragma unroll
    for (int i = 0; i < 4; i++) pin[i] = pose_in[i];    // the quaternion the render used (chain rule)
    if (ad.prior) {
#pragma unroll
      for (int i = 0; i < 7; i++) prior[i] = ad.prior[i];
#pragma unroll
      for (int i = 0; i < 3; i++) ptr_in[i] = pose_in[4 + i];
    }
    if (ad.pose) {
#pragma unroll
      for (int i = 0; i < 7; i++) { pcur[i] = ad.pose[i]; am[i] = ad.m[i]; av[i] = ad.v[i]; }
      step0 = *ad.step;
    }
  }
  {
    const int col = k & 15, grp = k >> 4;
    double a0 = 0.0, a1 = 0.0;
    if (col < NPOSE) {
      // (all of a lane's rows are requested before the first one is added: with the loads inside the loop every pair of rows
      //  cost a memory round trip of its own -- 5 in a row at 157 k Gaussians -- in this one-workgroup kernel)
      int r = grp;
      for (; r + 7 * NG < nrows; r += 8 * NG) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = *(posepartial + (size_t)(r + u * NG) * 32 + col);
#pragma unroll
        for (int u = 0; u < 8; u += 2) { a0 += (double)v[u]; a1 += (double)v[u + 1]; }
      }
      {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = (r + u * NG < nrows) ? *(posepartial + (size_t)(r + u * NG) * 32 + col) : 0.f;
#pragma unroll
        for (int u = 0; u < 8; u += 2) { a0 += (double)v[u]; a1 += (double)v[u + 1]; }
      }
    } else if (pls.rows) {   // columns 12, 13 and their helpers 14, 15 (odd row groups): L1 sum, pixel count
      // deferred masked-L1 normalisation: columns 12 / 13 sum the loss rows' L1 sum / pixel count
      // (four independent accumulators: 19 dependent loads in a row cost ~6 us of latency in this one-workgroup kernel)
      const double* lr = pls.rows + ((col - NPOSE) & 1);
      double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
      int r = grp + NG * ((col - NPOSE) >> 1);      // columns 12/13 take rows grp + 2 NG k, columns 14/15 rows grp + NG + 2 NG k
      for (; r + 6 * NG < pls.nrows; r += 8 * NG) {
        b0 += lr[(size_t)r * 12]; b1 += lr[(size_t)(r + 2 * NG) * 12]; b2 += lr[(size_t)(r + 4 * NG) * 12]; b3 += lr[(size_t)(r + 6 * NG) * 12];
      }
      for (; r < pls.nrows; r += 2 * NG) b0 += lr[(size_t)r * 12];
      a0 = (b0 + b1) + (b2 + b3);
    }
    part[grp][col] = a0 + a1;
  }
  __syncthreads();
  // NG row groups -> NG / 8 -> 1 in a fixed order (a 64-step serial sum of dependent LDS reads cost ~2 us of pure latency)
  if ((k >> 4) < NG / 8) {
    double acc = 0.0;
#pragma unroll
    for (int gq = 0; gq < 8; gq++) acc += part[(k >> 4) * 8 + gq][k & 15];
    part8[k >> 4][k & 15] = acc;
  }
  __syncthreads();
  if (k < 16) {
    double acc = 0.0;
#pragma unroll
    for (int gq = 0; gq < NG / 8; gq++) acc += part8[gq][k];
    tot[k] = acc;
  }
  __syncthreads();
  if (k == 0) {
    if (pls.rows) {
      // dL/d(image) was left unnormalised (sign * w_l1 / 3 on the masked pixels): the pose gradient is linear in it
      tot[NPOSE] += tot[NPOSE + 2]; tot[NPOSE + 1] += tot[NPOSE + 3];
      const double npx = tot[NPOSE + 1];
      const double sc = npx > 0.0 ? 1.0 / npx : 0.0;
      for (int i = 0; i < NPOSE; i++) tot[i] *= sc;
      if (pls.loss4) {
        const double l1 = npx > 0.0 ? tot[NPOSE] / (3.0 * npx) : 0.0;
        pls.loss4[0] = (float)(pls.w_l1 * l1); pls.loss4[1] = (float)l1; pls.loss4[2] = 0.f; pls.loss4[3] = 0.f;
      }
    }
    const float w0 = pin[0], x0 = pin[1], y0 = pin[2], z0 = pin[3];
    const float n = sqrtf(w0 * w0 + x0 * x0 + y0 * y0 + z0 * z0), inv = 1.f / n;
    float dR[3][3];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) dR[i][j] = (float)tot[i * 3 + j];
    const float qn[4] = {w0 * inv, x0 * inv, y0 * inv, z0 * inv};
    float grad[7];
    dR_to_dq_raw(qn, inv, dR, grad);
    for (int i = 0; i < 3; i++) grad[4 + i] = (float)tot[9 + i];
    if (ad.prior) {
      // IMU relative-pose residual (utils/loss_utils.py:20-40, slam/tracker.py:146-155), on the RAW pose like the reference:
      //   w_t |t - t0|^2 + w_q 2 acos(|d_w|),  d = normalize(q (x) conj(q0))   (Hamilton product, utils/pose_utils.py:219-237)
      const float w2 = prior[0], x2 = -prior[1], y2 = -prior[2], z2 = -prior[3];
      const float d0 = w0 * w2 - x0 * x2 - y0 * y2 - z0 * z2, d1 = w0 * x2 + x0 * w2 + y0 * z2 - z0 * y2;
      const float d2 = w0 * y2 - x0 * z2 + y0 * w2 + z0 * x2, d3 = w0 * z2 + x0 * y2 - y0 * x2 + z0 * w2;
      const float dn = fmaxf(sqrtf(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3), 1e-12f), idn = 1.f / dn;
      const float u0 = d0 * idn, u1 = d1 * idn, u2 = d2 * idn, u3 = d3 * idn;
      const float s2 = 1.f - u0 * u0;
      float t_l = 0.f;
#pragma unroll
      for (int i = 0; i < 3; i++) { const float e = ptr_in[i] - prior[4 + i]; t_l += e * e; grad[4 + i] += ad.prior_w_t * 2.f * e; }
      const float ang = 2.f * acosf(fminf(fabsf(u0), 1.f));
      if (s2 > 0.f) {     // at q == q0 the reference's autograd yields NaN (acos'(1) = -inf times 0); taken as 0 here
        const float coef = ad.prior_w_q * -2.f * (u0 < 0.f ? -1.f : 1.f) / sqrtf(s2);
        // dL/dd = coef (e_w - u_w u) / |d|, then through the (linear) Hamilton product
        const float g0 = coef * (1.f - u0 * u0) * idn, g1 = coef * (-u0 * u1) * idn, g2 = coef * (-u0 * u2) * idn, g3 = coef * (-u0 * u3) * idn;
        grad[0] += g0 * w2 + g1 * x2 + g2 * y2 + g3 * z2;
        grad[1] += -g0 * x2 + g1 * w2 - g2 * z2 + g3 * y2;
        grad[2] += -g0 * y2 + g1 * z2 + g2 * w2 - g3 * x2;
        grad[3] += -g0 * z2 - g1 * y2 + g2 * x2 + g3 * w2;
      }
      float* l4 = pls.loss4 ? pls.loss4 : ad_loss4;
      if (l4) l4[0] += ad.prior_w_t * t_l + ad.prior_w_q * ang;    // after the image terms were written (same stream)
    }
    // the iteration's total loss (image terms of the launches before this one, or of the deferred masked L1 above, + the prior): only read
    // when a best candidate is kept
    float* const l4_total = pls.loss4 ? pls.loss4 : ad_loss4;
    if (dpose) for (int i = 0; i < 7; i++) dpose[i] = grad[i];
    // (an iteration whose forward overflowed its capacity is void, see slam_bwd_body: the pose keeps its value AND its Adam state)
    if (ad.pose && ovf_word == 0u) {
      const int t = step0 + 1;
      *ad.step = t;
      // scalars in double, rounded once to float (torch.optim.Adam does this arithmetic on Python floats)
      const double bc1 = 1.0 - pow_int(ad.beta1, t);
      const float bc2s = (float)sqrt(1.0 - pow_int(ad.beta2, t));
      const float omb1 = (float)(1.0 - ad.beta1), b2 = (float)ad.beta2, omb2 = (float)(1.0 - ad.beta2);
      const float ss_q = (float)(ad.lr_q / bc1), ss_t = (float)(ad.lr_t / bc1);
      for (int i = 0; i < 7; i++) {
        const AdamElem r = adam_elem(pcur[i], am[i], av[i], grad[i], omb1, b2, omb2, bc2s, ad.eps, i < 4 ? ss_q : ss_t);
        ad.m[i] = r.m; ad.v[i] = r.v;
        pcur[i] = r.p;
        ad.pose[i] = pcur[i];
      }
      if (ad.best && l4_total) {      // Mm3dgsPoseAdam.best: the loss at the pose the render used against the best so far, the candidate is the stepped pose
        const float lt = l4_total[0];
        if (lt < ad.best[0]) {
          ad.best[0] = lt;
          for (int i = 0; i < 7; i++) ad.best[1 + i] = pcur[i];
        }
      }
    }
  }
}

__global__ void __launch_bounds__(1024) slam_pose_finish_kernel(const float* __restrict__ posepartial, int nrows, const float* __restrict__ pose_in,
                                        float* __restrict__ dpose, PoseAdam ad, PoseLossScale pls, float* __restrict__ ad_loss4,
                                        const uint32_t* __restrict__ ovf) {
  pose_finish_body<64>(posepartial, nrows, pose_in, dpose, ad, pls, ad_loss4, ovf);
}

// The backward projection of an iteration that needs the pose gradient (every tracking iteration; mapping views under bundle adjustment).
// (The pose finish in the LAST workgroup of this launch -- a ticket counter -- was measured and rejected: 25 .. 32 us against 9.1 + 6.8 for the two
// launches; the finish stays a one-workgroup launch of its own, slam_pose_finish_kernel.)
template <bool TRACK, bool DIRECT, bool WORLD, bool SH = false, int SHDIR = 0>
__global__ void __launch_bounds__(SLAM_BWD_FB)
slam_preprocess_bwd_kernel(CamDev cam, int P, SlamIn in, const int32_t* __restrict__ radii, GeomView g, BinView bn, uint32_t N_cap,
                           const float* __restrict__ dsub, float* __restrict__ posepartial, SlamGrads out, MapAdam ma,
                           const uint32_t* __restrict__ ovf) {
  const PoseProj u = load_pose_proj(in.pose, cam.proj);
  slam_bwd_body<TRACK, DIRECT, WORLD, SH, SHDIR>(cam, P, in, u, radii, g, N_cap, dsub, posepartial, out, ma, nullptr, ovf);
}

// The pose finish alone, over the per-TILE rows the tracking compositor's pose chain wrote (composite.hip): rows[nrows][32] floats.
void launch_slam_pose_finish(const float* rows, int nrows, const float* pose_in, float* dpose, const PoseAdam& ad, hipStream_t s,
                             const PoseLossScale* pls, float* loss4, const uint32_t* ovf) {
  const PoseLossScale none = {nullptr, 0, 0.f, nullptr};
  hipLaunchKernelGGL(slam_pose_finish_kernel, dim3(1), dim3(1024), 0, s, rows, nrows, pose_in, dpose, ad, pls ? *pls : none, loss4, ovf);
}

// runtime (sh_deg, sh_dir, world, mapping or tracking records) -> instantiation; DIRECT = direct bins
template <bool DIRECT>
static auto pick_slam_preprocess_bwd(const SlamIn& in, bool map) -> decltype(&slam_preprocess_bwd_kernel<false, DIRECT, false>) {
  // an active SH degree > 0 runs on mapping-layout records even when only the pose gradient is wanted
  // (sh_dir: 0 -- the instances of ABI 209; 1 -- world mean about the origin; 2 -- world-frame means, direction from the camera centre)
  if (in.sh_deg > 0)
    return in.sh_dir == 2 ? slam_preprocess_bwd_kernel<false, DIRECT, true, true, 2>
         : in.sh_dir == 1 ? slam_preprocess_bwd_kernel<false, DIRECT, false, true, 1> : slam_preprocess_bwd_kernel<false, DIRECT, false, true, 0>;
  if (in.world) return map ? slam_preprocess_bwd_kernel<false, DIRECT, true> : slam_preprocess_bwd_kernel<true, DIRECT, true>;
  return map ? slam_preprocess_bwd_kernel<false, DIRECT, false> : slam_preprocess_bwd_kernel<true, DIRECT, false>;
}

void launch_slam_preprocess_bwd(const CamDev& cam, int P, const SlamIn& in, const int32_t* radii, GeomView g, BinView b, size_t N_cap,
                                BwdView bw, const SlamGrads& out, float* dpose, const PoseAdam& ad, const MapAdam& ma, hipStream_t s,
                                const PoseLossScale* pls, float* loss4, bool direct, const uint32_t* ovf) {
  const uint32_t ncap = (uint32_t)(N_cap > 0xffffffffull ? 0xffffffffull : N_cap);
  const bool want_pose = dpose != nullptr || ad.pose != nullptr;
  float* partial = want_pose ? bw.campartial : nullptr;
  if (P > 0) {
    const bool map = out.d_xyz || ma.on;
    auto kern = direct ? pick_slam_preprocess_bwd<true>(in, map) : pick_slam_preprocess_bwd<false>(in, map);
    hipLaunchKernelGGL(kern, dim3((P + SLAM_BWD_FB - 1) / SLAM_BWD_FB), dim3(SLAM_BWD_FB), 0, s, cam, P, in, radii, g, b, ncap, bw.dsub, partial, out, ma, ovf);
  }
  // (rows = workgroups of the launch above; the partial-row region is sized for 256-lane workgroups writing double rows, i.e. it holds
  //  twice as many float rows)
  if (want_pose) launch_slam_pose_finish(bw.campartial, P > 0 ? (P + SLAM_BWD_FB - 1) / SLAM_BWD_FB : 0, in.pose, dpose, ad, s, pls, loss4, ovf);
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused Adam over the map's parameter groups (slam/gaussian_model.py:143-195: Adam(lr=0, eps=1e-15), one group per
// parameter; same update formula as torch.optim.Adam).  One launch for all groups.
__global__ void __launch_bounds__(256) fused_adam_kernel(AdamArgs a) {
  const unsigned long long tid = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  for (int gi = 0; gi < a.ngroups; gi++) {
    const AdamGroup G = a.grp[gi];
    const float step = G.step_size;
    const bool vec = ((G.n & 3ull) == 0) && ((((uintptr_t)G.p | (uintptr_t)G.g | (uintptr_t)G.m | (uintptr_t)G.v) & 15) == 0);
    if (vec) {
      const unsigned long long n4 = G.n >> 2;
      float4* p4 = (float4*)G.p; const float4* g4 = (const float4*)G.g; float4* m4 = (float4*)G.m; float4* v4 = (float4*)G.v;
      for (unsigned long long i = tid; i < n4; i += stride) {
        float4 pr = p4[i], gr = g4[i], mi = m4[i], vi = v4[i];
        float* pp = (float*)&pr; const float* gg = (const float*)&gr; float* mm = (float*)&mi; float* vv = (float*)&vi;
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const AdamElem r = adam_elem(pp[c], mm[c], vv[c], gg[c], a.omb1, a.beta2, a.omb2, a.bc2s, a.eps, step);
          mm[c] = r.m; vv[c] = r.v; pp[c] = r.p;
        }
        p4[i] = pr; m4[i] = mi; v4[i] = vi;
      }
    } else {
      for (unsigned long long i = tid; i < G.n; i += stride) {
        const float gr = G.g[i];
        const AdamElem r = adam_elem(G.p[i], G.m[i], G.v[i], gr, a.omb1, a.beta2, a.omb2, a.bc2s, a.eps, step);
        G.m[i] = r.m; G.v[i] = r.v; G.p[i] = r.p;
      }
    }
  }
}
void launch_fused_adam(const AdamArgs& a, hipStream_t s) {
  unsigned long long tot = 0;
  for (int i = 0; i < a.ngroups; i++) tot = tot > a.grp[i].n ? tot : a.grp[i].n;
  if (!tot) return;
  int blocks = (int)((tot / 4 + 255) / 256) + 1;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(fused_adam_kernel, dim3(blocks), dim3(256), 0, s, a);
}

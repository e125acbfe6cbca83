// Map surgery on the device (8f row 2): the pruning predicate, order-preserving stream compaction of the
// SoA state (parameters + Adam moments + densification statistics) and the seeding of new Gaussians from an RGB-D frame.
//
// Reference: slam/gaussian_model.py:380-451 (prune_points / _prune_optimizer: every per-Gaussian tensor keeps the rows with
// mask == false, in order), :574-588 (prune: sigmoid(opacity) < min_opacity, max exp(scaling) > 0.1 extent, max_radii2D > size
// threshold), slam/mapper.py:409-493,600-688 (one Gaussian per selected pixel in raster order: back-projected position,
// log-scale log(z / ((fx + fy) / 2)) on all axes, opacity logit 0, identity quaternion, f_dc = (rgb - 0.5) / C0).
//
// Compaction = three small launches over `n` flagged elements (Gaussians or pixels): per-256 counts, one workgroup scanning the
// counts, scatter by rank.  Order preserving and deterministic (no atomics decide a position).  Densification (clone + split,
// slam/gaussian_model.py:490-592) is the same machinery with three classes: classify + count, three scans, one scatter.
#include "mm3dgs_common.h"
#include <algorithm>
#include "fused_api.h"
#include "mm3dgs_math.h"       // quat_to_R
#include "block_ops.h"         // scan_block_counts, block_rank, block_flag_counts, block_sums_u32, Carve
#include "view_pixel.h"        // Rigid, rigid_from_pose (shared with pointcloud.hip and tsdf.hip)

#define CB 256

__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || a > b) ? a : b; }      // torch.max: NaN wins

// keep[i] = !pruned; *n_pruned += number of pruned elements (sticky device counter: the host may read it much later)
__global__ void __launch_bounds__(CB)
prune_mask_kernel(int P, const float* __restrict__ opacity, const float* __restrict__ scaling, const float* __restrict__ max_radii2D,
                  float min_opacity, float max_scale, float max_screen_size, int use_screen, uint8_t* __restrict__ keep,
                  uint32_t* __restrict__ n_pruned) {
  const int i = blockIdx.x * CB + threadIdx.x;
  bool pr = false;
  if (i < P) {
    const float o = 1.f / (1.f + expf(-opacity[i]));      // (accurate exp: the decisions must match torch.sigmoid / torch.exp)
    // (max_nan, not fmaxf: a NaN component makes the scale clause false, as get_scaling.max(dim=1).values > 0.1 extent does)
    const float s = max_nan(max_nan(scaling[(size_t)i * 3], scaling[(size_t)i * 3 + 1]), scaling[(size_t)i * 3 + 2]);
    pr = (o < min_opacity) || (expf(s) > max_scale) || (use_screen && max_radii2D[i] > max_screen_size);
    keep[i] = pr ? 0 : 1;
  }
  const unsigned long long m = __ballot(pr);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_pruned, (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(CB) compact_count_kernel(int n, const uint8_t* __restrict__ keep, uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t wsum[1][CB / 64];
  const int i = blockIdx.x * CB + threadIdx.x;
  const bool kept[1] = {i < n && keep[i] != 0};
  const uint32_t t = block_flag_counts(kept, wsum);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = t;
}

__global__ void __launch_bounds__(1024) compact_scan_kernel(int nb, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ n_keep) {
  scan_block_counts(nb, block_counts, n_keep);
}

__global__ void __launch_bounds__(CB)
compact_rows_kernel(int n, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ block_pre, CompactTable t) {
  __shared__ uint32_t wsum[CB / 64];
  const int i = blockIdx.x * CB + threadIdx.x;
  const bool kept = i < n && keep[i] != 0;
  const uint32_t r = block_rank(kept, block_pre[blockIdx.x], wsum);      // its position among the kept ones
  if (!kept) return;
  for (int a = 0; a < t.n_arrays; a++) {
    const int w = t.width[a];
    const float* s = t.src[a] + (size_t)i * w;
    float* d = t.dst[a] + (size_t)r * w;
    for (int c = 0; c < w; c++) d[c] = s[c];
  }
}

// world->camera 7-vector (qw,qx,qy,qz,tx,ty,tz) -> (R, t) in float32; the quaternion is normalised by its reciprocal norm
__device__ __forceinline__ void pose_to_Rt(const float* __restrict__ pose, float R[3][3], float t[3]) {
  const float n = 1.f / sqrtf(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2] + pose[3] * pose[3]);
  const float q[4] = {pose[0] * n, pose[1] * n, pose[2] * n, pose[3] * n};
  quat_to_R(q, R);
  t[0] = pose[4]; t[1] = pose[5]; t[2] = pose[6];
}

// pixel i (raster order) with keep[i] seeds Gaussian row0 + rank(i)
__global__ void __launch_bounds__(CB)
seed_gaussians_kernel(int H, int W, const float* __restrict__ color, const float* __restrict__ depth, const uint8_t* __restrict__ keep,
                      const uint32_t* __restrict__ block_pre, const float* __restrict__ pose, float fx, float fy, float cx, float cy, uint32_t row0,
                      SeedOut o) {
  __shared__ uint32_t wsum[CB / 64];
  const int n = H * W;
  const int i = blockIdx.x * CB + threadIdx.x;
  const bool kept = i < n && keep[i] != 0;
  const uint32_t r = row0 + block_rank(kept, block_pre[blockIdx.x], wsum);
  if (!kept) return;
  // camera-to-world of the world-to-camera pose (qw,qx,qy,qz,tx,ty,tz): x_w = R^T (x_c - t)
  float R[3][3], t[3];
  pose_to_Rt(pose, R, t);
  const int u = i % W, v = i / W;
  const float z = depth[i];
  const float c[3] = {((float)u - cx) / fx * z - t[0], ((float)v - cy) / fy * z - t[1], z - t[2]};
#pragma unroll
  for (int a = 0; a < 3; a++) o.xyz[(size_t)r * 3 + a] = R[0][a] * c[0] + R[1][a] * c[1] + R[2][a] * c[2];
  const float ls = logf(z / ((fx + fy) * 0.5f));     // log sqrt((z / f)^2)
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float rgb = color[(size_t)a * n + i];
    o.rgb[(size_t)r * 3 + a] = rgb;
    o.f_dc[(size_t)r * 3 + a] = (rgb - 0.5f) / 0.28209479177387814f;
    o.scaling[(size_t)r * 3 + a] = ls;
  }
  for (int a = 0; a < o.n_rest * 3; a++) o.f_rest[(size_t)r * o.n_rest * 3 + a] = 0.f;
  o.opacity[r] = 0.f;
  o.rotation[(size_t)r * 4] = 1.f; o.rotation[(size_t)r * 4 + 1] = 0.f; o.rotation[(size_t)r * 4 + 2] = 0.f; o.rotation[(size_t)r * 4 + 3] = 0.f;
}

// ---- densification (slam/gaussian_model.py:490-592): clone + split as one classify-and-plan pass and one scatter ---------------------
// Class per row: 0 kept, 1 cloned (kept + a copy appended), 2 split (replaced by N children).  Three order-preserving ranks per row --
// among the rows that stay (class < 2), the clones, the split rows -- from per-workgroup counts and one scan per class; the scatter
// recomputes them from the class bytes by ballot, like compact_rows_kernel.  Output order (the reference's after its clone, split and
// prune-of-parents sequence): [kept rows][clones][child 0 of each split row]...[child N-1].
#define DENSIFY_KEEP 0
#define DENSIFY_CLONE 1
#define DENSIFY_SPLIT 2

__global__ void __launch_bounds__(CB)
densify_classify_kernel(int P, int nb, const float* __restrict__ grad_accum, const float* __restrict__ denom, const float* __restrict__ scaling,
                        float max_grad, float max_clone_scale, uint8_t* __restrict__ cls, uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t wsum[3][CB / 64];
  const int i = blockIdx.x * CB + threadIdx.x;
  int c = 3;
  if (i < P) {
    float g = grad_accum[i] / denom[i];
    if (g != g) g = 0.f;                                   // rows never seen: 0 / 0
    // (accurate exp, as the prune predicate: the decisions must match torch.exp)
    const float s = max_nan(max_nan(expf(scaling[(size_t)i * 3]), expf(scaling[(size_t)i * 3 + 1])), expf(scaling[(size_t)i * 3 + 2]));
    c = g >= max_grad ? (s > max_clone_scale ? DENSIFY_SPLIT : (s <= max_clone_scale ? DENSIFY_CLONE : DENSIFY_KEEP)) : DENSIFY_KEEP;
    cls[i] = (uint8_t)c;
  }
  const bool is[3] = {c < 2, c == DENSIFY_CLONE, c == DENSIFY_SPLIT};
  const uint32_t t = block_flag_counts(is, wsum);
  if (threadIdx.x < 3) block_counts[threadIdx.x * nb + blockIdx.x] = t;
}

// workgroup k scans class k's block counts; counts[k] = its total
__global__ void __launch_bounds__(1024) densify_scan_kernel(int nb, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ counts) {
  scan_block_counts(nb, block_counts + (size_t)blockIdx.x * nb, counts + blockIdx.x);
}

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// parameters (and, with_moments, both moments -- else zeros) of source row i to destination row d, groups skipped by mask bit
__device__ __forceinline__ void densify_copy_row(const DensifyTable& t, int i, uint32_t d, bool with_moments, unsigned skip) {
  for (int a = 0; a < 7; a++) {
    const int w = t.width[a];
    if (w == 0) continue;
    const size_t si = (size_t)i * w, di = (size_t)d * w;
    if (!((skip >> a) & 1u))
      for (int c = 0; c < w; c++) t.dst[a][di + c] = t.src[a][si + c];
    if (t.m_dst[a])
      for (int c = 0; c < w; c++) t.m_dst[a][di + c] = with_moments ? t.m_src[a][si + c] : 0.f;
    if (t.v_dst[a])
      for (int c = 0; c < w; c++) t.v_dst[a][di + c] = with_moments ? t.v_src[a][si + c] : 0.f;
  }
  t.grad_accum[d] = 0.f; t.denom[d] = 0.f; t.max_radii2D[d] = 0.f;
  if (t.parent) t.parent[d] = i;
}

__global__ void __launch_bounds__(CB)
densify_rows_kernel(int P, int nb, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ block_pre, uint32_t n_keep, uint32_t n_clone,
                    uint32_t n_split, int N, uint32_t seed, float shrink, DensifyTable t) {
  __shared__ uint32_t wsum[3][CB / 64];
  const int i = blockIdx.x * CB + threadIdx.x;
  const int c = i < P ? cls[i] : 3;
  const uint32_t r_keep = block_rank(c < 2, block_pre[blockIdx.x], wsum[0]);
  const uint32_t r_clone = block_rank(c == DENSIFY_CLONE, block_pre[nb + blockIdx.x], wsum[1]);
  const uint32_t r_split = block_rank(c == DENSIFY_SPLIT, block_pre[2 * nb + blockIdx.x], wsum[2]);
  if (i >= P) return;
  if (c != DENSIFY_SPLIT) {
    densify_copy_row(t, i, r_keep, true, 0u);
    if (c == DENSIFY_CLONE) densify_copy_row(t, i, n_keep + r_clone, false, 0u);
    return;
  }
  // split: N children with xyz = R(normalize(q)) (exp(s) * z) + xyz, scaling = log(exp(s) / (0.8 N)) (gaussian_model.py:490-515)
  // (R written out, not quat_to_R: through the helper the compiler contracts the children's xyz differently -- 23 of the 55 densification
  // runs of tests/surgery_cases.py changed bytes on an MI355X; the quaternion is divided by its norm, as the reference normalises)
  const float* q = t.src[5] + (size_t)i * 4;
  float w = q[0], x = q[1], y = q[2], z = q[3];
  const float qn = sqrtf(w * w + x * x + y * y + z * z);
  w /= qn; x /= qn; y /= qn; z /= qn;
  const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - w * z), 2.f * (x * z + w * y)},
                         {2.f * (x * y + w * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - w * x)},
                         {2.f * (x * z - w * y), 2.f * (y * z + w * x), 1.f - 2.f * (x * x + y * y)}};
  const float* ls = t.src[4] + (size_t)i * 3;
  const float* p = t.src[0] + (size_t)i * 3;
  const float sc[3] = {expf(ls[0]), expf(ls[1]), expf(ls[2])};
  const uint32_t base = fmix32(fmix32(seed) ^ (uint32_t)i);
  for (int k = 0; k < N; k++) {
    const uint32_t d = n_keep + n_clone + (uint32_t)k * n_split + r_split;
    densify_copy_row(t, i, d, false, (1u << 0) | (1u << 4));
    float v[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      // general_utils.densify_normals, operation for operation in float32
      const uint32_t k0 = fmix32(base ^ (uint32_t)(8 * k + 2 * a)), k1 = fmix32(base ^ (uint32_t)(8 * k + 2 * a + 1));
      const float u0 = ((float)(k0 >> 8) + 0.5f) * 0x1p-24f, u1 = ((float)(k1 >> 8) + 0.5f) * 0x1p-24f;
      v[a] = sc[a] * (sqrtf(-2.f * logf(u0)) * cosf(u1 * 6.28318548f));
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
      t.dst[0][(size_t)d * 3 + a] = R[a][0] * v[0] + R[a][1] * v[1] + R[a][2] * v[2] + p[a];
      t.dst[4][(size_t)d * 3 + a] = logf(sc[a] / shrink);
    }
  }
}

// ---- keyframe test: covisibility ratio of two views (slam/mapper.py:141-173 need_new_keyframe -> get_depth_pointcloud :175-196 +
// is_covisible :198-216): the surface points of the last keyframe (its rendered depth where the silhouette is > 0.99, minus points
// that round to the world origin at 4 decimals) back-projected to the world and projected into the current view;
// counts[0] = points that land inside the image in front of the camera, counts[1] = points tested.  One pass over the rendered
// depth / silhouette planes instead of ~30 element-wise torch launches; a fixed small grid, so only a handful of atomics per counter.
__global__ void __launch_bounds__(CB)
covisibility_ratio_kernel(int H, int W, const float* __restrict__ depth, const float* __restrict__ sil, const float* __restrict__ kf_pose,
                          const float* __restrict__ cur_pose, float fx, float fy, float cx, float cy, uint32_t* __restrict__ counts) {
  float Rk[3][3], tk[3], Rc[3][3], tc[3];
  pose_to_Rt(kf_pose, Rk, tk);
  pose_to_Rt(cur_pose, Rc, tc);
  const int n = H * W;
  uint32_t n_in = 0, n_sel = 0;
  for (int i = blockIdx.x * CB + threadIdx.x; i < n; i += gridDim.x * CB) {
    const float z = sil[i] > 0.99f ? depth[i] : 0.f;
    const float u = (float)(i % W), v = (float)(i / W);
    const float c[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
    // camera -> world of the keyframe (closed-form rigid inverse: R^T x - R^T t), then world -> current camera
    const float tt[3] = {-(Rk[0][0] * tk[0] + Rk[1][0] * tk[1] + Rk[2][0] * tk[2]), -(Rk[0][1] * tk[0] + Rk[1][1] * tk[1] + Rk[2][1] * tk[2]),
                         -(Rk[0][2] * tk[0] + Rk[1][2] * tk[1] + Rk[2][2] * tk[2])};
    float pw[3], p[3];
#pragma unroll
    for (int a = 0; a < 3; a++) pw[a] = c[0] * Rk[0][a] + c[1] * Rk[1][a] + c[2] * Rk[2][a] + tt[a];
    // torch.round(pts, decimals=4).abs().sum(1) > 0  <=>  some coordinate does not round (half to even) to zero
    const bool sel = z > 0.f && (fabsf(pw[0] * 10000.f) > 0.5f || fabsf(pw[1] * 10000.f) > 0.5f || fabsf(pw[2] * 10000.f) > 0.5f);
#pragma unroll
    for (int a = 0; a < 3; a++) p[a] = pw[0] * Rc[a][0] + pw[1] * Rc[a][1] + pw[2] * Rc[a][2] + tc[a];
    const float zc = p[2] + 1e-5f;
    const float uu = (fx * p[0] + cx * p[2]) / zc, vv = (fy * p[1] + cy * p[2]) / zc;
    const bool inside = sel && uu < (float)W && uu > 0.f && vv < (float)H && vv > 0.f && zc > 0.f;
    n_in += inside ? 1u : 0u; n_sel += sel ? 1u : 0u;
  }
  __shared__ uint32_t red[2][CB / 64];
  const uint32_t nn[2] = {n_in, n_sel};
  const uint32_t t = block_sums_u32(nn, red);
  if (threadIdx.x < 2 && t) atomicAdd(&counts[threadIdx.x], t);
}

// ---- work buffers, carved for api.hip: it hands the launchers these pointers, and sizes a buffer by the walk from a null base -----------
// compaction = [uint32 per 256 elements, + 1]; densification = [class byte per row][3 x uint32 per 256 rows, + 1]
uint32_t* compact_work(const void* work, size_t n, size_t* bytes) {
  Carve c = {(uintptr_t)work};
  uint32_t* block_pre = c.take<uint32_t>((n + 255) / 256 + 1);
  if (bytes) *bytes = c.at;
  return block_pre;
}
uint32_t* densify_work(const void* work, size_t P, uint8_t*& cls, size_t* bytes) {
  Carve c = {(uintptr_t)work};
  cls = c.take<uint8_t>(P);
  uint32_t* block_counts = c.take<uint32_t>(3 * ((P + 255) / 256) + 1);
  if (bytes) *bytes = c.at;
  return block_counts;
}

// ---- launchers (called from api.hip) ------------------------------------------------------------------------------------------
void launch_prune_mask(int P, const float* opacity, const float* scaling, const float* max_radii2D, float min_opacity, float max_scale,
                       float max_screen_size, int use_screen, uint8_t* keep, uint32_t* n_pruned, hipStream_t s) {
  if (P <= 0) return;
  hipLaunchKernelGGL(prune_mask_kernel, dim3((P + CB - 1) / CB), dim3(CB), 0, s, P, opacity, scaling, max_radii2D, min_opacity, max_scale,
                     max_screen_size, use_screen, keep, n_pruned);
}
void launch_compact_plan(int n, const uint8_t* keep, uint32_t* block_pre, uint32_t* n_keep, hipStream_t s) {
  const int nb = (n + CB - 1) / CB;
  if (n > 0) hipLaunchKernelGGL(compact_count_kernel, dim3(nb), dim3(CB), 0, s, n, keep, block_pre);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, n > 0 ? nb : 0, block_pre, n_keep);
}
void launch_compact_rows(int n, const uint8_t* keep, const uint32_t* block_pre, const CompactTable& t, hipStream_t s) {
  if (n <= 0 || t.n_arrays <= 0) return;
  hipLaunchKernelGGL(compact_rows_kernel, dim3((n + CB - 1) / CB), dim3(CB), 0, s, n, keep, block_pre, t);
}
void launch_seed_gaussians(int H, int W, const float* color, const float* depth, const uint8_t* keep, const uint32_t* block_pre,
                           const float* pose, float fx, float fy, float cx, float cy, uint32_t row0, const SeedOut& o, hipStream_t s) {
  const int n = H * W;
  if (n <= 0) return;
  hipLaunchKernelGGL(seed_gaussians_kernel, dim3((n + CB - 1) / CB), dim3(CB), 0, s, H, W, color, depth, keep, block_pre, pose, fx, fy, cx, cy,
                     row0, o);
}
void launch_densify_plan(int P, const float* grad_accum, const float* denom, const float* scaling, float max_grad, float max_clone_scale,
                         uint8_t* cls, uint32_t* block_counts, uint32_t* counts, hipStream_t s) {
  const int nb = (P + CB - 1) / CB;
  if (P > 0)
    hipLaunchKernelGGL(densify_classify_kernel, dim3(nb), dim3(CB), 0, s, P, nb, grad_accum, denom, scaling, max_grad, max_clone_scale, cls,
                       block_counts);
  hipLaunchKernelGGL(densify_scan_kernel, dim3(3), dim3(1024), 0, s, nb, block_counts, counts);
}
void launch_densify_rows(int P, const uint8_t* cls, const uint32_t* block_pre, uint32_t n_keep, uint32_t n_clone, uint32_t n_split, int N,
                         uint32_t seed, float shrink, const DensifyTable& t, hipStream_t s) {
  if (P <= 0) return;
  const int nb = (P + CB - 1) / CB;
  hipLaunchKernelGGL(densify_rows_kernel, dim3(nb), dim3(CB), 0, s, P, nb, cls, block_pre, n_keep, n_clone, n_split, N, seed, shrink, t);
}
__global__ void zero_words_kernel(uint32_t* __restrict__ p, int n) {
  if ((int)threadIdx.x < n) p[threadIdx.x] = 0u;
}
void launch_covisibility_ratio(int H, int W, const float* depth, const float* sil, const float* kf_pose, const float* cur_pose, float fx, float fy,
                               float cx, float cy, uint32_t* counts, hipStream_t s) {
  // (a two-word hipMemsetAsync goes through the runtime's fill path: ~75 us before the next kernel starts, measured; a one-wave launch: 5)
  hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(64), 0, s, counts, 2);
  if (H * W <= 0) return;
  const int nb = std::min((H * W + CB - 1) / CB, 64);
  hipLaunchKernelGGL(covisibility_ratio_kernel, dim3(nb), dim3(CB), 0, s, H, W, depth, sil, kf_pose, cur_pose, fx, fy, cx, cy, counts);
}

// ---- rigid 4x4 algebra of the one-lane pose kernels below, in double: Rigid = (R, t), rigid_from_pose (view_pixel.h) ------------------
// closed-form inverse [R^T | -R^T t]
__device__ inline Rigid rigid_inverse(const Rigid& a) {
  Rigid o;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) o.R[i][j] = a.R[j][i];
    o.t[i] = -(a.R[0][i] * a.t[0] + a.R[1][i] * a.t[1] + a.R[2][i] * a.t[2]);
  }
  return o;
}
// a b = [Ra Rb | Ra tb + ta]
__device__ inline Rigid rigid_mul(const Rigid& a, const Rigid& b) {
  Rigid o;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) o.R[i][j] = a.R[i][0] * b.R[0][j] + a.R[i][1] * b.R[1][j] + a.R[i][2] * b.R[2][j];
    o.t[i] = a.R[i][0] * b.t[0] + a.R[i][1] * b.t[1] + a.R[i][2] * b.t[2] + a.t[i];
  }
  return o;
}
// (m, t) -> 7-vector, rounded to float32 at the store: the best-conditioned of the four matrix -> quaternion formulas (the largest of
// |w|, |x|, |y|, |z|; utils/pose_utils.py:285-349,371-383), first maximum like argmax
__device__ inline void store_pose(const double (*m)[3], const double* t, float* __restrict__ out) {
  const double four_sq[4] = {1.0 + m[0][0] + m[1][1] + m[2][2], 1.0 + m[0][0] - m[1][1] - m[2][2], 1.0 - m[0][0] + m[1][1] - m[2][2],
                             1.0 - m[0][0] - m[1][1] + m[2][2]};
  const double cand[4][4] = {{four_sq[0], m[2][1] - m[1][2], m[0][2] - m[2][0], m[1][0] - m[0][1]},
                             {m[2][1] - m[1][2], four_sq[1], m[1][0] + m[0][1], m[0][2] + m[2][0]},
                             {m[0][2] - m[2][0], m[1][0] + m[0][1], four_sq[2], m[1][2] + m[2][1]},
                             {m[1][0] - m[0][1], m[2][0] + m[0][2], m[2][1] + m[1][2], four_sq[3]}};
  int best = 0;
  double mag = sqrt(fmax(four_sq[0], 0.0));
  for (int k = 1; k < 4; k++) {
    const double mk = sqrt(fmax(four_sq[k], 0.0));
    if (mk > mag) { mag = mk; best = k; }       // (first maximum, like argmax)
  }
  const double den = 2.0 * fmax(mag, 0.1);
  for (int k = 0; k < 4; k++) out[k] = (float)(cand[best][k] / den);
  for (int k = 0; k < 3; k++) out[4 + k] = (float)t[k];
}

// ---- constant-velocity pose prediction (utils/pose_utils.py:203-216 propagate_const_vel; :352-383 get_camera_from_tensor /
// get_tensor_from_camera): W' = (W1 W2^-1) W1 for the last two world->camera poses, back to (q, t).  One lane, double precision (the
// tracker used to read the two poses back and do this on the host: a device drain at the head of every frame).  Same algebra as
// pose_utils.propagate_const_vel_np: normalised quaternion -> R, closed-form rigid inverse, best-conditioned matrix -> quaternion branch.
__global__ void propagate_const_vel_kernel(const float* __restrict__ pm1, const float* __restrict__ pm2, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const Rigid W1 = rigid_from_pose(pm1), W2 = rigid_from_pose(pm2);
  const double (*R1)[3] = W1.R, (*R2)[3] = W2.R;
  const double *t1 = W1.t, *t2 = W2.t;
  // step = W1 W2^-1: rotation A = R1 R2^T, translation a = t1 - A t2;  W' = step W1: rotation A R1, translation A t1 + a
  double A[3][3], a[3], m[3][3], tn[3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) A[i][j] = R1[i][0] * R2[j][0] + R1[i][1] * R2[j][1] + R1[i][2] * R2[j][2];
  for (int i = 0; i < 3; i++) a[i] = t1[i] - (A[i][0] * t2[0] + A[i][1] * t2[1] + A[i][2] * t2[2]);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) m[i][j] = A[i][0] * R1[0][j] + A[i][1] * R1[1][j] + A[i][2] * R1[2][j];
    tn[i] = A[i][0] * t1[0] + A[i][1] * t1[1] + A[i][2] * t1[2] + a[i];
  }
  store_pose(m, tn, out);
}
void launch_propagate_const_vel(const float* pm1, const float* pm2, float* out, hipStream_t s) {
  hipLaunchKernelGGL(propagate_const_vel_kernel, dim3(1), dim3(64), 0, s, pm1, pm2, out);
}

// ---- IMU dead-reckoning of the tracker's start pose (utils/pose_utils.py:148-200 propagate_imu, :43-99 euler_matrix 'sxyz'): the IMU pose
// i2w = W1^-1 c2i^-1 of frame idx-1 is stepped through the n samples of the interval -- velocity from the last two poses (constant over the
// samples, as in the reference), gravity removed in the IMU frame, delta = [Rz Ry Rx (omega dt) | v dt + a dt^2 / 2] -- and W' = (i2w c2i)^-1
// goes back to (q, t).  One lane, double precision, same algebra and operation order as pose_utils.propagate_imu_np; the tracker's host path
// read the pose back (a device drain at the head of every frame) and ran this as ~100 one-element float32 torch operators.  The sample
// rows are read only (the reference subtracts gravity from the caller's rows in place; every row is used once, so the pose is the same).
__global__ void propagate_imu_kernel(const float* __restrict__ pm1, const float* __restrict__ pm2, const float* __restrict__ imu6, int n,
                                     const float* __restrict__ c2i, double dt_cam, double dt_imu, double gx, double gy, double gz,
                                     float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Rigid C;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) C.R[i][j] = c2i[4 * i + j];
    C.t[i] = c2i[4 * i + 3];
  }
  const Rigid Ci = rigid_inverse(C);
  const Rigid i2w1 = rigid_mul(rigid_inverse(rigid_from_pose(pm1)), Ci);
  const Rigid i2w2 = rigid_mul(rigid_inverse(rigid_from_pose(pm2)), Ci);
  const Rigid rel = rigid_mul(rigid_inverse(i2w2), i2w1);      // i(idx-1) -> i(idx-2)
  const double vel[3] = {rel.t[0] / dt_cam, rel.t[1] / dt_cam, rel.t[2] / dt_cam};
  Rigid X = i2w1;
  for (int s = 0; s < n; s++) {
    const float* __restrict__ row = imu6 + (size_t)s * 6;      // angular velocity xyz, linear acceleration xyz (gravity included)
    Rigid D;
    for (int k = 0; k < 3; k++) {
      const double acc = (double)row[3 + k] - (X.R[0][k] * gx + X.R[1][k] * gy + X.R[2][k] * gz);      // a - R(i2w)^T g
      D.t[k] = vel[k] * dt_imu + 0.5 * acc * dt_imu * dt_imu;
    }
    const double ai = (double)row[0] * dt_imu, aj = (double)row[1] * dt_imu, ak = (double)row[2] * dt_imu;
    const double si = sin(ai), sj = sin(aj), sk = sin(ak), ci = cos(ai), cj = cos(aj), ck = cos(ak);
    D.R[0][0] = cj * ck; D.R[0][1] = sj * si * ck - ci * sk; D.R[0][2] = sj * ci * ck + si * sk;
    D.R[1][0] = cj * sk; D.R[1][1] = sj * si * sk + ci * ck; D.R[1][2] = sj * ci * sk - si * ck;
    D.R[2][0] = -sj;     D.R[2][1] = cj * si;                D.R[2][2] = cj * ci;
    X = rigid_mul(X, D);
  }
  const Rigid W = rigid_inverse(rigid_mul(X, C));
  store_pose(W.R, W.t, out);
}
void launch_propagate_imu(const float* pm1, const float* pm2, const float* imu6, int n, const float* c2i, double dt_cam, double dt_imu,
                          double gx, double gy, double gz, float* out, hipStream_t s) {
  hipLaunchKernelGGL(propagate_imu_kernel, dim3(1), dim3(64), 0, s, pm1, pm2, imu6, n, c2i, dt_cam, dt_imu, gx, gy, gz, out);
}

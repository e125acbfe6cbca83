// Internal structs + launchers of the fused SLAM path (fused.hip, loss.hip), shared with api.hip.
#pragma once
#include "mm3dgs_common.h"

struct SlamIn {
  const float* pose; const float* xyz; const float* f_dc; const float* opacity; const float* scaling; const float* rotation;
  int isotropic;
  int world;     // Mm3dgsSlamInputs.world_means
  const float* f_rest; int sh_deg; int n_rest;      // active SH degree > 0 (ABI 209): rows [P][n_rest][3]; sh_deg == 0: unused
  int sh_dir;    // Mm3dgsSlamInputs.sh_dir (ABI 211): the SH viewing direction's source; 0 whenever sh_deg == 0
};
struct SlamGrads {
  float* d_xyz; float* d_f_dc; float* d_opacity; float* d_scaling; float* d_rotation;
  float* max_radii2D; float* grad_accum; float* denom;
  float* d_f_rest;
};
// Adam scalars as torch.optim.Adam applies them: formed in double on the host, rounded once to float.
//   omb1 = 1 - beta1 (lerp weight), beta2, omb2 = 1 - beta2, step_size = lr / (1 - beta1^t) per group, bc2s = sqrt(1 - beta2^t)
struct MapAdam { float* p[5]; float* m[5]; float* v[5]; float step_size[5]; float omb1, beta2, omb2, eps, bc2s; int on; const uint8_t* opt_mask;
                 float* rp; float* rm; float* rv; float rest_step_size; };      // (the sixth group: f_rest, active SH degree > 0)
struct PoseAdam { float* pose; float* m; float* v; int* step; double lr_q, lr_t, beta1, beta2; float eps; const float* prior; float prior_w_t, prior_w_q; float* best; };
struct AdamGroup { float* p; const float* g; float* m; float* v; unsigned long long n; float step_size; };
struct AdamArgs { AdamGroup grp[8]; int ngroups; float omb1, beta2, omb2, eps, bc2s; };
struct LossCfg {
  int H, W;
  float w_l1, w_ssim, w_pearson;
  int l1_mask, pearson_mask, pearson_invert;
  float sil_thr;
  float window[11];
  // `method: splatam` forms (standalone loss kernels only; api.hip never folds such a configuration into the compositors):
  float w_depth;       // weight of the depth-L1 term |ref - depth| over depth_mask (bit0 silhouette > sil_thr, bit1 ref > 0)
  int depth_mask;
  int l1_sum;          // the L1 terms are sums over their masks instead of means;  l1_mask bit1: ref > 0
};

// A tracking iteration without SSIM folds the per-pixel loss into the compositors (mm3dgs_slam_track): the forward epilogue
// writes the per-tile partial sums loss_reduce_kernel would, the backward prologue derives dL/d(image) from the finished
// sums instead of reading the gradient image loss_grad_kernel would have written.  Two launches and a 7 MB round trip less.
struct TrackLoss {
  LossCfg cfg;
  const float* gt;      // [3,H,W]
  const float* ref;     // [H,W] or NULL (Pearson off)
  const float* out;     // [6,H,W] the rendered bundle (backward prologue)
  const float* dmaps;   // [9,H,W] SSIM derivative maps (mapping loss folded into the backward compositor's prologue) or NULL
  double* partial;      // [tiles][12]
  const double* sums;   // finished sums (loss_finish_kernel)
  float* loss4;         // {total, l1, 1-ssim, 1-rho} or NULL
  int defer_scale;      // 1: masked-L1 only -- the 1/(3 n) normalisation is applied to the pose gradient by the pose
                        //    finishing kernel (the gradient is linear in dL), so no loss-finish launch is needed at all
};
// the loss partial rows the pose finishing kernel sums when the normalisation is deferred (see TrackLoss::defer_scale)
struct PoseLossScale { const double* rows; int nrows; float w_l1; float* loss4; };
void launch_loss_finish(const LossCfg& cfg, double* sums, const double* partial, hipStream_t s, float* loss4 = nullptr);

void launch_slam_preprocess_fwd(const CamDev& cam, int P, const SlamIn& in, int32_t* radii, GeomView g, ImageView iv, hipStream_t s,
                                uint32_t* seen_only = nullptr, bool visibility_only = false, bool want_poserec = false);
// the pose finish alone over per-tile pose rows (the tracking compositor's pose chain: composite.hip, GeomView.poserec)
void launch_slam_pose_finish(const float* rows, int nrows, const float* pose_in, float* dpose, const PoseAdam& ad, hipStream_t s,
                             const PoseLossScale* pls, float* loss4, const uint32_t* ovf);
void launch_slam_preprocess_bwd(const CamDev& cam, int P, const SlamIn& in, const int32_t* radii, GeomView g, BinView b, size_t N_cap,
                                BwdView bw, const SlamGrads& out, float* dpose, const PoseAdam& ad, const MapAdam& ma, hipStream_t s,
                                const PoseLossScale* pls = nullptr, float* loss4 = nullptr, bool direct = false, const uint32_t* overflow_flag = nullptr);
// dl_planes: 6, or 4 when the caller guarantees that the silhouette / depth^2 planes of dL are zero AND need not be read
// (the mapping loop's loss kernel does not even write them)
// pose_chain (tracking only): apply GeomView.poserec per (block, splat) and write the tile's pose-gradient row to dsub[tile][32] instead of
// gradient records
void launch_composite_bwd_slam(const CamDev& cam, bool tracking, GeomView g, ImageView iv, BinView b, size_t N_cap, const float* dL,
                               float* dsub, hipStream_t s, const TrackLoss* tl = nullptr, int dl_planes = 6, bool pose_chain = false);
// sort + forward compositing of the 6-channel SLAM bundle in one launch (lists <= 2048 per tile stay in LDS)
void launch_sort_composite_fwd6(const CamDev& cam, GeomView g, ImageView iv, BinView b, size_t N_cap, float* out, int clean, hipStream_t s,
                                const TrackLoss* tl = nullptr, int direct_blocks = 0, uint32_t direct_cap = 0, int slot_bits = DIRECT_SLOT_BITS_MAX);
// the same + the backward compositor of a tracking iteration (masked-L1 loss, deferred normalisation) in that launch
void launch_sort_composite_fwd_bwd_track(const CamDev& cam, GeomView g, ImageView iv, BinView b, size_t N_cap, float* out, int clean,
                                         hipStream_t s, const TrackLoss& tl, int direct_blocks, float* dsub, uint32_t direct_cap = 0, int slot_bits = DIRECT_SLOT_BITS_MAX,
                                         bool pose_chain = false);
// backward projection + map Adam of one mapping iteration and projection + binning of the next one (its pose: next_pose) in one launch
void launch_slam_bwd_project(const CamDev& cam, int P, const SlamIn& in, int32_t* radii, GeomView g, ImageView iv, BinView b, size_t N_cap,
                             BwdView bw, const SlamGrads& out, const MapAdam& ma, const float* next_pose, uint32_t bin_cap,
                             int slot_bits, hipStream_t s);
// projection + binning in one launch (direct bins: every tile owns bin_cap pairs at tile * bin_cap)
void launch_slam_project_bin(const CamDev& cam, int P, const SlamIn& in, int32_t* radii, GeomView g, ImageView iv, BinView b, uint32_t bin_cap,
                             int slot_bits, hipStream_t s, bool want_poserec = false);
// the map's Adam step from gradient arrays (the multi-GPU window: all-reduced gradients) + projection + binning of the next view in one launch
void launch_slam_adam_project(const CamDev& cam, int P, const SlamIn& in, int32_t* radii, GeomView g, ImageView iv, BinView b, const SlamGrads& gr,
                              const MapAdam& ma, const float* next_pose, uint32_t bin_cap, int slot_bits, hipStream_t s);
void launch_fused_adam(const AdamArgs& a, hipStream_t s);
void launch_loss(const LossCfg& cfg, const float* out, const float* gt, const float* ref, float* dmaps, double* sums, double* partial,
                 float* dL, float* loss, hipStream_t s);
void launch_loss_after_forward_rows(const LossCfg& cfg, const float* out, const float* gt, const float* ref, float* dmaps, double* sums,
                                    double* partial, float* dL, hipStream_t s);

// ---- map surgery (compact.hip) ----
struct CompactTable { const float* src[32]; float* dst[32]; int width[32]; int n_arrays; };
struct SeedOut { float* xyz; float* f_dc; float* f_rest; float* opacity; float* scaling; float* rotation; float* rgb; int n_rest; };
void launch_prune_mask(int P, const float* opacity, const float* scaling, const float* max_radii2D, float min_opacity, float max_scale,
                       float max_screen_size, int use_screen, uint8_t* keep, uint32_t* n_pruned, hipStream_t s);
void launch_compact_plan(int n, const uint8_t* keep, uint32_t* block_pre, uint32_t* n_keep, hipStream_t s);
void launch_compact_rows(int n, const uint8_t* keep, const uint32_t* block_pre, const CompactTable& t, hipStream_t s);
// densification: groups in the optimiser's order (0 xyz, 1 f_dc, 2 f_rest, 3 opacity, 4 scaling, 5 rotation, 6 rgb); width 0 skips a group,
// NULL moment pointers mean a group without Adam state
struct DensifyTable {
  const float* src[7]; float* dst[7]; const float* m_src[7]; float* m_dst[7]; const float* v_src[7]; float* v_dst[7]; int width[7];
  float* grad_accum; float* denom; float* max_radii2D; int32_t* parent;
};
void launch_densify_plan(int P, const float* grad_accum, const float* denom, const float* scaling, float max_grad, float max_clone_scale,
                         uint8_t* cls, uint32_t* block_counts, uint32_t* counts, hipStream_t s);
void launch_densify_rows(int P, const uint8_t* cls, const uint32_t* block_pre, uint32_t n_keep, uint32_t n_clone, uint32_t n_split, int N,
                         uint32_t seed, float shrink, const DensifyTable& t, hipStream_t s);
void launch_seed_gaussians(int H, int W, const float* color, const float* depth, const uint8_t* keep, const uint32_t* block_pre,
                           const float* pose, float fx, float fy, float cx, float cy, uint32_t row0, const SeedOut& o, hipStream_t s);

void launch_covisibility_ratio(int H, int W, const float* depth, const float* sil, const float* kf_pose, const float* cur_pose, float fx, float fy,
                               float cx, float cy, uint32_t* counts, hipStream_t s);
void launch_propagate_const_vel(const float* pm1, const float* pm2, float* out, hipStream_t s);
// imu6: [n,6] rows (angular velocity xyz, linear acceleration xyz incl. gravity), read only; c2i: 16 floats, row-major camera->IMU
void launch_propagate_imu(const float* pm1, const float* pm2, const float* imu6, int n, const float* c2i, double dt_cam, double dt_imu,
                          double gx, double gy, double gz, float* out, hipStream_t s);
// depth alignment (align.hip): rows = the work buffer of align_depth_work_bytes(H, W); sil and out may be NULL
size_t align_depth_work_bytes(int H, int W);
void launch_align_depth(int H, int W, const float* est, const float* depth, const float* sil, float sil_min, float est_min, double* rows,
                        double* fit, float* out, hipStream_t s);
// image evaluation (eval.hip): PSNR / SSIM / depth L1 of one frame into row[16] (device); rows = the work buffer of
// eval_image_work_bytes(H, W); depth and gt_depth are both NULL or both given; window = the host's 11 SSIM taps; H W <= 2^28
size_t eval_image_work_bytes(int H, int W);
void launch_eval_image(int H, int W, const float* image, const float* gt, const float* depth, const float* gt_depth, const float* window,
                       double* rows, double* row, hipStream_t s);
// one posed pinhole camera: the image size, the intrinsics and the world->camera 7-vector (qw,qx,qy,qz,tx,ty,tz; device).  Every view struct
// below begins with it, api.hip's view_check fills and checks it, view_pixel.h states what the kernels do with it
struct PinholeView { int H, W; double fx, fy, cx, cy; const float* pose; };
// fused point cloud (pointcloud.hip): one view's valid pixels lifted to world points and appended to rows (16 B each) from counters[0],
// thinned to the first point per voxel through the caller's table when voxel > 0 (table NULL otherwise); work = the buffer of
// pointcloud_work_bytes(H, W); H W <= 2^28, slots a power of two >= 64 and hash_shift = 64 - log2(slots), as the entry point has checked
struct PointCloudView : PinholeView {
  const float* color; const float* depth; const float* sil;
  float sil_min, depth_max;
  double voxel;
  uint32_t view;
  unsigned long long* table; uint64_t slots; int hash_shift;
};
size_t pointcloud_work_bytes(int H, int W);
void launch_pointcloud_reset(void* table, uint64_t slots, uint64_t* counters, hipStream_t s);
void launch_pointcloud_add_view(const PointCloudView& v, void* rows, uint64_t cap, uint64_t* counters, void* work, hipStream_t s);
// coloured triangle mesh (tsdf.hip): one view fused into the caller's dense volume (tsdf_w float2, rgb_w float4 over nx x ny x nz samples at
// o + voxel (i, j, k), x fastest), and marching tetrahedra over it in two calls (plan: counts and bases into work = the buffer of
// tsdf_mesh_work_bytes; emit: rows and triangles); every size >= 2 and nx ny nz <= 2^30, as the entry points have checked
struct TsdfView : PinholeView {
  const float* color; const float* depth; const float* sil;
  float sil_min, depth_max;
  double o[3], voxel, trunc;
  int nx, ny, nz;
};
size_t tsdf_mesh_work_bytes(int nx, int ny, int nz);
void launch_tsdf_integrate(const TsdfView& v, void* tsdf_w, void* rgb_w, uint64_t* counters, hipStream_t s);
void launch_tsdf_mesh_plan(int nx, int ny, int nz, const void* tsdf_w, float min_weight, void* work, uint64_t* counters, hipStream_t s);
void launch_tsdf_mesh_emit(int nx, int ny, int nz, const void* tsdf_w, const void* rgb_w, const double* origin, double voxel, const void* work, void* rows,
                           uint64_t vcap, void* tris, uint64_t tcap, uint64_t* counters, hipStream_t s);
// the same as a voxel-block volume (tsdf_sparse.hip): 8 x 8 x 8-sample blocks named by 63-bit keys in the caller's open-addressing table
// ({uint64 key} x slots, {uint32 rank} x slots, per-256 counts), reserved per view, listed, and -- once the caller has sorted the keys --
// indexed; the pool is tsdf_w float2 [n][512], rgb_w float4 [n][512] in the order of the sorted keys.  TsdfView: o = the anchor, nx / ny /
// nz unused.  Sizes, pointers, trunc <= 16 voxel, max_blocks and n <= 2^21: as the entry points have checked
struct TsdfBlockClip { int lo[3], hi[3]; };      // the block coordinates a reservation may touch, inclusive
size_t tsdf_blocks_table_bytes(uint64_t max_blocks, uint64_t* slots);
void launch_tsdf_blocks_reset(void* table, uint64_t max_blocks, uint64_t* counters, hipStream_t s);
void launch_tsdf_blocks_reserve(const TsdfView& v, const TsdfBlockClip& clip, void* table, uint64_t max_blocks, uint64_t* counters, hipStream_t s);
void launch_tsdf_blocks_list(void* table, uint64_t max_blocks, uint64_t* keys, uint64_t cap, hipStream_t s);
void launch_tsdf_blocks_index(void* table, uint64_t max_blocks, const uint64_t* keys, uint64_t n, int* neighbours, uint64_t* counters, hipStream_t s);
void launch_tsdf_blocks_integrate(const TsdfView& v, const uint64_t* keys, uint64_t n, void* tsdf_w, void* rgb_w, uint64_t* counters, hipStream_t s);
size_t tsdf_blocks_mesh_work_bytes(uint64_t n);
void launch_tsdf_blocks_mesh_plan(uint64_t n, const int* neighbours, const void* tsdf_w, float min_weight, void* work, uint64_t* counters, hipStream_t s);
void launch_tsdf_blocks_mesh_emit(uint64_t n, const uint64_t* keys, const int* neighbours, const void* tsdf_w, const void* rgb_w, const double* anchor, double voxel,
                                  const void* work, void* rows, uint64_t vcap, void* tris, uint64_t tcap, uint64_t* counters, hipStream_t s);
// geometry scores (geometry.hip): a uniform grid over a reference point set (16-byte rows), the exact truncated nearest-neighbour distance
// of every query row with one row of eight figures, and area-uniform samples of a triangle mesh; sizes, pointers, cell, max_dist, rmax =
// ceil(max_dist / cell) and density as the entry points have checked them (gx gy gz <= 2^26, at most 2^30 rows, rmax <= 2^20)
struct NnGrid { double cell; double o[3]; int gx, gy, gz; };      // o: the origin cell per axis (an integer value)
struct MeshSample { const uint4* vrows; uint32_t n_vertices; const int* tris; uint32_t m; double density; uint32_t seed; };
size_t nn_grid_work_bytes(uint64_t n_ref, int gx, int gy, int gz);
void launch_nn_grid_build(const NnGrid& g, uint64_t n_ref, const void* rows, void* cell_start, void* sorted, uint64_t* counters, void* work, hipStream_t s);
size_t nn_query_work_bytes(uint64_t n_q);
// index_out_or_null: what the normal scores need, the original reference row of the nearest record per query (0xffffffff: none); the bytes
// of dist_out and row do not depend on it
void launch_nn_query(const NnGrid& g, uint64_t n_q, const void* qrows, uint64_t n_ref, const void* cell_start, const void* sorted, double max_dist,
                     double threshold, int rmax, float* dist_out, uint32_t* index_out_or_null, double* row, void* work, hipStream_t s);
// point-to-point ICP of the query rows onto the grid's reference set: a zeroing launch and 2 (iters + 1) launches, the stop decided on the
// device (state [16], log [iters + 1][16] doubles; dist_out / index_out may be NULL); work = the buffer of icp_work_bytes(n_q); sizes,
// max_dist, rmax, 1 <= iters <= 1000 and the tolerances as the entry point has checked them.  rows_move: rows_out = rows_in moved by T
// (12 doubles on the device, row-major [3][4]); the two arrays may be one
size_t icp_work_bytes(uint64_t n_q);
void launch_icp_point(const NnGrid& g, uint64_t n_q, const void* qrows, uint64_t n_ref, const void* cell_start, const void* sorted, double max_dist, int rmax,
                      int iters, double rel_fitness, double rel_rmse, double* state, double* log, float* dist_out, uint32_t* index_out, void* work, hipStream_t s);
void launch_rows_move(uint64_t n, const void* rows_in, const double* T, void* rows_out, hipStream_t s);
size_t mesh_sample_work_bytes(uint64_t m);
void launch_mesh_sample_plan(const MeshSample& ms, void* work, uint64_t* counters, hipStream_t s);
// tri_out_or_null: the triangle of every sample (the normal scores'); the bytes of rows do not depend on it
void launch_mesh_sample_emit(const MeshSample& ms, const void* work, void* rows, uint32_t* tri_out_or_null, uint64_t cap, uint64_t* counters, hipStream_t s);
// normal consistency of one direction: per query its triangle tri_q[i] of mesh q, its nearest reference row index[i] (0xffffffff: none) and
// that row's triangle tri_r[index[i]] of mesh r -> dot_out[i] and one row of eight figures; density and seed of the meshes are unused;
// work = the buffer of normal_consistency_work_bytes(n_q); n_q, n_r <= 2^30 and the meshes as the entry point has checked them
size_t normal_consistency_work_bytes(uint64_t n_q);
void launch_normal_consistency(uint64_t n_q, const uint32_t* tri_q, const uint32_t* index, uint64_t n_r, const uint32_t* tri_r, const MeshSample& mq,
                               const MeshSample& mr, float* dot_out, double* row, void* work, hipStream_t s);
// area-weighted vertex normals in fixed point (float [n_vertices][3]); work = the buffer of mesh_vertex_normals_work_bytes(n_vertices)
size_t mesh_vertex_normals_work_bytes(uint64_t n_vertices);
void launch_mesh_vertex_normals(const MeshSample& ms, float* normals, void* work, uint64_t* counters, hipStream_t s);
// visibility culling (cull.hip): one view marks the rows (16 bytes each) it sees in seen (uint32 per row, += 1), select keeps the rows with
// seen >= min_views in order; depth NULL = frustum only; work = the buffer of cull_work_bytes(n); n <= 2^30, near / far / eps >= 0 and
// finite, H W <= 2^28, as the entry points have checked
struct CullView : PinholeView {
  const float* depth;
  float depth_max;
  double z_near, z_far, eps;
};
size_t cull_work_bytes(uint64_t n);
void launch_cull_mark_view(const CullView& v, uint64_t n, const void* rows, uint32_t* seen, uint64_t* counters, hipStream_t s);
void launch_cull_select(uint64_t n, const void* rows, const uint32_t* seen, uint32_t min_views, void* out_rows, uint64_t cap, uint32_t* index, void* work,
                        uint64_t* counters, hipStream_t s);
// mesh cleaning (meshclean.hip): label = the smallest vertex of a vertex's component (through valid triangles: three indices in [0, V)),
// tri_count = the valid triangles per label, counters [0..3]; plan: which components the mode keeps, the per-256 counts, their scan and
// the vertex remap into work = the buffer of mesh_clean_work_bytes(V, T), counters [4..7]; emit: kept rows and re-indexed triangles in
// their order below the caps; V, T <= 2^30, mode 1 / 2, min_triangles >= 1 in mode 1, as the entry points have checked
size_t mesh_clean_work_bytes(uint64_t V, uint64_t T);
void launch_mesh_components(uint64_t V, uint64_t T, const int* tris, uint32_t* label, uint32_t* tri_count, uint64_t* counters, hipStream_t s);
void launch_mesh_clean_plan(uint64_t V, uint64_t T, const int* tris, const uint32_t* label, const uint32_t* tri_count, int mode, uint32_t min_triangles,
                            void* work, uint64_t* counters, hipStream_t s);
void launch_mesh_clean_emit(uint64_t V, uint64_t T, const void* rows, const int* tris, const void* work, void* out_rows, uint64_t vcap, int* out_tris,
                            uint64_t tcap, uint32_t* index, uint64_t* counters, hipStream_t s);
// mesh depth (meshdepth.hip): a triangle mesh (16-byte vertex rows, int32 [T][3] triangles) rendered to a depth image [H,W] float32 and the
// winning triangle [H,W] int32 (tri NULL: not written) from one posed camera, through per-tile lists of at most max_pairs (tile, triangle)
// pairs in work = the buffer of mesh_depth_work_bytes; and one row [8] of the comparison of two depth images, work = the buffer of
// depth_compare_work_bytes; V, T <= 2^30, max_pairs <= 2^31, H W <= 2^28, near / far >= 0 and finite, as the entry points have checked
struct MeshDepthView : PinholeView { double z_near, z_far; };
size_t mesh_depth_work_bytes(uint64_t V, uint64_t T, int H, int W, uint64_t max_pairs);
void launch_mesh_depth_render(const MeshDepthView& v, uint64_t V, const void* vrows, uint64_t T, const int* tris, uint64_t max_pairs, float* depth, int* tri,
                              void* work, uint64_t* counters, hipStream_t s);
size_t depth_compare_work_bytes(int H, int W);
void launch_depth_compare(int H, int W, const float* a, const float* b, void* work, double* row, hipStream_t s);
// frame ingest (ingest.hip): raw uint8 RGB [Hs,Ws,3] + uint16 depth [Hs,Ws] -> colour [3,H,W] in [0,1] + depth [H,W] in metres, one
// launch; depth and out_depth are both NULL or both given; H W and Hs Ws are at most 2^30 (the entry point checks)
void launch_ingest_frame(int Hs, int Ws, const uint8_t* rgb, const uint16_t* depth, double depth_scale, int H, int W, float* out_color,
                         float* out_depth, hipStream_t s);
// the monocular depth estimate (ingest.hip): raw [Hs,Ws] float32 (dtype 0) / float16 (1) / uint16 (2) -> float32 [H,W], bilinear, times
// scale, one launch; arguments as the entry point has checked them
void launch_ingest_est(int Hs, int Ws, const void* est, int dtype, double scale, int H, int W, float* out, hipStream_t s);
// debug mosaic (mosaic.hip): rows x cols panels of H x W float32 images -> one interleaved uint8 image [rows H, cols W, 3]; kind 0 colour
// (a [3,H,W]), 1 |a - b|, 2 depth (a [H,W]) through the caller's quantised colour table lut [256,3]; work = mosaic_work_bytes(rows, cols)
// bytes, 8-byte aligned; at most 2^28 pixels and MOSAIC_MAX_PANELS panels, kinds and pointers as the entry point has checked them
#define MOSAIC_MAX_PANELS 8
struct MosaicPanels { const float* a[MOSAIC_MAX_PANELS]; const float* b[MOSAIC_MAX_PANELS]; int kind[MOSAIC_MAX_PANELS]; };
size_t mosaic_work_bytes(int rows, int cols);
void launch_mosaic(int H, int W, int rows, int cols, const MosaicPanels& panels, const uint8_t* lut, int quant, int bgr, void* work, uint8_t* out,
                   hipStream_t s);

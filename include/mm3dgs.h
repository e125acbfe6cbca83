/*
 * mm3dgs.h -- C ABI of libmm3dgs_hip.so: the MI355X (gfx950) differentiable 3D-Gaussian tile rasterizer that
 * sits behind MM3DGS-SLAM's render boundary.
 *
 * What this boundary replaces in the reference (/root/reference):
 *   - the un-vendored CUDA extension `diff_gaussian_rasterization` (.gitmodules:1-3; imported only at
 *     slam/renderer.py:15-18).  Its Python surface -- GaussianRasterizationSettings (slam/renderer.py:125-138)
 *     and GaussianRasterizer.__call__ (slam/renderer.py:140,196-214) plus the autograd backward driven by
 *     slam/tracker.py:157 and slam/mapper.py:875 -- is rebuilt in mm3dgs_slam_amd/rasterizer.py on top of the
 *     entry points below through ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with `host_`; all buffers are caller-owned
 *     (torch allocations); the library never allocates device memory.
 *   - float32 everywhere, row-major; matrices use the reference's row-vector convention
 *     (p_view = [p,1] * viewmatrix, slam/renderer.py:117-124).
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); no entry point synchronises the
 *     host.  A caller that wants an exactly-sized binning buffer runs stage 1, waits for `host_num_rendered`
 *     itself, then runs stage 2 (this is what the Python shim's "exact" policy does).
 *   - return value: 0 on success, negative on error; mm3dgs_last_error() returns a thread-local message.
 */
#ifndef MM3DGS_H
#define MM3DGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM3DGS_TILE 16
#define MM3DGS_MAX_CHANNELS 6
#define MM3DGS_SPLAT_FLOATS 12 /* packed per-Gaussian screen-space record: xy, conic(3), opacity, 6 colours */

/* Per-call camera / configuration bundle == GaussianRasterizationSettings (slam/renderer.py:125-138). */
typedef struct Mm3dgsCamera {
  int32_t image_height;
  int32_t image_width;
  float tanfovx;          /* W / (2 fx), slam/renderer.py:61 */
  float tanfovy;          /* H / (2 fy), slam/renderer.py:62 */
  float scale_modifier;
  int32_t sh_degree;      /* active degree, 0..3 */
  int32_t prefiltered;
  int32_t debug;
  const float* bg;         /* [3]   background, added as T_final * bg (slam/renderer.py:80-83,130) */
  const float* viewmatrix; /* [4,4] row-vector convention (w2c^T), or identity in transform_means_python mode */
  const float* projmatrix; /* [4,4] viewmatrix @ P^T (slam/renderer.py:121-123) */
  const float* campos;     /* [3] */
} Mm3dgsCamera;

/* Header at offset 0 of the image-state buffer; counters are written by the device. */
typedef struct Mm3dgsHeader {
  uint32_t num_rendered; /* N = sum of tiles touched (the reference lineage's `num_rendered`) */
  uint32_t overflow;     /* 1 if N exceeded the binning capacity of a call (output then incomplete).  STICKY in the fused
                            SLAM path (persistent state, MM3DGS_FWD_STATE_CLEAN): set by any forward since the host last
                            cleared it, so one read after a whole optimisation loop sees an overflow of ANY iteration.
                            While it is set the SLAM backward entry points take NO optimiser step (map Adam, pose Adam), write
                            zero gradients and leave the densification statistics alone: an overflowing forward dropped pairs
                            without writing their gradient records, so its iteration -- and every later one of the loop, until
                            the host clears the word -- is void rather than wrong */
  uint32_t max_tile_len; /* longest per-tile list (fused SLAM path: maximum since the host last cleared it) */
  uint32_t max_num_rendered; /* fused SLAM path: maximum N since the host last cleared it (capacity model) */
  /* diagnostics, only counted when the environment variable MM3DGS_STATS=1 (adds atomics; not for timing runs) */
  uint32_t fwd_wave_iters; /* (wave, splat) evaluations executed by the forward compositor  */
  uint32_t bwd_wave_iters; /* (wave, splat) evaluations that reached the gradient reduction */
  uint32_t bwd_wave_visits;/* (wave, splat) evaluations executed by the backward compositor */
  uint32_t bin_cap;        /* 0: the tile bins are packed (bin of tile t = [ranges[t], ranges[t+1])); otherwise every tile owns a
                              fixed span of bin_cap pairs starting at t * bin_cap (MM3DGS_FWD_DIRECT_BINS) and ranges[t] holds
                              its length.  Written by every forward. */
  uint32_t reserved8;         /* always 0 */
  uint32_t tile_order_tiles;  /* 0: workgroup -> tile by arithmetic; H << 16 | W: image_state holds a load-balanced workgroup -> tile table
                                 for an H x W image, written by the SLAM loop entry points from the list lengths of the last render
                                 (any permutation of the tiles renders the same image; only the speed depends on it) */
  uint32_t overflow_seen;     /* ABI 205: the value of `overflow` as the mapping-mode backward compositor of an iteration found it, i.e. after
                                 every launch of THAT iteration's forward.  The fused backward projection + next projection launch reads
                                 this copy: its second half bins the NEXT view and may raise `overflow` while workgroups of its first half
                                 are still starting -- with the copy, all of them take the same step / no-step decision */
  uint32_t mean_wave_steps;   /* ABI 207: mean list walk of a compositing wave (8x8 sub-tile) in the render the workgroup -> tile table was built from
                                 (written with the table, 0: unknown): the compositors raise the issue priority of waves whose walk is well above it */
} Mm3dgsHeader;

struct Mm3dgsLossConfig;   /* defined with mm3dgs_loss below; the SLAM loop entry points take a pointer to it */

/* ---- buffer sizing (pure host arithmetic) ------------------------------------------------------------- */
size_t mm3dgs_geom_bytes(int P);                       /* per-Gaussian screen-space state               */
size_t mm3dgs_image_bytes(int H, int W);               /* header + per-tile counters/ranges + per-pixel */
size_t mm3dgs_binning_bytes(size_t N_capacity);        /* (depth,id) keys + 4x4-block lists + block masks */
size_t mm3dgs_backward_scratch_bytes(int P, size_t N_capacity); /* per-(sub-tile,splat) gradient records + camera */

/* ---- forward ------------------------------------------------------------------------------------------
 * Channels: C = n_sh_channels + n_extra.  If `shs` != NULL the first 3 channels are SH colour evaluated at
 * cam->sh_degree with M coefficients per Gaussian ([P,M,3], slam/renderer.py:191) and `colors_precomp`
 * (may be NULL) supplies `C-3` extra channels [P,C-3]; otherwise `colors_precomp` supplies all C channels
 * [P,C] (slam/renderer.py:207-214 passes [z,1,z^2]).  C in {1..6}.  Extra channels beyond 3 use bg = 0.
 * Exactly one of (scales,rotations) / cov3D_precomp ([P,6]) must be non-NULL.
 *
 * Stage 1: project, cull, EWA-splat to 2D conics, colour, count per-tile overlaps, scan tile counts.
 *          Writes radii[P] (int32, 0 == culled) and the header (num_rendered).  If host_num_rendered is
 *          non-NULL (must be pinned host memory) N is also copied there asynchronously. */
int mm3dgs_forward_geom(const Mm3dgsCamera* cam, int P, int M, int C, const float* means3D, const float* shs,
                        const float* colors_precomp, const float* opacities, const float* scales,
                        const float* rotations, const float* cov3D_precomp, int32_t* radii, void* geom_state,
                        void* image_state, uint32_t* host_num_rendered, void* stream);

/* Stage 2: scatter (depth,id) keys into per-tile bins, sort every tile's bin in LDS, composite front to back.
 *          Writes out_color[C,H,W].  N_capacity is the number of (tile,Gaussian) pairs `binning_state` was
 *          sized for; on overflow header.overflow is set and the image is incomplete (never out of bounds). */
int mm3dgs_forward_raster(const Mm3dgsCamera* cam, int P, int C, const void* geom_state, void* image_state,
                          void* binning_state, size_t N_capacity, float* out_color, void* stream);

/* Both stages back to back, no host synchronisation (capacity-bounded binning). */
int mm3dgs_forward(const Mm3dgsCamera* cam, int P, int M, int C, const float* means3D, const float* shs,
                   const float* colors_precomp, const float* opacities, const float* scales,
                   const float* rotations, const float* cov3D_precomp, float* out_color, int32_t* radii,
                   void* geom_state, void* image_state, void* binning_state, size_t N_capacity, void* stream);

/* ---- backward -----------------------------------------------------------------------------------------
 * dL_dout [C,H,W] -> gradients of every tensor input of the forward.  Output pointers may be NULL when that
 * gradient is not wanted.  dL_dmeans2D is [P,3] with (x,y) = dL/d(ndc-scaled screen position), z = 0, which
 * is what slam/gaussian_model.py:594-598 consumes.  Camera gradients dL_dview[16], dL_dproj[16],
 * dL_dcampos[3] (row-vector layout, same as the inputs) are produced when non-NULL ("-w-pose" behaviour,
 * slam/renderer.py:115-124).  flags: see MM3DGS_BWD_*. */
#define MM3DGS_BWD_SKIP_GAUSSIAN_GRADS 1 /* tracker mode: only dL_dmeans3D / dL_dcolors_precomp / camera */

int mm3dgs_backward(const Mm3dgsCamera* cam, int P, int M, int C, const float* means3D, const float* shs,
                    const float* colors_precomp, const float* opacities, const float* scales,
                    const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                    const void* geom_state, const void* image_state, const void* binning_state,
                    size_t N_capacity, const float* dL_dout, void* backward_scratch, float* dL_dmeans3D,
                    float* dL_dmeans2D, float* dL_dshs, float* dL_dcolors_precomp, float* dL_dopacities,
                    float* dL_dscales, float* dL_drotations, float* dL_dcov3D, float* dL_dview, float* dL_dproj,
                    float* dL_dcampos, int flags, void* stream);

/* visible[P] (uint8) = z_view > 0.2 -- the lineage's markVisible. */
int mm3dgs_mark_visible(const Mm3dgsCamera* cam, int P, const float* means3D, uint8_t* visible, void* stream);

/* =====================================================================================================
 * Fused SLAM iteration (section 8f rows 1-2).
 * One projection kernel folds in the pose transform of `transform_means_python` mode (slam/renderer.py:142-153),
 * the [z,1,z^2] depth bundle (:26-43), the GaussianModel activations (slam/gaussian_model.py:108-137) and, in the
 * backward, their chain rules, the pose gradient (P -> 12 float reduction -> (dq,dt)), the densification statistics
 * (slam/mapper.py:887-899) and the pose Adam step (slam/tracker.py:233-246).  SH degrees 0-3 (Mm3dgsSlamInputs.sh_degree / sh_dir).
 * Output image has 6 channels: RGB, alpha-weighted z, silhouette, alpha-weighted z^2.
 * ===================================================================================================== */
typedef struct Mm3dgsSlamInputs {
  const float* pose;      /* [7] (qw,qx,qy,qz,tx,ty,tz) world->camera, raw                              */
  const float* xyz;       /* [P,3] GaussianModel._xyz                                                    */
  const float* f_dc;      /* [P,3] GaussianModel._features_dc ([P,1,3])                                  */
  const float* opacity;   /* [P]   logits (GaussianModel._opacity)                                       */
  const float* scaling;   /* [P,3] log-scales                                                            */
  const float* rotation;  /* [P,4] raw quaternions (w,x,y,z)                                             */
  int32_t isotropic;      /* pipeline.force_isotropic (slam/renderer.py:167-168)                         */
  int32_t world_means;    /* 0: pipeline.transform_means_python (the shipped configs): the means are moved to the camera frame, the
                             rasterizer's view matrix is the identity and the Gaussians' covariances keep their WORLD orientation
                             (slam/renderer.py:142-153,171-173); 1: transform_means_python: false (:117-124): world-frame means under
                             the full view matrix -- the covariance is rotated into the view, the pose gradient also flows through that
                             rotation, and the depth bundle takes the reference's literal z' = (w2c^T [x; 1])_z of :207-214 (the
                             transposed matrix: third COLUMN of R, no translation)                          */
  /* ABI 209 (appended): an ACTIVE spherical-harmonics degree above 0 -- a map resumed from a checkpoint starts at its maximal degree
   * (slam/gaussian_model.py:363), and slam/renderer.py:179-193 then hands the rasterizer shs = cat(f_dc, f_rest) with sh_degree = the active
   * degree and campos = 0 in the shipped mode (means pre-transformed: the viewing direction is the camera-space mean, normalised).  NULL / 0:
   * degree 0 (colour = SH_C0 f_dc + 0.5, no direction).  The direction the basis is evaluated at is chosen by sh_dir (ABI 211).     */
  const float* f_rest;    /* [P, n_rest, 3] GaussianModel._features_rest (n_rest = (max_sh_degree + 1)^2 - 1) or NULL    */
  int32_t sh_degree;      /* active degree 0..3; its (sh_degree + 1)^2 - 1 first rows of f_rest are used            */
  int32_t n_rest;         /* rows of f_rest per Gaussian                                                            */
  /* ABI 211 (appended): the source of the SH viewing direction d at sh_degree > 0 (p = R x + t the camera-space mean, c = -R^T t the camera centre):
   *   0  p / |p|              world_means = 0, the rasterizer's own SH evaluation (convert_SHs_python: false); a zero-initialised struct gets this
   *   1  x / |x|              world_means = 0 with convert_SHs_python: true -- the world mean about the ORIGIN: slam/renderer.py:179-193 takes
   *                           pc.get_xyz - camera_pos with camera_pos = 0 (the view matrix is the identity in that mode); d does not depend on the pose
   *   2  (x - c) / |x - c|    world_means = 1 (either SH flag): the world mean seen from the camera centre; the pose gradient gains the centre's terms
   * At sh_degree > 0, world_means = 1 needs sh_dir = 2 and sh_dir = 2 needs world_means = 1 (error -2 otherwise); at degree 0 the direction
   * does not enter and any value 0..2 renders the same.                                                                                           */
  int32_t sh_dir;
} Mm3dgsSlamInputs;

typedef struct Mm3dgsSlamGrads {
  float* d_xyz; float* d_f_dc; float* d_opacity; float* d_scaling; float* d_rotation; /* all or none (tracking) */
  float* max_radii2D; float* grad_accum; float* denom; /* [P] updated in place when max_radii2D != NULL          */
  float* d_f_rest;        /* ABI 209 (appended): [P, n_rest, 3] with the other d_* when Mm3dgsSlamInputs.sh_degree > 0 (rows beyond the active degree: 0) */
} Mm3dgsSlamGrads;

/* Optional: the map's Adam step applied inside the backward projection kernel (no gradient round trip through HBM, one
 * launch less).  Same formula as mm3dgs_adam / torch.optim.Adam; groups in the order xyz, f_dc, opacity, scaling, rotation.
 * When passed to mm3dgs_slam_backward the d_* outputs of Mm3dgsSlamGrads may be NULL. */
typedef struct Mm3dgsMapAdam {
  float* param[5]; float* exp_avg[5]; float* exp_avg_sq[5];
  /* hyper-parameters are doubles, exactly the Python floats torch.optim.Adam holds: the library forms 1 - beta, the bias
   * corrections and lr / (1 - beta1^step) in double and rounds ONCE to float, like torch does (1 - 0.999f in float arithmetic
   * is off by 1.3e-5 relative) */
  double lr[5]; double beta1, beta2, eps; int32_t step;
  /* optional: uint8 [P]; the gradient of a Gaussian with opt_mask == 0 is set to zero before the step (bundle adjustment optimises
   * the Gaussians seen by >= 2 window keyframes plus the new ones, slam/mapper.py:931-936; a zero gradient still decays the moments,
   * as `p.grad[~mask] = 0` followed by optimizer.step() does).  NULL: every Gaussian. */
  const uint8_t* opt_mask;
  /* ABI 209 (appended): the sixth group, f_rest [P, n_rest, 3] (lr = feature_lr / 20, slam/gaussian_model.py:143-195), stepped in the kernel when
   * Mm3dgsSlamInputs.sh_degree > 0 (rows beyond the active degree take a zero gradient: moments decay, as torch's Adam does it); NULL otherwise */
  float* rest_param; float* rest_exp_avg; float* rest_exp_avg_sq; double rest_lr;
} Mm3dgsMapAdam;

typedef struct Mm3dgsPoseAdam { /* torch.optim.Adam on (q; lr_q) and (t; lr_t); pose == NULL: no step */
  float* pose; float* m; float* v; int32_t* step; double lr_q, lr_t, beta1, beta2, eps;   /* doubles: see Mm3dgsMapAdam */
  /* optional IMU relative-pose residual added to the tracking loss (utils/loss_utils.py:20-40 rel_pose_loss, used at
   * slam/tracker.py:146-155): w_t * |t - t0|^2 + w_q * 2 acos(|normalize(q (x) conj(q0))_w|), (q0, t0) = prior_pose[7]
   * (device; the pose the optimisation started from).  NULL or both weights 0: no residual.  At q == q0 the angle term's
   * autograd gradient is NaN in the reference (acos'(1) = -inf times 0); here it is taken as 0 there. */
  const float* prior_pose; float prior_w_t, prior_w_q;
  /* ABI 206, optional: the best pose candidate of the loop (slam/tracker.py:88-91,161-181 -- the reference computes it and, by a
   * rebinding bug, discards it; this repository's `keep_best_candidate` option keeps it).  best[8] = { loss, pose[7] }, initialised by the
   * caller to { 1e20, starting pose }: after every step, if the iteration's total loss (image terms + prior; evaluated at the pose BEFORE
   * the step, as the reference compares it) is below best[0], best <- { loss, the pose AFTER the step }.  NULL: not tracked. */
  float* best;
} Mm3dgsPoseAdam;

/* The SLAM entry points (mm3dgs_slam_*) render the reference's bundle -- RGB and, as channels 3..5, the depth pass [z, 1, z^2] of
 * slam/renderer.py:207-214 -- in one pass.  The reference composites BOTH passes over cam->bg (renderer.py:80-83,196-214), so here
 * channels 3..5 receive T_final * bg[ch - 3] as well (with `white_background` the silhouette channel is 1 everywhere), and the backward
 * carries the corresponding -T_final bg . dL term.  (mm3dgs_forward with C = 6 keeps "extra channels over black", see above.) */
/* flags for mm3dgs_slam_forward */
#define MM3DGS_FWD_STATE_CLEAN 1 /* image_state's header+tile counters are already zero (the library leaves them zero
                                    after every forward), so the per-call memset is skipped: for persistent state buffers */
#define MM3DGS_FWD_DIRECT_BINS 4 /* N_capacity was sized as T x (per-tile capacity): projection and binning run as ONE launch that
                                    drops every (Gaussian, tile) pair straight into the tile's fixed span (no tile counting pass, no
                                    scan).  A tile with more pairs than N_capacity / T sets `overflow`.  Needs STATE_CLEAN and
                                    SHORT_LISTS; ignored (packed bins) otherwise, or when the map is too large for the key layout
                                    (id and slot share 32 bits: spans of up to 8191 pairs to 512 k Gaussians, 4095 at 1 M, none
                                    beyond 4 M).  The per-tile gradient
                                    records are then laid out per projection workgroup (256 Gaussians): each owns
                                    N_capacity / ceil(P / 256) of them, and one with more pairs than that sets `overflow` too. */
#define MM3DGS_FWD_SHORT_LISTS 2 /* hint: no tile list exceeds 2048 splats -> one sort launch (longer lists stay correct
                                    through the global-memory path, only slower)                                        */
#define MM3DGS_FWD_PROJECTED 16 /* mm3dgs_slam_forward / the FIRST view of mm3dgs_slam_map: projection + binning of this view were
                                    already launched by mm3dgs_slam_adam_project (direct bins only; ignored otherwise)            */
#define MM3DGS_FWD_KEEP_TILE_ORDER 8 /* mm3dgs_slam_track / mm3dgs_slam_map: do not rebuild image_state's load-balanced workgroup -> tile
                                    table at the head of this call (Mm3dgsHeader.tile_order_tiles); the table of an earlier call stays
                                    in force while it matches the image size.  For callers that enqueue ONE iteration per call (the
                                    multi-GPU window: gradients out, all-reduce, step): any valid table renders the same image, a
                                    fresher one only balances better, and rebuilding it costs a 9 us launch                 */
int mm3dgs_slam_forward(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, float* out_color /*[6,H,W]*/,
                        int32_t* radii, void* geom_state, void* image_state, void* binning_state, size_t N_capacity,
                        int flags, void* stream);
int mm3dgs_slam_backward(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, const int32_t* radii,
                         const void* geom_state, const void* image_state, const void* binning_state, size_t N_capacity,
                         const float* dL_dout /*[6,H,W]*/, void* backward_scratch, const Mm3dgsSlamGrads* grads,
                         float* dL_dpose /*[7] or NULL*/, const Mm3dgsPoseAdam* pose_adam, const Mm3dgsMapAdam* map_adam,
                         int flags /* the flags of the mm3dgs_slam_forward call whose state this is */, void* stream);

/* Visibility of the map from one pose with the projection stage alone (no binning, no compositing): radii[P] as the forward pass
 * would report them, and seen_count[i] += (radii[i] > 0) when seen_count != NULL -- what get_covisible_gaussians needs
 * (slam/mapper.py:690-716: Gaussians visible in >= 2 window keyframes).  geom_state: scratch of mm3dgs_geom_bytes(P). */
int mm3dgs_slam_visibility(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, int32_t* radii, uint32_t* seen_count_or_null,
                           void* geom_state, void* stream);

/* n_iter tracking iterations enqueued back to back from C (slam/tracker.py:94-177 with the "vigs" loss): each is
 * forward -> loss -> backward with the pose Adam step on the device; the pose buffer is updated in place. */
int mm3dgs_slam_track(int n_iter, const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, float* out_color,
                      int32_t* radii, void* geom_state, void* image_state, void* binning_state, size_t N_capacity,
                      int fwd_flags, const struct Mm3dgsLossConfig* loss_cfg, const float* gt_color,
                      const float* ref_depth_or_null, void* loss_work, float* dL_dout, float* loss4,
                      void* backward_scratch, const Mm3dgsPoseAdam* pose_adam, void* stream);

/* n_iter mapping iterations enqueued back to back from C (the loop of slam/mapper.py:803-950 between two pruning steps):
 * iteration i renders view i of the window (its pose, colour target, optional reference depth), takes the mapping loss and
 * the backward pass with the map's Adam step inside (map_adam->step = step number of iteration 0, +1 per iteration);
 * `grads_stats` (may be NULL): max_radii2D / grad_accum / denom = the densification statistics of slam/mapper.py:887-899;
 * its d_* pointers, when set, receive the parameter gradients of the LAST iteration (map_adam may then be NULL: a window
 * rank that all-reduces gradients before a common Adam step runs n_iter = 1 this way).  `in->pose` is ignored.  No host
 * synchronisation; `views` is read on the host during the call. */
typedef struct Mm3dgsMapView {
  const float* pose; const float* gt_color; const float* ref_depth_or_null;
  /* bundle adjustment (mapping.do_BA, slam/mapper.py:718-795,931-942): when set, the pose gradient of this view is reduced and
   * the Adam step of ITS pose is taken on the device (pose_adam->pose must be `pose`; per-keyframe moments and step counter). */
  const Mm3dgsPoseAdam* pose_adam_or_null;
  /* bundle adjustment with a sharded mapping window (pose gradients are summed over the ranks before a common step):
   * when set (and pose_adam_or_null is NULL), the view's pose gradient [7] = dL/d(qw, qx, qy, qz, tx, ty, tz) is written here and
   * no pose step is taken. */
  float* dpose_out_or_null;
} Mm3dgsMapView;
/* (loss4 may be NULL: the loss scalars of the call's last iteration are then not finished -- one launch less) */
int mm3dgs_slam_map(int n_iter, const Mm3dgsMapView* views, const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in,
                    float* out_color, int32_t* radii, void* geom_state, void* image_state, void* binning_state,
                    size_t N_capacity, int fwd_flags, const struct Mm3dgsLossConfig* loss_cfg, void* loss_work, float* dL_dout,
                    float* loss4, void* backward_scratch, const Mm3dgsSlamGrads* grads_stats, const Mm3dgsMapAdam* map_adam,
                    void* stream);

/* Image losses with the gradient image as output (slam/tracker.py:104-155, slam/mapper.py:836-873,
 * utils/loss_utils.py): w_l1 * mean|rgb-gt| (optionally over silhouette > sil_thr) + w_ssim * (1 - SSIM 11x11)
 * + w_pearson * (1 - rho(depth, ref)).  loss[4] = {total, l1, 1-ssim, 1-rho}.  work: mm3dgs_loss_work_bytes().
 * The `method: splatam` losses (slam/tracker.py:110-126, slam/mapper.py:836-855) add a depth term and masked sums:
 *   + w_depth_l1 * mean|ref - depth| over depth_l1_mask;  l1_sum = 1 turns both L1 means into sums over their masks
 * (tracking: l1_mask = depth_l1_mask = 3, l1_sum = 1, w_l1 = 0.5, w_depth_l1 = 1;  mapping: depth_l1_mask = 2, w_depth_l1 = 1,
 * w_l1 = 0.5 (1 - lambda), w_ssim = 0.5 lambda).  The depth-L1 and Pearson terms are exclusive (they share the partial-sum
 * columns); with w_depth_l1 != 0, loss[3] is the depth term.  The reference's NaN masks are not modelled: this renderer
 * produces no NaN.  Configurations that use the three splatam fields run the loss as its own launches (not folded into the
 * compositors). */
typedef struct Mm3dgsLossConfig {
  int32_t H, W;
  float w_l1, w_ssim, w_pearson;
  int32_t l1_mask;        /* bit0 silhouette > sil_thr, bit1 ref > 0 (0: all pixels)                     */
  int32_t pearson_mask;   /* bit0 silhouette > sil_thr, bit1 ref > 0                                     */
  int32_t pearson_invert; /* 1: min over targets -ref and 1/(ref+200) (utils/loss_utils.py:53-57)        */
  float sil_thr;
  float window[11];       /* normalised 1-D Gaussian window (sigma 1.5), as utils/loss_utils.py:95-112    */
  float w_depth_l1;       /* weight of the depth-L1 term (0: none)                                       */
  int32_t depth_l1_mask;  /* bit0 silhouette > sil_thr, bit1 ref > 0                                     */
  int32_t l1_sum;         /* 1: the colour and depth L1 terms are sums over their masks, not means       */
} Mm3dgsLossConfig;
size_t mm3dgs_loss_work_bytes(int H, int W);
int mm3dgs_loss(const Mm3dgsLossConfig* cfg, const float* out6, const float* gt_color, const float* ref_depth_or_null,
                void* work, float* dL_dout6, float* loss4, void* stream);

/* Fused Adam over up to 8 parameter groups in one launch (slam/gaussian_model.py:143-195; torch.optim.Adam formula).
 * step = 1-based step count used for the bias corrections. */
typedef struct Mm3dgsAdamGroup { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; uint64_t n; double lr; } Mm3dgsAdamGroup;
int mm3dgs_adam(const Mm3dgsAdamGroup* groups, int n_groups, int step, double beta1, double beta2, double eps, void* stream);

/* The multi-GPU mapping window's optimiser step AND the next view's projection + binning in one launch: the map's Adam step
 * (slam/mapper.py:931-948) from gradient ARRAYS -- grads->d_* as mm3dgs_slam_map wrote them out and the caller all-reduced them; the
 * statistics pointers are ignored -- with `adam` as for mm3dgs_slam_backward (opt_mask included), then, from the stepped parameters
 * still in registers, what the head of the next mm3dgs_slam_map / mm3dgs_slam_forward call would launch for the view at in->pose.
 * That call must carry MM3DGS_FWD_PROJECTED (and the same cam, P, buffers, capacity and flags).  Replaces mm3dgs_adam + the next
 * call's projection launch; same arithmetic as both.  Needs direct bins (MM3DGS_FWD_DIRECT_BINS in fwd_flags and honoured for this
 * P / capacity): returns -3 otherwise, nothing done.
 * ABI 212: in->sh_degree 1-3 is accepted.  It needs grads->d_f_rest and the rest_* group of `adam` (-2 otherwise, nothing done); every
 * one of the n_rest rows steps with rest_lr (rows beyond the active degree take a zero gradient, their moments decay), and the next
 * view's SH colour is evaluated from the stepped rows, with the direction of in->sh_dir. */
/* 1 if the SLAM entry points run with direct bins for this camera, map size, capacity and flags, 0 otherwise (pure host arithmetic:
 * what a caller of mm3dgs_slam_adam_project asks first). */
int mm3dgs_slam_direct_bins(const Mm3dgsCamera* cam, int P, size_t N_capacity, int fwd_flags);
int mm3dgs_slam_adam_project(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, const Mm3dgsSlamGrads* grads,
                             const Mm3dgsMapAdam* adam, int32_t* radii, void* geom_state, void* image_state, void* binning_state,
                             size_t N_capacity, int fwd_flags, void* stream);

/* =====================================================================================================
 * Map surgery on the device: pruning predicate, order-preserving compaction of the
 * per-Gaussian SoA state, seeding of new Gaussians.  Replaces the torch nonzero / index_select / cat machinery of
 * slam/gaussian_model.py:380-451 (prune_points, _prune_optimizer) and slam/mapper.py:409-493,644-668 (get_pointcloud +
 * initialisation of the new rows).  All asynchronous; the counts land in device words the caller reads when it chooses to.
 * ===================================================================================================== */
/* keep[i] = 0 where  sigmoid(opacity[i]) < min_opacity  ||  max_k exp(log_scales[i,k]) > max_scale  ||
 * (max_radii2D != NULL && max_radii2D[i] > max_screen_size)   (slam/gaussian_model.py:574-588), else 1; a NaN makes its clause
 * false as in torch -- the maximum propagates a NaN scale component (torch.max), so such a row is not pruned for its size;
 * *n_pruned_accum += number of zeros written (a sticky counter: never reset by the library). */
int mm3dgs_prune_mask(int P, const float* opacity_logits, const float* log_scales, const float* max_radii2D_or_null, float min_opacity,
                      float max_scale, float max_screen_size, uint8_t* keep, uint32_t* n_pruned_accum, void* stream);
/* Ranks of the kept elements of keep[0..n) in order: `work` (mm3dgs_compact_work_bytes(n)) receives the plan, *n_keep the total. */
size_t mm3dgs_compact_work_bytes(size_t n);
int mm3dgs_compact_plan(size_t n, const uint8_t* keep, void* work, uint32_t* n_keep, void* stream);
/* dst[rank(i)][0..width) = src[i][0..width) for every kept i, for up to 32 arrays in one launch (rows are `width` floats). */
typedef struct Mm3dgsCompactArray { const float* src; float* dst; int32_t width; } Mm3dgsCompactArray;
int mm3dgs_compact_rows(size_t n, const uint8_t* keep, const void* work, const Mm3dgsCompactArray* arrays, int n_arrays, void* stream);
/* One new Gaussian per kept pixel (raster order) of an RGB-D frame, written to rows row0 + rank of the output arrays:
 * xyz = back-projection through `pose` (world->camera 7-vector), log-scale log(z / ((fx+fy)/2)) on all three axes, opacity logit 0,
 * identity quaternion, f_dc = (rgb - 0.5) / C0, f_rest = 0 (n_rest coefficients), rgb = colour.  Plan from mm3dgs_compact_plan(H*W). */
typedef struct Mm3dgsSeedOutputs { float* xyz; float* f_dc; float* f_rest; float* opacity; float* scaling; float* rotation; float* rgb; } Mm3dgsSeedOutputs;
int mm3dgs_seed_gaussians(int H, int W, const float* color /*[3,H,W]*/, const float* depth /*[H,W]*/, const uint8_t* keep, const void* work,
                          const float* pose, float fx, float fy, float cx, float cy, uint32_t row0, const Mm3dgsSeedOutputs* out, int n_rest,
                          void* stream);

/* Densification (slam/gaussian_model.py:490-592: densify_and_clone :560-583, densify_and_split :490-558, densify :585-590) on the
 * device, in two calls around one 12-byte read-back.
 * mm3dgs_densify_plan: grad = grad_accum[i] / denom[i] (NaN -> 0), s = max_k exp(log_scales[i,k]); row i is
 *   split  if grad >= max_grad && s >  max_clone_scale (max_clone_scale = percent_dense * scene extent),
 *   clone  if grad >= max_grad && s <= max_clone_scale (the row stays and a copy is appended),
 *   kept   otherwise;
 * `work` (mm3dgs_densify_work_bytes(P)) receives the class bytes and three order-preserving rank plans (no atomics decide a position),
 * counts[3] (device memory) = { n_keep (rows that are not split), n_clone, n_split }. */
size_t mm3dgs_densify_work_bytes(size_t P);
int mm3dgs_densify_plan(size_t P, const float* grad_accum /*[P]*/, const float* denom /*[P]*/, const float* log_scales /*[P,3]*/, float max_grad,
                        float max_clone_scale, void* work, uint32_t* counts /*[3]*/, void* stream);
/* One per-Gaussian array of the scatter: rows of `width` floats (0 skips the group), its Adam moments (NULL: a group without state). */
typedef struct Mm3dgsDensifyGroup {
  const float* src; float* dst; const float* m_src; float* m_dst; const float* v_src; float* v_dst; int32_t width;
} Mm3dgsDensifyGroup;
/* group[] in the optimiser's order: xyz [P,3], f_dc, f_rest (any width, 0 at SH degree 0), opacity, scaling [P,3], rotation [P,4], rgb.
 * The statistics arrays (n_keep + n_clone + N n_split rows) are zero-filled; parent[dst] = source row of dst. */
typedef struct Mm3dgsDensifyState {
  Mm3dgsDensifyGroup group[7];
  float* grad_accum; float* denom; float* max_radii2D;
  int32_t* parent; /* may be NULL */
} Mm3dgsDensifyState;
/* mm3dgs_densify_rows: the densified map, rows in the reference's order after its clone, split and prune-of-parents sequence:
 *   [kept rows in order: parameters and both moments copied] [clones in order: parameters copied, moments 0]
 *   [split child k = 0 of each split row, in order] ... [child k = N-1]: xyz = R(normalize(q)) (exp(s) * z) + xyz,
 *   scaling = log(exp(s) / (0.8 N)), the rest copied, moments 0.
 * z = the stateless normals of general_utils.densify_normals: key_j = fmix32(fmix32(fmix32(seed) ^ row) ^ (8 k + j)), j = 0..5,
 * u_j = ((key_j >> 8) + 0.5) 2^-24, z_a = sqrt(-2 ln u_2a) cos(2 pi u_2a+1), row = index before densification.  The counts are the
 * plan's (read back by the caller); src and dst must not overlap. */
int mm3dgs_densify_rows(size_t P, const void* work, uint32_t n_keep, uint32_t n_clone, uint32_t n_split, int N, uint32_t seed,
                        const Mm3dgsDensifyState* state, void* stream);

/* Keyframe test (slam/mapper.py:141-216: need_new_keyframe -> get_depth_pointcloud + is_covisible): back-project the last keyframe's
 * rendered surface (depth where silhouette > 0.99, minus points that round to the world origin at 4 decimals) to the world and
 * project it into the current view.  counts[0] = points inside the image in front of the camera, counts[1] = points tested
 * (device memory, zeroed by the call); the covisibility ratio is counts[0] / max(counts[1], 1).  Poses are world->camera
 * (qw,qx,qy,qz,tx,ty,tz) on the device. */
int mm3dgs_covisibility_ratio(int H, int W, const float* depth /*[H,W]*/, const float* silhouette /*[H,W]*/, const float* keyframe_pose,
                              const float* current_pose, float fx, float fy, float cx, float cy, uint32_t* counts /*[2]*/, void* stream);

/* Constant-velocity pose prediction of the tracker (utils/pose_utils.py:203-216 propagate_const_vel, called at slam/tracker.py:200-206):
 * out = pose of (W1 W2^-1) W1 for the world->camera poses of the last two frames, all three (qw,qx,qy,qz,tx,ty,tz) on the device;
 * computed in double precision by one lane, so the frame's first tracking launch needs no pose on the host. */
int mm3dgs_propagate_const_vel(const float* pose_m1 /*[7], frame idx-1*/, const float* pose_m2 /*[7], frame idx-2*/, float* out_pose /*[7]*/,
                               void* stream);

/* IMU dead-reckoning of the tracker's start pose (utils/pose_utils.py:148-200 propagate_imu, called at slam/tracker.py:200-206): the IMU pose
 * i2w = W1^-1 c2i^-1 of frame idx-1 stepped through the n samples of the interval (frame idx-1, frame idx] -- velocity
 * (i2w2^-1 i2w1)[:3,3] / dt_cam held constant over the samples, acc = a - R(i2w)^T g, delta = [euler 'sxyz' (omega dt_imu) |
 * v dt_imu + acc dt_imu^2 / 2], i2w <- i2w delta -- and out = pose of (i2w c2i)^-1.  Poses are world->camera (qw,qx,qy,qz,tx,ty,tz); every
 * pointer is device memory; imu6 is read only (the reference subtracts gravity from the caller's rows in place) and may be NULL when
 * n == 0, which returns pose_m1 with a unit quaternion.  c2i must be rigid (the inverses are closed-form).  Computed in double precision
 * by one lane, rounded to float32 at the store; no host synchronisation.  -1: a NULL pointer; -2: n < 0, dt_cam == 0 or a non-finite
 * dt / gravity (nothing is launched). */
int mm3dgs_propagate_imu(const float* pose_m1 /*[7], frame idx-1*/, const float* pose_m2 /*[7], frame idx-2*/,
                         const float* imu6 /*[n,6]: angular velocity xyz (rad/s), linear acceleration xyz incl. gravity (m/s^2)*/, int n,
                         const float* c2i /*16 floats, row-major camera->IMU*/, double dt_cam, double dt_imu, double gx, double gy, double gz,
                         float* out_pose /*[7]*/, void* stream);

/* Least-squares alignment of a monocular depth estimate to a depth image (slam/SLAM.py:411-448 with utils/depth_utils.py:44-99):
 * fits scale * est + shift ~ 1 / depth over the valid pixels and, with out_or_null, writes out = 1 / (scale * est + shift) for EVERY
 * pixel in float32 (unfused multiply and add, correctly rounded division, the float32-rounded scale and shift).
 *   considered: with a silhouette  silhouette > sil_min && est > est_min  (strict, float32; the SLAM frame path passes 0.99f and 1e-6f);
 *               with silhouette_or_null = NULL  depth > 0  (sil_min and est_min are not read)
 *   valid:      considered && 0 < z < +inf, z = the correctly rounded float32 1.0f / depth.  NaN, zero, negative and +inf depth are invalid,
 *               and so is a depth so small that 1 / depth overflows (the host path of the Python package sums that pixel and returns NaN,
 *               as the reference does).  A NaN / inf of est at a pixel that is not considered does not reach the sums.
 * Sums in double over the valid pixels, h = est: a00 = sum h^2, a01 = sum h, n = sum 1, b0 = sum h z, b1 = sum z; det = a00 n - a01^2;
 * ok = n >= 2 && |det| > 1e-9 max(|a00 n|, 1e-300) && isfinite(det); scale = (n b0 - a01 b1) / det, shift = (a00 b1 - a01 b0) / det, each
 * rounded once to float32; not ok: scale 1, shift 0.  fit[16] (device, 8-byte aligned): scale, shift (the float32 values, widened), ok (0 / 1),
 * n, a00, a01, b0, b1, then eight zeros.  work: mm3dgs_align_depth_work_bytes(H, W) bytes of device memory, 8-byte aligned, contents irrelevant
 * before and after.  The images need no more than a float's alignment (planes of a [6,H,W] render qualify).  Two launches on `stream`, no
 * atomics, no host synchronisation; the same inputs give the same bits on every call.  -1 (nothing is launched): H <= 0, W <= 0, a NULL est,
 * depth, work or fit, or a misaligned work / fit. */
size_t mm3dgs_align_depth_work_bytes(int H, int W);
int mm3dgs_align_depth(int H, int W, const float* est /*[H,W]*/, const float* depth /*[H,W]*/, const float* silhouette_or_null /*[H,W]*/,
                       float sil_min, float est_min, void* work, double* fit /*[16], device*/, float* out_or_null /*[H,W]*/, void* stream);

/* ---- image evaluation: PSNR, SSIM and depth L1 / RMSE of one rendered frame against the recorded one, two launches ---------------------
 * The per-frame scoring of the reference's evaluation (slam/SLAM.py:197-231: utils/image_utils.py:17-19 psnr, utils/loss_utils.py:95-154 ssim)
 * plus a depth metric, as one row of sixteen doubles on the device.  image, gt: [3,H,W] float32; depth, gt_depth: [H,W] float32, both given or
 * both NULL; window: the HOST's 11 float32 taps of the SSIM window; row: [16] doubles on the device, 8-byte aligned -- it may point into a
 * larger table (table + 16 k), so a whole evaluation fills one tensor and is read back once.
 *   colour, per channel c:  sse_c = sum ((double)image - (double)gt)^2 over the H W pixels (widened first, subtracted in double);
 *                           mse_c = sse_c / (H W).
 *   SSIM, per channel c:    the map of utils/loss_utils.py:95-154 -- 2-D window = outer product of `window`, zero padding 5, C1 = 0.01^2,
 *                           C2 = 0.03^2 -- with the moments and the map in float32 (the separable strips of the mapping loss, mm3dgs_loss;
 *                           the map's quotient is one correctly rounded division); each map value is widened and summed in double: ssim_sum_c.
 *   depth:                  a pixel is valid when 0 < gt_depth < +inf, a strict float32 test: NaN, +-0, negative and +inf are invalid.
 *                           n = the number of valid pixels, l1 = sum |(double)depth - (double)gt_depth|, l2 = the sum of its square, over the
 *                           valid pixels.  A NaN of `depth` at a valid pixel propagates; at an invalid pixel `depth` does not reach the sums.
 *   row[0]     psnr        the mean over c of 20 log10(1 / sqrt(mse_c)) -- eval_utils.psnr(...).mean(); mse_c == 0 gives +inf, as torch does
 *   row[1]     ssim        (sum over c of ssim_sum_c) / (3 H W)
 *   row[2]     depth_l1    l1 / n; NaN when n == 0 or when the depth pointers are NULL
 *   row[3]     n           0 when the depth pointers are NULL
 *   row[4..6]  mse_c
 *   row[7..9]  ssim_sum_c / (H W)
 *   row[10]    depth_rmse  sqrt(l2 / n); NaN when n == 0 or when the depth pointers are NULL
 *   row[11..15] zeros
 * Against the host path of the Python package (eval_utils.image_metrics_host, float64 throughout): rows 0, 2, 3, 4..6 and 10 to the rounding of
 * another summation order in double (1e-9 relative is generous; n exactly), rows 1 and 7..9 to the distance of a float32 evaluation of the map
 * from the float64 one (tests/test_gpu_eval.py).
 * work: mm3dgs_eval_image_work_bytes(H, W) bytes of device memory, 8-byte aligned, contents irrelevant before and after.  The images need no
 * more than a float's alignment (planes of a [6,H,W] render qualify).  Two launches on `stream` -- one 256-lane workgroup per 16x16-pixel tile
 * writes a row of double partial sums into work, then one workgroup adds the rows in a fixed order and writes row[0:16] --, no atomics, no
 * arrival counter, no host synchronisation; the same inputs give the same bits on every call.  Nothing outside row[0:16] and
 * work[0:work_bytes] is written.  -1 (nothing is launched): a non-positive size or more than 2^28 pixels, a NULL image, gt, window, work or row,
 * exactly one of the two depth pointers, a work or row that is not 8-byte aligned, an image that is not 4-byte aligned.
 * mm3dgs_eval_image_work_bytes returns 0 for a shape that mm3dgs_eval_image rejects. */
size_t mm3dgs_eval_image_work_bytes(int H, int W);
int mm3dgs_eval_image(int H, int W, const float* image /*[3,H,W]*/, const float* gt /*[3,H,W]*/, const float* depth_or_null /*[H,W]*/,
                      const float* gt_depth_or_null /*[H,W]*/, const float* window /*host [11]*/, void* work, double* row /*[16], device*/,
                      void* stream);

/* ---- fused coloured point cloud: the valid pixels of one RGB-D view lifted to world points and appended to a growing cloud ---------------
 * The computational core of the reference's scripts/visualizer.py (rgbd2pcd, :69-112), one call per view; with a voxel size only the first
 * point that ever reached a voxel is kept, so the cloud of a whole run stays small and is the same on every run.
 * color [3,H,W], depth [H,W], silhouette_or_null [H,W]: float32 on the device, 4-byte aligned; pose: the 7 floats (qw qx qy qz tx ty tz) of the
 * world->camera pose on the device, the quaternion is normalised here; fx, fy, cx, cy: host doubles.
 *   valid pixel   depth > 0 && depth < +inf && (depth_max <= 0 || depth <= depth_max) && (silhouette == NULL || silhouette > sil_min), strict
 *                 float32 comparisons on the inputs: a NaN fails.
 *   position      p_c = ((u - cx) / fx z, (v - cy) / fy z, z) with the integer pixel indices u, v (no half-pixel offset: the reference's
 *                 convention and mm3dgs_seed_gaussians'), p_w = R^T (p_c - t); evaluated in double from the float32 inputs, rounded once to
 *                 float32 at the store.
 *   row           16 bytes {float x, y, z; uint32 rgba}, one 16-byte store; each channel (uint8)(min(max(c, 0), 1) * 255.0f + 0.5f) in float32,
 *                 NaN gives 0; alpha 255; red in the low byte: the bytes in memory are r g b a.
 *   rows          [cap] rows, 16-byte aligned.  counters[0] is the number of rows already there: a call appends behind them.
 *   voxel == 0    every valid pixel becomes a row, in raster order (count, scan, scatter by rank: no atomic decides a position); table ignored.
 *   voxel > 0     cell per axis = floor((double)x_f32 / voxel) of the float32 value that is stored; a point with some |cell| >= 2^20 (or a
 *                 position that is not a number) is dropped and counted as out of range; with the cells (i, j, k): key = (i + 2^20) << 42 |
 *                 (j + 2^20) << 21 | (k + 2^20).  table: `slots` (a power of two, 64 <= slots <= 2^40) pairs {uint64 key, uint64 ticket}, 16-byte aligned, all
 *                 ones when empty (mm3dgs_pointcloud_reset), open addressing from a multiplicative hash, linear probing over at most
 *                 min(128, slots) slots; a point that finds neither its key nor an empty slot there is dropped and counted as probe_fail.
 *                 ticket = (uint64)view << 32 | pixel index; the caller increases `view` from call to call, so a voxel keeps the first
 *                 point that reached it in stream order (view, then raster) and a view's rows are final when its call returns.  The rows a
 *                 call appends are its voxels' representatives in raster order: the set and the order of the rows do not depend on the order
 *                 in which the atomics of the claim land (tests/test_gpu_pointcloud.py: equal to a host first-occurrence selection, bit for
 *                 bit).  Rows that would land at or beyond cap are not written and counted as capacity_dropped.
 *   counters      uint64[8] on the device, 8-byte aligned, cumulative since mm3dgs_pointcloud_reset: [0] rows in the cloud (<= cap), [1] valid
 *                 pixels, [2] merged into a voxel that has its point, [3] out of range, [4] probe_fail, [5] capacity_dropped, [6] views, [7] 0;
 *                 [1] == [0] + [2] + [3] + [4] + [5] after every call.
 * work: mm3dgs_pointcloud_work_bytes(H, W) bytes of device memory, 8-byte aligned, contents irrelevant before and after.  Three launches on
 * `stream` without a voxel size, four with one (claim: 64-bit atomicCAS / atomicMin on the table; select + count; one-workgroup scan, which
 * also updates the counters; scatter); every loop is bounded, a full table or a full row buffer ends as a count; no host synchronisation.
 * Nothing outside rows[counters[0] : cap], the table, counters[0:8] and work[0:work_bytes] is written.
 * mm3dgs_pointcloud_reset sets the table (NULL: none) to all ones and the counters to zero.
 * -1 (nothing is launched): H or W <= 0 or more than 2^28 pixels; a NULL color, depth, pose, rows, counters or work; a voxel that is negative
 * or not finite; voxel > 0 with a NULL table or with slots not a power of two in [64, 2^40]; fx or fy zero or not finite, cx or cy not finite;
 * rows or table not 16-byte aligned, counters or work not 8-byte aligned, an image or the pose not 4-byte aligned.
 * mm3dgs_pointcloud_work_bytes returns 0 for a shape that mm3dgs_pointcloud_add_view rejects. */
size_t mm3dgs_pointcloud_work_bytes(int H, int W);
int mm3dgs_pointcloud_reset(void* table_or_null, uint64_t slots, uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_pointcloud_add_view(int H, int W, double fx, double fy, double cx, double cy, const float* pose /*[7], device*/,
                               const float* color /*[3,H,W]*/, const float* depth /*[H,W]*/, const float* silhouette_or_null /*[H,W]*/,
                               float sil_min, float depth_max, double voxel, uint32_t view, void* rows /*[cap] x 16 bytes*/, uint64_t cap,
                               void* table_or_null /*[slots] x 16 bytes*/, uint64_t slots, uint64_t* counters /*[8], device*/, void* work,
                               void* stream);

/* ---- coloured triangle mesh: posed RGB-D views fused into a truncated signed distance volume, its zero level as an indexed mesh ---------
 * What the point cloud leaves to a viewer: a surface.  The volume is the caller's, dense, x fastest, two device arrays over an nx x ny x nz
 * lattice of sample points: tsdf_w float2 [nz][ny][nx] {truncated distance T in [-1, 1], observation weight W}, 8-byte aligned, and rgb_w
 * float4 [nz][ny][nx] {running mean colour, colour weight}, 16-byte aligned.  Sample (i, j, k) sits at origin + voxel (i, j, k); origin:
 * host double[3], voxel: host double.  All zeros is the empty volume (mm3dgs_tsdf_reset: three memsets, the counters too).  Every size is at
 * least 2 and nx ny nz <= 2^30.
 *
 * mm3dgs_tsdf_integrate: one launch per view.  color, depth, silhouette_or_null, pose, fx, fy, cx, cy, sil_min, depth_max: as for
 * mm3dgs_pointcloud_add_view.  One lane owns one sample of a slice, 64 consecutive x make a wave, a workgroup walks up to 8 z slices.  Per sample, in double from the float32 inputs:
 *   camera point  p_c = R p_w + t (the quaternion is normalised here); skipped if z <= 0.
 *   pixel         u = floor(fx x / z + cx + 0.5), v likewise: pixel centres at integer coordinates, the point cloud's and
 *                 mm3dgs_seed_gaussians' convention; skipped if outside the image.
 *   valid pixel   the point cloud's test, word for word (one shared function); skipped otherwise.
 *   distance      sdf = depth - z; skipped if sdf < -trunc; s = min(1, sdf / trunc).
 *   update        T <- (T W + s) / (W + 1), W <- W + 1, rounded to float32 once at the 8-byte store; only if sdf <= trunc the colour mean
 *                 and its weight in the same way, from the pixel's float32 colour as it is (one 16-byte store).
 * A skipped sample touches no volume memory: the decision falls before the first load from the volume.  No atomic except one integer add
 * per workgroup and counter; no host synchronisation; the one loop has at most 8 rounds.  counters: uint64[8] on the device, 8-byte aligned, cumulative: [0] views, [1]
 * distance updates, [2] colour updates, the rest 0.  Nothing outside tsdf_w, rgb_w and counters[0:3] is written.
 * -1 (nothing is launched): H or W <= 0 or more than 2^28 pixels; a lattice size below 2 or more than 2^30 samples; a NULL color, depth, pose,
 * origin, tsdf_w, rgb_w or counters; voxel or trunc not finite or not positive; an origin that is not finite; fx or fy zero or not finite,
 * cx or cy not finite; rgb_w not 16-byte aligned, tsdf_w or counters not 8-byte aligned, an image or the pose not 4-byte aligned.
 *
 * mm3dgs_tsdf_mesh_plan / mm3dgs_tsdf_mesh_emit: marching tetrahedra.  Every lattice cube is cut into the six Kuhn tetrahedra, the paths
 * from corner (0,0,0) to (1,1,1) along one axis permutation each, permutations in lexicographic order (x,y,z) (x,z,y) (y,x,z) (y,z,x)
 * (z,x,y) (z,y,x); the cut is the same in every cube, so face diagonals agree between neighbours and the surface closes.
 *   known, inside a sample is known if W >= min_weight (a NaN is not) and inside if T < 0; a cube is valid if its 8 corners are known.
 *   vertex        lies on a lattice edge that leaves a sample q in one of the 7 directions d in {0,1}^3 \ {0} (d as a 3-bit number, x the
 *                 low bit).  The edge carries a vertex iff its endpoints differ in `inside` and at least one valid cube contains it.  The
 *                 vertex list is ordered by q in raster order (x fastest), then by d.
 *   position      t = T0 / (T0 - T1) of the distances at q and q + d; p = origin + voxel (q + t d); colour c0 + t (c1 - c0) of the two
 *                 endpoints' mean colours; all in double, rounded once to float32; the row and its colour bytes as in the point cloud:
 *                 16 bytes {float x, y, z; uint32 rgba}, one 16-byte store.
 *   triangles     int32[3] each; a corner's index is base[q] + popcount(mask[q] & ((1 << d) - 1)).  Ordered by cube (origin in raster order),
 *                 then by tetrahedron, then by case order; wound so that the normal points from inside to outside (towards free space).
 * plan leaves per sample {vertex base, 7-bit edge mask} and per cube its triangle base in work, and writes counters (uint64[8], device,
 * 8-byte aligned, not cumulative): [0] vertices, [1] triangles, [2:8] 0.  emit (same lattice, volume and work as the plan before it)
 * writes the rows and the triangles and counters [2] vertices written = min([0], vcap), [3] triangles written, [4] vertices dropped, [5]
 * triangles dropped: a vertex at or beyond vcap is not written; a triangle at or beyond tcap, or one that references a vertex that was not
 * written, is not written (its place, if below tcap, keeps what it held); [3] + [5] == [1].  The totals are exact while they are below
 * 2^32; triangle indices are int32.  work: mm3dgs_tsdf_mesh_work_bytes bytes of device memory, 8-byte aligned, contents irrelevant before
 * plan.  Five launches on `stream` for plan (no atomic at all: the edges are gathered from the cubes around them), two for emit (one
 * integer add per wave for counters [3] and [5]); no atomic decides a position or an index, so the same volume gives the same bytes on
 * every call; every loop is bounded; no host synchronisation.  Nothing outside work[0:work_bytes], counters[0:8], rows[0:vcap] and
 * triangles[0:tcap] is written.
 * -1 (nothing is launched): a lattice size below 2 or more than 2^30 samples; a NULL tsdf_w, work or counters (emit: also rgb_w, origin,
 * and rows or triangles with a cap above 0); a min_weight that is not a number; voxel not finite or not positive, an origin that is not
 * finite; rgb_w or rows not 16-byte aligned, tsdf_w, work or counters not 8-byte aligned, triangles not 4-byte aligned.
 * mm3dgs_tsdf_mesh_work_bytes returns 0 for a lattice the calls reject. */
int mm3dgs_tsdf_reset(int nx, int ny, int nz, void* tsdf_w, void* rgb_w, uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_tsdf_integrate(int H, int W, double fx, double fy, double cx, double cy, const float* pose /*[7], device*/,
                          const float* color /*[3,H,W]*/, const float* depth /*[H,W]*/, const float* silhouette_or_null /*[H,W]*/,
                          float sil_min, float depth_max, const double* origin /*host [3]*/, double voxel, double trunc, int nx, int ny,
                          int nz, void* tsdf_w, void* rgb_w, uint64_t* counters /*[8], device*/, void* stream);
size_t mm3dgs_tsdf_mesh_work_bytes(int nx, int ny, int nz);
int mm3dgs_tsdf_mesh_plan(int nx, int ny, int nz, const void* tsdf_w, float min_weight, void* work, uint64_t* counters /*[8], device*/,
                          void* stream);
int mm3dgs_tsdf_mesh_emit(int nx, int ny, int nz, const void* tsdf_w, const void* rgb_w, const double* origin /*host [3]*/, double voxel,
                          const void* work, void* rows /*[vcap] x 16 bytes*/, uint64_t vcap, void* triangles /*[tcap] x int32[3]*/,
                          uint64_t tcap, uint64_t* counters /*[8], device*/, void* stream);

/* ---- the same volume as voxel blocks: storage only where a depth pixel puts the truncation band --------------------------------------
 * The dense volume pays for the whole box; a surface occupies O(area / voxel^2) of its O(volume / voxel^3) samples.  Here sample (i, j, k)
 * in Z^3 (signed) sits at anchor + voxel (i, j, k), evaluated in double in exactly that form (anchor: host double[3]); storage is allocated
 * in blocks of 8 x 8 x 8 samples, block b = floor(index / 8) per axis with |b| < 2^20, named by the key (bz + 2^20) << 42 | (by + 2^20) <<
 * 21 | (bx + 2^20): ascending keys are blocks in z-major raster order; all ones is the empty key.  Two passes: every view is reserved, the
 * block set is frozen (list, the caller's sort, index), then every view is integrated; a sample outside the frozen set is never touched,
 * and every sample of a reserved block carries exactly the value the dense volume holds at that position (one shared device function).
 * All calls need trunc <= 16 voxel; max_blocks and n are 1 .. 2^21 (2^30 samples: 32-bit bases, int32 indices).
 *
 * table: mm3dgs_tsdf_blocks_table_bytes(max_blocks) bytes of device memory, 8-byte aligned, the caller's: a power of two >= 2 max_blocks
 * slots of 64-bit keys, a 32-bit rank per slot, and per-256-slot counts; 0 for a max_blocks the calls reject.
 * counters: uint64[8] on the device, cumulative since the reset: [0] views reserved, [1] valid pixels, [2] (pixel, block) pairs, [3]
 * distinct blocks claimed, [4] dropped: pairs whose probe window (128 slots) held no room plus blocks claimed beyond max_blocks, [5]
 * pixels out of range, [6] errors of the last mm3dgs_tsdf_blocks_index, [7] 0.  [4] != 0 means the block set is incomplete.
 * mm3dgs_tsdf_blocks_reset: every key empty, every rank none, the counters 0.
 * mm3dgs_tsdf_blocks_reserve: one launch per view, one lane per pixel; the only thing that decides which blocks exist.  A pixel (u, v) that
 * passes the point cloud's validity test with depth d is lifted to its world point P (the point cloud's rule, in double, not rounded); with
 *   ax = (|u - cx| trunc + (d + trunc) / 2) / |fx|,  ay = (|v - cy| trunc + (d + trunc) / 2) / |fy|,  R = sqrt(ax^2 + ay^2 + trunc^2)
 * every block from floor(floor((P - R - anchor) / voxel) / 8) to floor(ceil((P + R - anchor) / voxel) / 8) per axis is claimed (64-bit
 * atomicCAS where an agent-scope load read empty, linear probing, at most 128 probes).  A sample the integration updates through that
 * pixel with |sdf| <= trunc lies within R of P: |z - d| <= trunc, the nearest-pixel projection is at most half a pixel off, and the ray's
 * slope; floor and ceil leave a whole sample of slack.  A box that leaves |b| < 2^20 or spans more than 8 blocks on an axis skips the
 * pixel ([5]).  clip_or_null: host int[6] = the lowest and the highest block coordinate per axis a reservation may touch (mesh.bounds).
 * Nothing outside the table and the counters is written.
 * mm3dgs_tsdf_blocks_list: the table's keys into keys[0:cap] by count, scan and scatter, in slot order (unspecified: the caller sorts); a
 * key whose place is at or beyond cap is not written.  Three launches.
 * mm3dgs_tsdf_blocks_index: keys = the n sorted keys.  Writes each key's rank into its slot and neighbours int32 [n][27] (entry (dz + 1)
 * 9 + (dy + 1) 3 + (dx + 1): the rank of the block at that offset, -1 for none; entry 13 is the block itself).  Keys that are not
 * strictly ascending, an empty key or a key that is not in the table are counted in counters[6] (set by this call) and then nothing is
 * indexed: neither a rank nor a neighbour is written.  Four launches.
 * mm3dgs_tsdf_blocks_integrate: one launch per view, one workgroup per block, a wave of 64 lanes is one 8 x 8 z slice.  The pool is tsdf_w
 * float2 [n][512] and rgb_w float4 [n][512], block r = the r-th sorted key, x fastest inside a block, zeros = empty.  The per-sample rule
 * and the counters ([0] views, [1] distance updates, [2] colour updates; an array of its own, not the reservation's) are
 * mm3dgs_tsdf_integrate's.  A block whose bounding sphere lies behind the camera or projects outside the image leaves early
 * (conservatively).
 * mm3dgs_tsdf_blocks_mesh_plan / _emit: the dense rule (known / inside / valid cube, Kuhn tetrahedra, vertex on edge (q, d), case table,
 * winding) applied to the lattice that holds the pool's values in the reserved blocks and is unknown everywhere else: a cube or an edge at a
 * block face reads the neighbour block, or unknown where there is none.  Vertices by block in ascending key, then by sample in raster
 * order inside the block, then by d; triangles by block, then cube, then tetrahedron, then case.  Positions anchor + voxel (q + t d) with
 * q the global sample index, in double, rounded once.  work (mm3dgs_tsdf_blocks_mesh_work_bytes(n)), counters, caps and what is written:
 * as for mm3dgs_tsdf_mesh_plan / _emit over n 512 samples.  No atomic decides a position or an index.
 * Every loop in every kernel is bounded (128 probes, 8^3 blocks of a pixel, 27 neighbours); no host synchronisation.
 * -1 (nothing is launched): max_blocks or n of 0 or above 2^21; a NULL required pointer (silhouette and clip may be NULL; rows / triangles
 * / keys with a cap of 0); H or W <= 0 or more than 2^28 pixels; voxel or trunc not finite or not positive, trunc > 16 voxel; an anchor
 * that is not finite; fx or fy zero or not finite, cx or cy not finite; min_weight not a number; table, keys, tsdf_w, work or counters not
 * 8-byte aligned, rgb_w or rows not 16-byte aligned, an image, the pose, neighbours or triangles not 4-byte aligned. */
size_t mm3dgs_tsdf_blocks_table_bytes(uint64_t max_blocks);
int mm3dgs_tsdf_blocks_reset(void* table, uint64_t max_blocks, uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_tsdf_blocks_reserve(int H, int W, double fx, double fy, double cx, double cy, const float* pose /*[7], device*/,
                               const float* depth /*[H,W]*/, const float* silhouette_or_null /*[H,W]*/, float sil_min, float depth_max,
                               const double* anchor /*host [3]*/, double voxel, double trunc, const int* clip_or_null /*host [6]*/, void* table,
                               uint64_t max_blocks, uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_tsdf_blocks_list(void* table, uint64_t max_blocks, uint64_t* keys /*[cap], device*/, uint64_t cap, void* stream);
int mm3dgs_tsdf_blocks_index(void* table, uint64_t max_blocks, const uint64_t* keys /*[n], sorted*/, uint64_t n, int32_t* neighbours /*[n][27]*/,
                             uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_tsdf_blocks_integrate(int H, int W, double fx, double fy, double cx, double cy, const float* pose /*[7], device*/,
                                 const float* color /*[3,H,W]*/, const float* depth /*[H,W]*/, const float* silhouette_or_null /*[H,W]*/,
                                 float sil_min, float depth_max, const double* anchor /*host [3]*/, double voxel, double trunc,
                                 const uint64_t* keys /*[n], sorted*/, uint64_t n, void* tsdf_w /*[n][512] float2*/, void* rgb_w /*[n][512] float4*/,
                                 uint64_t* counters /*[8], device*/, void* stream);
size_t mm3dgs_tsdf_blocks_mesh_work_bytes(uint64_t n);
int mm3dgs_tsdf_blocks_mesh_plan(uint64_t n, const int32_t* neighbours /*[n][27]*/, const void* tsdf_w, float min_weight, void* work,
                                 uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_tsdf_blocks_mesh_emit(uint64_t n, const uint64_t* keys /*[n], sorted*/, const int32_t* neighbours /*[n][27]*/, const void* tsdf_w,
                                 const void* rgb_w, const double* anchor /*host [3]*/, double voxel, const void* work,
                                 void* rows /*[vcap] x 16 bytes*/, uint64_t vcap, void* triangles /*[tcap] x int32[3]*/, uint64_t tcap,
                                 uint64_t* counters /*[8], device*/, void* stream);

/* ---- geometry scores: exact truncated nearest-neighbour distances between two point sets, and area-uniform samples of a mesh --------
 * Host statement: mm3dgs_slam_amd/geometry.py (nn_distances_host, direction_row, sample_mesh_host).  A point set is [n] x 16 bytes
 * {float x, y, z; uint32 rgba} on the device, 16-byte aligned (the point cloud's rows); only the position is read.
 *
 * The grid.  cell index = floor((double)x / cell) - origin_cell per axis, over gx x gy x gz cells, x fastest; origin_cell: host int64[3],
 * |.| < 2^40; gx gy gz <= 2^26.  The caller takes origin_cell and the sizes from the reference set's bounding box.
 * mm3dgs_nn_grid_build: counts per cell (integer atomic adds: a count does not depend on order), the exclusive prefix over the cells
 * (per-256 block scans, then the one-workgroup 1024-wide scan), and the scatter of the positions into cell order.  Outputs: cell_start
 * uint32 [gx gy gz + 1] (cell c holds the records cell_start[c] .. cell_start[c + 1]); sorted [n_ref] x 16 bytes {float x, y, z; uint32 row
 * index}, of which the first counters[0] are written -- the order inside a cell depends on the atomics, no result of a query does;
 * counters uint64[8], not cumulative: [0] rows in the grid, [1] rows skipped for a coordinate that is not finite, [2] finite rows outside
 * the box (left out too), [3] cells, the rest 0.  work: mm3dgs_nn_grid_work_bytes bytes, 8-byte aligned, contents irrelevant before and
 * after.  Six launches on `stream`, no host synchronisation.  Nothing outside cell_start, sorted, counters[0:8] and work is written.
 *
 * mm3dgs_nn_query: one lane per query row, 256-lane workgroups; grid arguments as they were given to the build.  For a finite query q
 *   d(q) = min(max_dist, min_p |q - p|), the distance in double from the float32 coordinates: each coordinate widened, then subtracted,
 *   three squares, a sum, a square root (no fused multiply-add); rounded to float32 once, at the store to dist_out [n_q].
 *   clamped: the double distance > max_dist (an empty neighbourhood included); the stored value is (float)max_dist.
 *   within:  the stored float32 value <= (float)threshold.
 *   a query with a coordinate that is not finite stores NaN, enters no figure and is counted as skipped.
 * The search visits the cells at Chebyshev ring r = 0, 1, 2, ... around the query's own cell (which may lie outside the grid), clipped to
 * the grid, and stops after ring r when best <= r cell (every unsearched record is farther: the result is exact), after ring
 * ceil(max_dist / cell) (at most 2^20), or when no further ring touches the grid; it starts at the first ring that touches the grid.  A
 * row of cells along x is one range of records, so rings 0 and 1 are nine ranges.  Every loop is bounded by these numbers.
 * row: double[8] on the device, 8-byte aligned: [0] n scored queries, [1] mean d, [2] rms d, [3] max d, [4] within / n, [5] clamped, [6]
 * skipped, [7] 0 -- over the stored float32 values widened to double; [1:5] are 0 when n is 0.  Per workgroup one partial row in a fixed lane
 * order, then one workgroup over the partial rows in a fixed order: no float atomic, the same inputs give the same bytes on every call,
 * and dist_out does not depend on the order of the reference rows.  work: mm3dgs_nn_query_work_bytes bytes, 8-byte aligned, contents
 * irrelevant before and after.  Two launches on `stream`, no host synchronisation.  Nothing outside dist_out[0:n_q], row[0:8] and work is written.
 *
 * mm3dgs_mesh_sample_plan / mm3dgs_mesh_sample_emit: vrows [n_vertices] x 16 bytes as above (the rgba is used), triangles int32 [m][3].
 * With h(seed, t, k) = mix(mix(mix(seed ^ 0x9e3779b9) + t) + k) in uint32 arithmetic, mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 * x *= 0x846ca68b; x ^= x >> 16, and corners a, b, c widened to double (no fused multiply-add anywhere):
 *   count     A = 0.5 |(b - a) x (c - a)|; n_t = min(floor(A density + h(seed, t, 0xffffffff) 2^-32), 2^23): stochastic rounding, so the
 *             expected count is proportional to the area.  n_t = 0 and the triangle counts as degenerate when an index is outside
 *             [0, n_vertices), a corner is not finite, or A is 0 or not finite.
 *   sample j  r1 = h(seed, t, 2j) 2^-32, r2 = h(seed, t, 2j + 1) 2^-32; if r1 + r2 > 1 both become 1 - r; p = a + r1 (b - a) + r2 (c - a),
 *             rounded once to float32; rgba of the corner with the largest of the weights (1 - r1 - r2, r1, r2), lowest index on a tie
 *             (exact comparisons).  Samples are ordered by triangle, then j.
 * plan writes counters (uint64[8], device, 8-byte aligned, not cumulative): [0] samples, [1] degenerate triangles, [4] m, [6] 1 when the
 * samples exceed 2^32 - 1 (then emit writes nothing), the rest 0; it leaves the exclusive prefix of n_t in work.  emit (same mesh, density,
 * seed and work as the plan before it) runs one lane per SAMPLE -- the lane finds its triangle by binary search in the prefix, so a
 * wall-sized triangle does not serialise -- and writes rows [cap] x 16 bytes and counters [2] samples written = min([0], cap), [3] samples
 * dropped; a sample at or beyond cap is not written.  work: mm3dgs_mesh_sample_work_bytes(m) bytes, 8-byte aligned, contents irrelevant
 * before plan.  Three launches for plan, one for emit, no atomics, no host synchronisation.  Nothing outside work, counters[0:8] and
 * rows[0:cap] is written.
 *
 * -1 (nothing is launched, nothing is written): n_ref, n_q or m of 0 or above 2^30; a grid size below 1 or more than 2^26 cells; cell or
 * max_dist not finite or not positive; max_dist / cell above 2^20; a threshold that is negative or not finite; an origin_cell that is NULL
 * or beyond +-2^40; n_vertices of 0 or above 2^31 - 1; density not finite or not positive; cap above 2^31; a NULL pointer (rows only with a
 * cap above 0); a point set or sorted not 16-byte aligned, work, counters or row not 8-byte aligned, cell_start, dist_out or triangles not
 * 4-byte aligned.  The *_work_bytes functions return 0 for sizes the calls reject. */
size_t mm3dgs_nn_grid_work_bytes(uint64_t n_ref, int gx, int gy, int gz);
int mm3dgs_nn_grid_build(uint64_t n_ref, const void* rows /*[n_ref] x 16 bytes*/, double cell, const int64_t* origin_cell /*host [3]*/, int gx, int gy,
                         int gz, uint32_t* cell_start /*[gx gy gz + 1]*/, void* sorted /*[n_ref] x 16 bytes*/, uint64_t* counters /*[8], device*/,
                         void* work, void* stream);
size_t mm3dgs_nn_query_work_bytes(uint64_t n_q);
int mm3dgs_nn_query(uint64_t n_q, const void* q_rows /*[n_q] x 16 bytes*/, uint64_t n_ref, double cell, const int64_t* origin_cell /*host [3]*/, int gx,
                    int gy, int gz, const uint32_t* cell_start, const void* sorted, double max_dist, double threshold, float* dist_out /*[n_q]*/,
                    double* row /*[8], device*/, void* work, void* stream);
size_t mm3dgs_mesh_sample_work_bytes(uint64_t m);
int mm3dgs_mesh_sample_plan(uint64_t n_vertices, const void* vrows /*[n_vertices] x 16 bytes*/, uint64_t m, const int32_t* triangles /*[m][3]*/,
                            double density, uint32_t seed, void* work, uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_mesh_sample_emit(uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* triangles, double density, uint32_t seed,
                            const void* work, void* rows /*[cap] x 16 bytes*/, uint64_t cap, uint64_t* counters /*[8], device*/, void* stream);

/* ---- normals: normal consistency of two sampled meshes, and area-weighted vertex normals ------------------------------------------------
 * Host statement: mm3dgs_slam_amd/geometry.py (nn_index_host, normal_row, vertex_normals_host).  Meshes as the sampler takes them.
 *
 * The face cross product c_t = (b - a) x (c - a) from the float32 corners widened to double, no fused multiply-add, as the sampler's area
 * forms it (one device function serves all three).  A triangle is rejected when an index is outside [0, n_vertices), a corner is not finite,
 * or c.c is 0 or not finite.
 *
 * mm3dgs_nn_query_index: mm3dgs_nn_query (same arguments, same launches, same bytes in dist_out, row and work) that also writes index_out
 * uint32 [n_q], 4-byte aligned: the original reference row (the fourth word of the sorted record) of the record with the smallest double
 * squared distance, the smallest row index on an exact tie -- the stop rule leaves only strictly farther records unsearched, so the
 * lexicographic minimum over (d2, row) of the searched records is the global one, whatever the order inside a cell -- and 0xffffffff for a
 * query that is skipped or clamped.
 *
 * mm3dgs_mesh_sample_emit_tri: mm3dgs_mesh_sample_emit (same bytes in rows and counters) that also writes tri_out uint32 [cap], 4-byte
 * aligned: the triangle of every written sample.
 *
 * mm3dgs_normal_consistency: one lane per query i with its triangle tq = tri_q[i] (of mesh q), its nearest row j = index[i] and that row's
 * triangle tr = tri_r[j] (of mesh r; tri_r has n_r entries).  dot = (c_tq . c_tr) / (sqrt(c_tq . c_tq) sqrt(c_tr . c_tr)) in double,
 * clamped to [-1, 1], rounded once to float32 at the store to dot_out [n_q].  Not counted, dot_out NaN: j == 0xffffffff (no neighbour; this
 * test comes first), or j >= n_r, tq >= m_q, tr >= m_r or a rejected triangle (bad triangle) -- nothing is read for an id out of range.
 * row: double[8] on the device: [0] n counted, [1] mean |dot|, [2] mean dot, [3] min |dot|, [4] 0, [5] not counted: no neighbour, [6] not
 * counted: bad triangle, [7] 0 -- over the stored float32 values widened to double, summed in mm3dgs_nn_query's order (per workgroup one
 * partial row in a fixed lane order, one workgroup over the partial rows); [1:4] are 0 when n is 0.  No float atomic: the same bytes on
 * every call.  work: mm3dgs_normal_consistency_work_bytes(n_q) bytes, 8-byte aligned.  Two launches, no host synchronisation.  Nothing
 * outside dot_out[0:n_q], row[0:8] and work is written.
 *
 * mm3dgs_mesh_vertex_normals: normals float [n_vertices][3], area-weighted, in fixed point so that no order of arrival changes a bit.
 * Every triangle t that is not rejected has E_t, the binary exponent of max(|c_x|, |c_y|, |c_z|) as frexp returns it; E_v = max E_t over
 * the triangles with corner v (integer atomicMax); every such triangle adds llrint(ldexp(c_k, 40 - E_v)), k = x, y, z, to three int64 sums
 * S_v (64-bit integer atomicAdd: each term is below 2^40 in magnitude, so the sums are exact up to a valence of 2^22; beyond it they wrap
 * in two's complement, which is the defined behaviour); n_v = S_v / sqrt(S_v . S_v) in double from the sums converted to double, rounded
 * once to float32; (0, 0, 0) when v has no such triangle or S_v = 0.  counters uint64[8], device, not cumulative: [0] vertices, [1] vertices
 * without a normal, [2] rejected triangles, the rest 0.  work: mm3dgs_mesh_vertex_normals_work_bytes(n_vertices) bytes, 8-byte aligned,
 * contents irrelevant before and after.  Four launches (zero, exponents, sums, normals), no adjacency, no sort, no host synchronisation.
 * Nothing outside normals[0:3 n_vertices], counters[0:8] and work is written.
 *
 * -1 (nothing is launched, nothing is written): the cases of mm3dgs_nn_query / mm3dgs_mesh_sample_emit for the first two, and a NULL
 * index_out or tri_out (tri_out only with a cap above 0) or one not 4-byte aligned; n_q or n_r of 0 or above 2^30; m of 0 or above 2^30;
 * n_vertices of 0 or above 2^31 - 1; a NULL pointer; vertex rows not 16-byte aligned, row, work or counters not 8-byte aligned, any other
 * array not 4-byte aligned.  The *_work_bytes functions return 0 for sizes the calls reject. */
int mm3dgs_nn_query_index(uint64_t n_q, const void* q_rows /*[n_q] x 16 bytes*/, uint64_t n_ref, double cell, const int64_t* origin_cell /*host [3]*/,
                          int gx, int gy, int gz, const uint32_t* cell_start, const void* sorted, double max_dist, double threshold,
                          float* dist_out /*[n_q]*/, uint32_t* index_out /*[n_q]*/, double* row /*[8], device*/, void* work, void* stream);
int mm3dgs_mesh_sample_emit_tri(uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* triangles, double density, uint32_t seed,
                                const void* work, void* rows /*[cap] x 16 bytes*/, uint32_t* tri_out /*[cap]*/, uint64_t cap,
                                uint64_t* counters /*[8], device*/, void* stream);
size_t mm3dgs_normal_consistency_work_bytes(uint64_t n_q);
int mm3dgs_normal_consistency(uint64_t n_q, const uint32_t* tri_q /*[n_q]*/, const uint32_t* index /*[n_q]*/, uint64_t n_r, const uint32_t* tri_r /*[n_r]*/,
                              uint64_t n_vertices_q, const void* vrows_q, uint64_t m_q, const int32_t* triangles_q, uint64_t n_vertices_r,
                              const void* vrows_r, uint64_t m_r, const int32_t* triangles_r, float* dot_out /*[n_q]*/, double* row /*[8], device*/,
                              void* work, void* stream);
size_t mm3dgs_mesh_vertex_normals_work_bytes(uint64_t n_vertices);
int mm3dgs_mesh_vertex_normals(uint64_t n_vertices, const void* vrows /*[n_vertices] x 16 bytes*/, uint64_t m, const int32_t* triangles /*[m][3]*/,
                               float* normals /*[n_vertices][3]*/, void* work, uint64_t* counters /*[8], device*/, void* stream);

/* ---- point-to-point ICP: the estimate registered to the reference before it is scored ------------------------------------------------------
 * Host statement: mm3dgs_slam_amd/geometry.py (icp_host, move_rows_host, _horn_solve).  Source rows q_rows and the reference set behind
 * the grid (cell_start, sorted: as mm3dgs_nn_grid_build wrote them, grid arguments as they were given to it) are 16-byte rows as above.
 *
 * mm3dgs_icp_point.  state: double[16] on the device; in: [0:12] the start T = (R | t), row-major [3][4]; out: [0:12] T, [12] passes run,
 * [13] status (0 converged, 1 iters reached, 2 fewer than 3 correspondences), [14:16] 0.  Pass k = 0 .. iters, everything in double, no
 * fused multiply-add:
 *   move    every finite source row p (widened) gives p' = ((R0 p.x + R1 p.y) + R2 p.z) + t per component, rounded once to float32; its
 *           correspondence q is what mm3dgs_nn_query_index finds for the row p' with this max_dist (the same grid, rings, stop rule and
 *           lexicographic minimum over (d2, original row)); none for a clamped row or one that is not finite.
 *   sums    over the rows with a correspondence, p the ORIGINAL coordinates (a solve gives the absolute transform, nothing is composed):
 *           n, sum p [3], sum q [3], sum p_a q_b [9] (each product rounded, then added), sum d2 (the double squared distance of the
 *           search); one lane per row, per 256-lane workgroup one partial row in a fixed lane order, one workgroup over the partial rows
 *           in a fixed order (mm3dgs_nn_query's order); no float atomic: the same inputs give the same bytes on every call.
 *   figures fitness = n / finite source rows, rmse = sqrt(sum d2 / n), both 0 with n = 0: those of the T the pass started with.
 *   stop    status 0 when k > 0 and |fitness_k - fitness_{k-1}| < rel_fitness and |rmse_k - rmse_{k-1}| < rel_rmse; else status 2 when
 *           n < 3; else status 1 when k == iters.  T stays as it was: the figures of the last pass belong to the returned T.
 *   solve   otherwise Horn's closed form: S = sum p q^T - sum p sum q^T / n, the dominant eigenvector of the symmetric 4 x 4 matrix N(S)
 *           by cyclic Jacobi rotations (+ - x / sqrt only), w >= 0, normalised; R from the quaternion, t = sum q / n - R sum p / n.
 * log: double [iters + 1][16] on the device, row k: [0] 1 when pass k ran, [1] n, [2] finite source rows, [3] fitness, [4] rmse, [5:9] the
 * quaternion (w, x, y, z) of the latest solve of this call (0 before the first), [9:12] t behind this pass, [12] the status on the row of
 * the pass that stopped, the rest 0; the rows behind the stop are 0.  dist_out float [n_q] / index_out uint32 [n_q], each optional: what
 * mm3dgs_nn_query_index stores for the moved rows of the last pass that ran (they belong to the returned T).
 * work: mm3dgs_icp_work_bytes(n_q) bytes, 8-byte aligned, contents irrelevant before and after.  One zeroing launch and 2 (iters + 1)
 * launches on `stream`, no host synchronisation: the stop is a word on the device, and the launches behind it return at entry.  Nothing
 * outside state[0:16], log, dist_out[0:n_q], index_out[0:n_q] and work is written.
 *
 * mm3dgs_rows_move: rows_out [n] = rows_in [n] with every finite position moved by T (double[12] on the device, row-major [3][4]) by the
 * component rule above, rounded once; the rgba and a row that is not finite are copied.  rows_out may be rows_in.  One launch.
 *
 * -1 (nothing is launched, nothing is written): n_q, n_ref or n of 0 or above 2^30; a grid size below 1 or more than 2^26 cells; cell or
 * max_dist not finite or not positive; max_dist / cell above 2^20; iters outside 1 .. 1000; a tolerance that is negative or not a number;
 * an origin_cell that is NULL or beyond +-2^40; a NULL pointer (dist_out and index_out may be NULL); rows or sorted not 16-byte aligned;
 * state, log, work or T not 8-byte aligned; cell_start, dist_out or index_out not 4-byte aligned.  mm3dgs_icp_work_bytes returns 0 for
 * sizes the call rejects. */
size_t mm3dgs_icp_work_bytes(uint64_t n_q);
int mm3dgs_icp_point(uint64_t n_q, const void* q_rows /*[n_q] x 16 bytes*/, uint64_t n_ref, double cell, const int64_t* origin_cell /*host [3]*/, int gx,
                     int gy, int gz, const uint32_t* cell_start, const void* sorted, double max_dist, int iters, double rel_fitness, double rel_rmse,
                     double* state /*[16], device*/, double* log /*[iters + 1][16], device*/, float* dist_out /*[n_q] or NULL*/,
                     uint32_t* index_out /*[n_q] or NULL*/, void* work, void* stream);
int mm3dgs_rows_move(uint64_t n, const void* rows_in /*[n] x 16 bytes*/, const double* T /*[12], device*/, void* rows_out /*[n] x 16 bytes*/,
                     void* stream);

/* ---- visibility culling: the rows of a point set that the views of a run could have seen ------------------------------------------------
 * Host statement: mm3dgs_slam_amd/cull.py (cull_host).  rows: [n] x 16 bytes {float x, y, z; uint32 rgba} on the device, 16-byte aligned;
 * seen: uint32 [n] and counters: uint64 [8] on the device, both zeroed by the caller before the first view.
 *
 * mm3dgs_cull_mark_view: one launch per view, one lane per row.  pose: world->camera (qw,qx,qy,qz,tx,ty,tz) on the device, normalised by
 * the kernel; depth_or_null: float32 [H,W] on the device.  A row is seen by the view when, every operation in double from the widened
 * float32 inputs, no fused multiply-add, p_c[k] = R[k][0] x + R[k][1] y + R[k][2] z + t[k] summed left to right:
 *   1. its three coordinates are finite (else it is skipped: seen by no view);
 *   2. z_c > z_near (a NaN fails);  3. z_far == 0 or z_c <= z_far;
 *   4. fu = floor(fx x_c / z_c + cx + 0.5) and fv likewise lie in [0, W) x [0, H);
 *   5. with a depth image: d = depth[fv][fu] satisfies d > 0, d < inf, and d <= depth_max when depth_max > 0 (strict float32 tests, a
 *      NaN fails: a hole sees nothing), and z_c <= (double)d + eps.
 * Then seen[i] += 1 (plain load and store: each row belongs to one lane, views are ordered on the stream); a row that is not seen touches
 * neither the depth image nor seen.  counters[0] += 1 (views), counters[1] += the rows this view sees, one integer atomic per workgroup.
 * Nothing else is written.  n = 0 counts the view.
 *
 * mm3dgs_cull_select: a row is kept when it is finite and seen[i] >= min_views (min_views >= 1).  Kept rows go to out_rows in their
 * original order, index_or_null[k] (uint32) = the original row of kept row k; a kept row at or beyond cap is not written.  Per-256 counts,
 * one 1024-wide scan, a scatter by rank: no atomic decides a position, the same inputs give the same bytes on every call.  counters [2]
 * kept, [3] written = min(kept, cap), [4] dropped for lack of room, [5] skipped rows (not finite), [6] [7] 0; [0] [1] are left as they are.
 * work: mm3dgs_cull_work_bytes(n) bytes, 8-byte aligned, contents irrelevant before and after.  Nothing outside out_rows[0:written],
 * index[0:written], counters[0:8] and work is written.  n = 0 launches nothing but the counter update.  No host synchronisation.
 *
 * -1 (nothing is launched, nothing is written): H or W not positive or H W above 2^28; n above 2^30; fx, fy not finite or 0; cx, cy not
 * finite; z_near, z_far or eps negative or not finite; depth_max NaN; min_views 0; cap above 2^31; a NULL pose, counters or work; NULL
 * rows or seen with n > 0; NULL out_rows with n > 0 and cap > 0; rows or out_rows not 16-byte aligned, counters or work not 8-byte
 * aligned, seen, index, depth or pose not 4-byte aligned.  mm3dgs_cull_work_bytes returns 0 for n above 2^30. */
int mm3dgs_cull_mark_view(int H, int W, double fx, double fy, double cx, double cy, const float* pose /*[7], device*/, const float* depth_or_null /*[H,W]*/,
                          float depth_max, double z_near, double z_far, double eps, uint64_t n, const void* rows /*[n] x 16 bytes*/, uint32_t* seen /*[n]*/,
                          uint64_t* counters /*[8], device*/, void* stream);
size_t mm3dgs_cull_work_bytes(uint64_t n);
int mm3dgs_cull_select(uint64_t n, const void* rows /*[n] x 16 bytes*/, const uint32_t* seen /*[n]*/, uint32_t min_views, void* out_rows /*[cap] x 16 bytes*/,
                       uint64_t cap, uint32_t* index_or_null /*[cap]*/, void* work, uint64_t* counters /*[8], device*/, void* stream);

/* ---- mesh depth: a triangle mesh rendered to a depth image from a camera, and the comparison of two depth images -------------------------
 * Host statement: mm3dgs_slam_amd/mesh_depth.py (render_host, compare_rows_host).  vrows: [V] x 16 bytes {float x, y, z; uint32 rgba} on the
 * device, 16-byte aligned; triangles: int32 [T][3]; pose: world->camera (qw,qx,qy,qz,tx,ty,tz) on the device, normalised by the kernel;
 * counters: uint64 [8] on the device, zeroed by the caller before the first view, accumulating over the calls.
 *
 * mm3dgs_mesh_depth_render: one view.  Every operation in double from the widened float32 inputs, no fused multiply-add, in this order:
 *   corner    p_c[k] = R[k][0] x + R[k][1] y + R[k][2] z + t[k], summed left to right.
 *   triangle  first match wins: invalid -- an index outside [0, V) or a corner whose p_c has a component that is not finite; behind -- no
 *             corner has z_c > z_near; otherwise drawn.
 *   setup     with corners a, b, c: n0 = b x c, n1 = c x a, n2 = a x b, each component p q - r s (two products, one subtraction), and
 *             det = a.x n0.x + a.y n0.y + a.z n0.z, summed left to right.
 *   pixel     with integer centre (u, v): dx = (u - cx) / fx, dy = (v - cy) / fy; E_i = n_i.x dx + n_i.y dy + n_i.z and S = E0 + E1 + E2,
 *             summed left to right; inside when E0, E1, E2 >= 0 and S > 0, or E0, E1, E2 <= 0 and S < 0 (two-sided); a hit when inside and
 *             z = det / S is finite, z > z_near, and z <= z_far when z_far > 0.
 *   result    the hit with the smallest double z, on an exact tie the lowest triangle index: depth_out[v][u] = (float)z, rounded once,
 *             tri_out_or_null[v][u] = that index; no hit gives 0.0f and -1.  Every pixel of both images is written on every call.
 * A drawn triangle is binned into the 16 x 16-pixel tiles its rectangle touches -- floor(min) - 1 .. ceil(max) + 1 of the projections
 * fx x / z + cx, fy y / z + cy, clamped to the image in double, when all three z_c > 0 and the projections are finite, else the whole
 * image: only ever a superset of the hits -- with room for max_pairs (tile, triangle) pairs; the pairs beyond it are dropped and counted,
 * and the images of a call that dropped pairs are void.  The order inside a tile's list depends on the order atomics arrive in; the images
 * do not (a minimum over (z, index)), so the same inputs give the same bytes on every call.  counters: [0] += 1 (views), [1] += drawn,
 * [2] += invalid, [3] += behind triangles, [4] += pairs kept, [5] += pairs dropped, [6] += hit pixels, [7] is left as it is.
 * work: mm3dgs_mesh_depth_work_bytes(V, T, H, W, max_pairs) bytes, 8-byte aligned, contents irrelevant before and after.  Nothing outside
 * depth_out, tri_out, counters[0:7] and work is written.  V = 0 or T = 0: all zeros and -1, the view is counted.  No host synchronisation.
 *
 * mm3dgs_depth_compare: a (estimate), b (reference): float32 [H,W] on the device.  A pixel is valid in an image when d > 0 && d < inf
 * (strict float32 tests, a NaN fails).  row: double [8] on the device, 8-byte aligned -- one row of the caller's table: [0] n, the pixels
 * valid in both, [1] mean |a - b|, [2] rms, [3] max, [4] pixels valid only in b, [5] only in a, [6] in neither, [7] 0; differences in
 * double from the widened values; [1..3] are 0 when n is 0.  The sums have one fixed order: per 256 consecutive pixels a balanced binary
 * tree over the lanes, then lane t of one workgroup adds the partial rows t, t + 256, ... in order and the 256 lanes are added in order.
 * work: mm3dgs_depth_compare_work_bytes(H, W) bytes, 8-byte aligned.  Nothing outside row[0:8] and work is written.
 *
 * -1 (nothing is launched, nothing is written): H or W not positive or H W above 2^28; V or T above 2^30; max_pairs above 2^31; fx, fy
 * not finite or 0; cx, cy not finite; z_near or z_far negative or not finite; a NULL pose, depth_out, a, b, row, work or counters; NULL
 * vrows with V > 0 or triangles with T > 0; vrows not 16-byte aligned, work, counters or row not 8-byte aligned, triangles, an image or the
 * pose not 4-byte aligned.  The two _work_bytes return 0 for sizes the calls reject. */
size_t mm3dgs_mesh_depth_work_bytes(uint64_t V, uint64_t T, int H, int W, uint64_t max_pairs);
int mm3dgs_mesh_depth_render(int H, int W, double fx, double fy, double cx, double cy, const float* pose /*[7], device*/, double z_near, double z_far,
                             uint64_t V, const void* vrows /*[V] x 16 bytes*/, uint64_t T, const int32_t* triangles /*[T][3]*/, uint64_t max_pairs,
                             float* depth_out /*[H,W]*/, int32_t* tri_out_or_null /*[H,W]*/, void* work, uint64_t* counters /*[8], device*/, void* stream);
size_t mm3dgs_depth_compare_work_bytes(int H, int W);
int mm3dgs_depth_compare(int H, int W, const float* a /*[H,W]*/, const float* b /*[H,W]*/, void* work, double* row /*[8], device*/, void* stream);

/* ---- mesh cleaning: the connected components of an indexed triangle mesh, and the mesh without its small pieces ------------------------
 * Host statement: mm3dgs_slam_amd/mesh_clean.py (components_host, clean_host).  rows: [V] x 16 bytes {float x, y, z; uint32 rgba} on the
 * device, 16-byte aligned (only moved, never read as numbers); triangles: int32 [T][3], 4-byte aligned -- what mm3dgs_tsdf_mesh_emit writes.
 * The rule, in integers only:
 *   valid        a triangle whose three indices lie in [0, V).  An invalid one joins nothing, is counted nowhere but in `skipped`, and is
 *                never written.  A triangle with a repeated index is valid and counts as one triangle.
 *   connected    two vertices that a valid triangle both uses; components are the transitive closure.  This is connectivity through shared
 *                VERTICES (Open3D's cluster_connected_triangles and trimesh use shared edges: the two differ where surfaces touch in a point).
 *   label[v]     the smallest vertex index of v's component; v itself for a vertex no valid triangle uses.
 *   tri_count[r] the valid triangles whose vertices carry label r; 0 at every index that is not a label.
 *   kept         mode MM3DGS_MESH_CLEAN_SMALL: the components with tri_count >= min_triangles (min_triangles >= 1);
 *                mode MM3DGS_MESH_CLEAN_LARGEST: the one component with the greatest tri_count, on a tie the one with the smallest label;
 *                without a valid triangle nothing is kept.
 *   output       the vertices of kept components (which all have a triangle: a vertex that no valid triangle uses is dropped) in their
 *                original order, the 16 row bytes untouched; the valid triangles of kept components in their original order, re-indexed to
 *                the new vertex positions; index_or_null[k] (uint32) = the original vertex of kept vertex k.
 * counters: uint64 [8] on the device, 8-byte aligned, not cumulative, shared by the three calls:
 *   mm3dgs_mesh_components  [0] components with a triangle, [1] the largest: (tri_count << 32) | (~label & 0xffffffff), 0 without a valid
 *                           triangle, [2] skipped (invalid) triangles, [3] vertices no valid triangle uses, [4..7] 0
 *   mm3dgs_mesh_clean_plan  [4] components kept, [5] vertices kept, [6] triangles kept, [7] 0; [0..3] are READ ([1] names mode largest's
 *                           winner) and left as they are
 *   mm3dgs_mesh_clean_emit  [7] (kept triangles not written << 32) | kept vertices not written; the rest is left as it is
 *
 * mm3dgs_mesh_components writes label [V] and tri_count [V] (both uint32) and counters.  label serves as the parent array of a union-find:
 * one lane per triangle joins (a, b) and (b, c) by hooking the larger of two roots under the smaller with one compare-and-swap, and goes on
 * from the value the swap returned when it fails; a second launch replaces every parent by its root, a third adds one per valid triangle to
 * tri_count[label] (integer atomic adds: order-free), and one workgroup reduces tri_count to the counters.  Parents only ever point to lower
 * vertices of the same component, so every walk is bounded by V; a compare-and-swap fails only because another lane's succeeded; no lane
 * waits for another (no flag, no spin, no cooperative launch); the smallest vertex of a component can never be hooked, so it is the root
 * whatever the order of arrival: the same input gives the same bytes on every call.  V = 0 launches only the counter update ([2] = T);
 * T = 0 the initialisation (label[v] = v, tri_count[v] = 0) and the counter update.  Nothing outside label[0:V], tri_count[0:V] and
 * counters[0:8] is written; triangles is read only and every index is range-checked before it addresses anything.
 *
 * mm3dgs_mesh_clean_plan (label, tri_count and counters as mm3dgs_mesh_components left them; any label array with label[v] < V is safe):
 * per-256 counts of kept vertices, kept roots and kept triangles, one 1024-wide scan of each, and the remap of every vertex to its new
 * index, all into work.  mm3dgs_mesh_clean_emit (same V, T, triangles and work): kept rows to out_rows [vcap] x 16 bytes and index_or_null
 * [vcap] at their remap, kept triangles through the remap to out_triangles [tcap][3] at block prefix + rank.  A kept row at or beyond vcap
 * and a kept triangle at or beyond tcap is not written and is counted in [7]; a written triangle may then name a vertex that was not
 * written -- with caps of [5] and [6], read back after the plan, nothing is dropped.  No atomic decides a position.  work:
 * mm3dgs_mesh_clean_work_bytes(V, T) bytes, 8-byte aligned, contents irrelevant before the plan.  V = 0 or T = 0 launches only the counter
 * updates.  Four launches at most for the plan, three for emit, no host synchronisation.  Nothing outside work, counters[0:8],
 * out_rows[0:min([5], vcap)], index[0:min([5], vcap)] and out_triangles[0:min([6], tcap)] is written; rows, triangles, label and tri_count
 * are read only.
 *
 * -1 (nothing is launched, nothing is written): V or T above 2^30; a mode other than the two; min_triangles 0 in mode small; vcap or tcap
 * above 2^31; a NULL counters or work; NULL label or tri_count with V > 0, NULL rows (emit) with V > 0, NULL triangles with T > 0; NULL
 * out_rows / out_triangles with V > 0, T > 0 and a cap above 0; rows or out_rows not 16-byte aligned, counters or work not 8-byte aligned,
 * triangles, out_triangles, label, tri_count or index not 4-byte aligned.  mm3dgs_mesh_clean_work_bytes returns 0 for V or T above 2^30. */
#define MM3DGS_MESH_CLEAN_SMALL 1
#define MM3DGS_MESH_CLEAN_LARGEST 2
size_t mm3dgs_mesh_clean_work_bytes(uint64_t V, uint64_t T);
int mm3dgs_mesh_components(uint64_t V, uint64_t T, const int32_t* triangles /*[T][3]*/, uint32_t* label /*[V]*/, uint32_t* tri_count /*[V]*/,
                           uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_mesh_clean_plan(uint64_t V, uint64_t T, const int32_t* triangles /*[T][3]*/, const uint32_t* label /*[V]*/, const uint32_t* tri_count /*[V]*/,
                           int mode, uint32_t min_triangles, void* work, uint64_t* counters /*[8], device*/, void* stream);
int mm3dgs_mesh_clean_emit(uint64_t V, uint64_t T, const void* rows /*[V] x 16 bytes*/, const int32_t* triangles /*[T][3]*/, const void* work,
                           void* out_rows /*[vcap] x 16 bytes*/, uint64_t vcap, int32_t* out_triangles /*[tcap][3]*/, uint64_t tcap,
                           uint32_t* index_or_null /*[vcap]*/, uint64_t* counters /*[8], device*/, void* stream);

/* ---- frame ingest: raw sensor bytes -> the two images the SLAM loops consume, in one launch ------------------------------------------
 * rgb: uint8 interleaved [Hs,Ws,3] on the device, any byte alignment; depth_or_null: uint16 [Hs,Ws], 2-byte aligned.  out_color [3,H,W]
 * float32 in [0,1]; out_depth_or_null [H,W] float32 in metres, required iff depth is given (a colour-only call passes NULL for both).
 * With sx = (double)Ws / W, sy = (double)Hs / H:
 *   colour, per output pixel (y, x) and channel: fx = (x + 0.5) sx - 0.5 in double, x0 = floor(fx), a = fx - x0; x0 < 0: x0 = 0, a = 0;
 *     x0 >= Ws - 1: x0 = Ws - 1, a = 0; x1 = min(x0 + 1, Ws - 1); the same rule gives y0, y1, b; v = the bilinear blend of the four bytes
 *     with the weights a, b; out = (float)v / 255.0f, the correctly rounded float32 division.
 *   depth: xs = min((int)floor(x sx), Ws - 1), ys likewise, products in double; out = (float)((double)d / png_depth_scale), the double
 *     quotient rounded once to float32.  Zero stays zero.
 * This is meant to be the reference's cv2.resize on float64 input (INTER_LINEAR / INTER_NEAREST) followed by its casts; the match to cv2
 * itself is unchecked (cv2 was not available).  Against the host path of the Python package (dataset.ingest_host): depth bit-exact at
 * every shape; colour bit-exact whenever Ws / W and Hs / H are integers (a, b are 0 or 0.5: v is exact), within 1e-6 otherwise.
 * Every source index is clamped: nothing outside [Hs,Ws] is read at any ratio.  One launch on `stream`, no atomics, no host
 * synchronisation.  -1 (nothing is launched): a non-positive size or more than 2^30 pixels on either side, a NULL rgb or out_color, depth
 * without out_depth or the reverse, a png_depth_scale that is not finite and positive, a misaligned depth (2) or output (4). */
int mm3dgs_ingest_frame(int Hs, int Ws, const uint8_t* rgb /*[Hs,Ws,3]*/, const uint16_t* depth_or_null /*[Hs,Ws]*/, double png_depth_scale,
                        int H, int W, float* out_color /*[3,H,W]*/, float* out_depth_or_null /*[H,W]*/, void* stream);

/* ---- monocular depth estimate: the depth network's raw output -> the float32 estimate at frame size, in one launch -------------------
 * est: [Hs,Ws] on the device, row-major, dtype 0 float32, 1 float16 (IEEE binary16), 2 uint16; aligned to its element size.  out: [H,W]
 * float32, 4-byte aligned.  This is the last step of the reference's MiDaS.estimate_depth (utils/depth_utils.py): F.interpolate(prediction,
 * size = (H, W), mode = "bilinear", align_corners = False); the network itself is not part of this library.  Per output pixel (y, x), every
 * operation in double, each source value widened exactly:
 *   Hs == H and Ws == W: out = (float)(p[y][x] * scale) -- the value itself, no blend: a non-finite neighbour does not spread.
 *   otherwise: (x0, x1, a) and (y0, y1, b) by the colour rule of mm3dgs_ingest_frame (sx = (double)Ws / W, fx = (x + 0.5) sx - 0.5, ...);
 *     v = (1 - b) ((1 - a) p00 + a p01) + b ((1 - a) p10 + a p11), evaluated as written, no fused multiply-add; out = (float)(v * scale):
 *     one rounding to float32.
 * Non-finite source values are not special-cased: they go through these operators (0 * inf is NaN).  Against the host path of the Python
 * package (dataset.ingest_est_host), which restates the same operators in float64: bit-exact at equal sizes, within one float32 ulp of the
 * largest tap elsewhere, the same set of non-finite outputs.  Every source index is clamped: nothing outside [Hs,Ws] is read at any ratio.
 * One launch on `stream`, no atomics, no host synchronisation.  -1 (nothing is launched): a non-positive size or more than 2^30 pixels on
 * either side, a NULL est or out, a dtype outside 0..2, an est that is not aligned to its element size or an out that is not 4-byte
 * aligned, a scale that is not finite and positive. */
int mm3dgs_ingest_est(int Hs, int Ws, const void* est /*[Hs,Ws]*/, int dtype /*0 float32, 1 float16, 2 uint16*/, double scale, int H, int W,
                      float* out /*[H,W]*/, void* stream);

/* ---- debug mosaic: rows x cols panels of H x W float32 images -> one interleaved uint8 image, two launches ------------------------------
 * The frame of the reference's debug video (slam/SLAM.py:233-276: 2 x 3, colour | render | |render - colour| over three coloured depth images)
 * and of SLAM.render() (:148-195: an image over its coloured depth) composed on the device; only the finished bytes go to the host.
 * kind, a, b: HOST arrays of rows * cols entries, panel (r, c) at index r * cols + c; a[p], b[p] are device pointers, 4-byte aligned (planes
 * of a [6,H,W] render qualify).  rows * cols <= 8.  Panel (r, c) fills out[r H : (r+1) H, c W : (c+1) W, :]; out is uint8 [rows H, cols W, 3],
 * any byte alignment.  Per pixel (y, x) and channel ch of a panel:
 *   kind 0, colour: a is [3,H,W]; v = a[ch,y,x]; byte = Q(v).
 *   kind 1, absolute difference: a, b are [3,H,W]; v = fabsf(a[ch,y,x] - b[ch,y,x]), one float32 subtraction; byte = Q(v).
 *   kind 2, depth colour map: a is [H,W]; lo, hi = the minimum and maximum over all H W values, both NaN if any value is NaN (torch.min /
 *     torch.max); t = (a[y,x] - lo) / (hi - lo) with float32 operators and the correctly rounded IEEE division; t < 0 -> 0, t > 1 -> 1, a
 *     NaN stays NaN; byte = lut[min((int)(t * 256), 255)][ch] (matplotlib's table lookup), and a NaN t gives 0 in all three channels
 *     (matplotlib's "bad" colour).  Hence a panel that holds a NaN, or whose values are all equal (hi == lo: 0 / 0), is (0, 0, 0) throughout;
 *     the other panels are not affected.  b[p] is ignored.
 *   lut: device uint8 [256,3], RGB, already quantised by the caller with the rule Q it wants for the table's float64 entries.
 *   Q, the quantiser of kinds 0 and 1: p = (double)v * 255, exact (a float32 times 255 has at most 32 significant bits).
 *     quant 0: NaN or p < 0 -> 0; p >= 255 -> 255; otherwise (uint8)trunc(p).  On [0,1] this is the reference's (vid_image * 255).to(torch.uint8)
 *              on the float64 tensor its torch.cat produces; outside [0,1] the reference is undefined and this library saturates.
 *     quant 1: NaN -> 0; otherwise (uint8)trunc(min(max(p + 0.5, 0), 255)), the sum rounded once in double: torchvision.utils.save_image's
 *              mul(255).add_(0.5).clamp_(0, 255) on float64.
 *   bgr != 0 swaps the first and the third output byte of every pixel (what the reference hands its video writer); kind 2 included.
 * Against the host path of the Python package (debug_frames.compose_host): the same bytes, every one.
 * work: mm3dgs_mosaic_work_bytes(H, W, rows, cols) bytes of device memory, 8-byte aligned, contents irrelevant before and after.  Two
 * launches on `stream` -- per-panel partial (min, max, NaN flag) records into work, then compose; the first only when a kind-2 panel is
 * present --, no atomics, no host synchronisation; min and max are exact in any order, so the same inputs give the same bytes on every call.
 * Nothing outside out[0 : rows H cols W 3] is written.  -1 (nothing is launched): a non-positive size, more than 8 panels or more than 2^28
 * pixels in all, a NULL kind or a, a kind outside 0..2, a NULL a[p], a NULL b or b[p] for kind 1, a NULL lut with a kind-2 panel present, a
 * quant other than 0 / 1, NULL work / out, a work that is not 8-byte or an image that is not 4-byte aligned.  mm3dgs_mosaic_work_bytes
 * returns 0 for a shape that mm3dgs_mosaic rejects. */
size_t mm3dgs_mosaic_work_bytes(int H, int W, int rows, int cols);
int mm3dgs_mosaic(int H, int W, int rows, int cols, const int32_t* kind /*host [rows*cols]*/, const float* const* a /*host [rows*cols], device pointers*/,
                  const float* const* b /*host [rows*cols], device pointers or NULL entries*/, const uint8_t* lut /*device [256,3]*/,
                  int quant /*0 truncate, 1 round*/, int bgr, void* work, uint8_t* out /*[rows*H, cols*W, 3]*/, void* stream);

/* ---- optional per-kernel timing (HIP events recorded on the caller's stream around each launch) ------------
 * Used by bench.py's roofline leg.  mm3dgs_profile_read() waits for the recorded events, returns the number of
 * (timed) launches and their summed duration since the previous read, and resets the counters. */
#define MM3DGS_PROF_PREPROCESS_FWD 0
#define MM3DGS_PROF_SCAN 1
#define MM3DGS_PROF_BIN_SORT 2
#define MM3DGS_PROF_COMPOSITE_FWD 3
#define MM3DGS_PROF_COMPOSITE_BWD 4
#define MM3DGS_PROF_PREPROCESS_BWD 5
#define MM3DGS_PROF_LOSS 6
#define MM3DGS_PROF_ADAM 7
#define MM3DGS_PROF_COMPOSITE_BWD_TRACK 8 /* the tracking-mode backward compositor of the fused SLAM path (COMPOSITE_BWD: every other form) */
#define MM3DGS_PROF_TRACK_FWD_BWD 9 /* sort + forward + backward compositing of a tracking iteration in one launch */
#define MM3DGS_PROF_KERNELS 10
void mm3dgs_profile_enable(int mode); /* 0 off, 1 every kernel, 2 every 64th launch of the forward (sort +) compositor and of the backward compositors only */
int mm3dgs_profile_read(int kernel, uint64_t* launches, double* total_ms);
/* what the event pair adds to an interval it brackets (measured on empty kernels: 2 T(1 launch) - T(2 launches)); synchronises the stream */
double mm3dgs_profile_event_overhead_ms(void* stream);

/* ---- Environment (developer switches) ------------------------------------------------------------------------
 * The library reads these variables; none is needed in production, all default to "off" / the value given.  They select an alternative
 * path that the tests hold equal to the default one (bit for bit where noted) or parametrise an A/B experiment.  The first SLAM entry
 * point of a process prints one line to stderr for every one that is set.
 *   MM3DGS_NO_DIRECT_BINS=1    packed bins (count, scan, scatter) instead of direct bins in the SLAM entry points          (bit-identical)
 *   MM3DGS_NO_FUSED_SORT=1     the per-tile sort as launches of its own instead of inside the forward compositor
 *   MM3DGS_NO_FUSED_SCAN=1     a separate scan_tiles launch on the packed path (also disables direct bins)
 *   MM3DGS_NO_FUSED_TRACK=1    mm3dgs_slam_track: forward and backward compositor as two launches                            (bit-identical)
 *   MM3DGS_NO_FOLDED_LOSS=1    the loss kernels as launches of their own instead of folded into the compositors
 *   MM3DGS_NO_FORWARD_ROWS=1   mm3dgs_slam_map: the standalone mm3dgs_loss instead of the forward compositor's row sums
 *   MM3DGS_NO_FUSED_PROJECT=1  mm3dgs_slam_map: backward projection and next projection as two launches                       (bit-identical)
 *   MM3DGS_NO_POSE_CHAIN=1     mm3dgs_slam_track: gradient records + backward projection instead of the compositor's pose chain (ABI 208)
 *   MM3DGS_NO_TILE_ORDER=1     arithmetic workgroup -> tile map instead of the load-balanced table                           (bit-identical)
 *   MM3DGS_TILEMAP=0           workgroup b composites tile b (default 1: a contiguous span of tiles per XCD)                 (bit-identical)
 *   MM3DGS_DIRECT_MAX_TILES=n  largest tile grid that may use direct bins (default 11264)
 *   MM3DGS_STATS=1             count compositor wave steps into Mm3dgsHeader (adds atomics: not for timing)
 *   MM3DGS_SLAM_LDS_PAD / MM3DGS_FWD_LDS_PAD / MM3DGS_BWD_LDS_PAD=bytes   never-touched dynamic LDS per workgroup (occupancy experiments)
 * Read by the Python package, not the library: MM3DGS_LIB=<path> loads a variant build of the library (tools/build_variant.sh).
 * MM3DGS_EXP (timing probes with a phase removed: INVALID results) exists only in a library built with -DMM3DGS_PROBES. */
const char* mm3dgs_last_error(void);
/* ABI version of the library = the version of this header (tests/test_cabi.py holds the two together).
   100: round 1 | 200: double optimiser hyper-parameters, flags in mm3dgs_slam_backward, direct bins, map surgery entry points
   201: Mm3dgsLossConfig grew by the three splatam fields | 202: mm3dgs_propagate_const_vel, per-tile gradient records (binning / scratch sizes grew)
   203: Mm3dgsMapView.dpose_out_or_null, header.tile_order_tiles = image-size key, overflowing iterations are void
   204: mm3dgs_slam_adam_project, MM3DGS_FWD_PROJECTED / MM3DGS_FWD_KEEP_TILE_ORDER
   205: Mm3dgsHeader.overflow_seen (appended) | 206: Mm3dgsPoseAdam.best (appended) | 207: Mm3dgsHeader.mean_wave_steps (appended)
   208: mm3dgs_geom_bytes grew by the per-Gaussian pose-chain record (80 B; mm3dgs_slam_track's compositor applies it and writes no gradient
        records); the SLAM modes' block records are addressed by list position and the sorted bin (mask | per-tile record) overwrites the keys:
        binning_state / backward_scratch keep their sizes, their interior layout is the library's own; image_state must be zero-initialised
        to at least sizeof(Mm3dgsHeader) before its first use with MM3DGS_FWD_STATE_CLEAN
   209: Mm3dgsSlamInputs.f_rest / sh_degree / n_rest, Mm3dgsSlamGrads.d_f_rest, Mm3dgsMapAdam.rest_* (all appended): native loops at an active SH degree > 0
   210: mm3dgs_densify_work_bytes / mm3dgs_densify_plan / mm3dgs_densify_rows, Mm3dgsDensifyGroup / Mm3dgsDensifyState (densification)
   211: Mm3dgsSlamInputs.sh_dir (appended): native loops at an active SH degree > 0 with the world-origin (convert_SHs_python) and camera-centre
        (world_means = 1) viewing directions
   212: mm3dgs_slam_adam_project accepts an active SH degree 1-3 (needs Mm3dgsSlamGrads.d_f_rest and Mm3dgsMapAdam.rest_*; no struct changes):
        the multi-GPU mapping window runs natively at an active SH degree
   213: mm3dgs_propagate_imu (the tracker's IMU pose prediction on the device; no struct changes)
        later, without a new number (purely additive: no struct, signature or size of 213 changes, and tests/test_imu_predict.py holds the
        library at exactly 213): mm3dgs_align_depth_work_bytes / mm3dgs_align_depth (the monocular depth estimate's least-squares fit to
        the map, its fit record and its application on the device); mm3dgs_ingest_frame (raw uint8 RGB + uint16 depth -> the float32 frame,
        one launch); mm3dgs_ingest_est (the monocular depth network's raw output, float32 / float16 / uint16 at any size -> the float32
        estimate at frame size, one launch); mm3dgs_mosaic_work_bytes / mm3dgs_mosaic (the debug video's and SLAM.render()'s panel
        mosaic as one uint8 image, composed on the device); mm3dgs_eval_image_work_bytes / mm3dgs_eval_image (PSNR, SSIM and depth L1 of a
        rendered frame as one row of a device table); mm3dgs_pointcloud_work_bytes / mm3dgs_pointcloud_reset / mm3dgs_pointcloud_add_view
        (the fused coloured point cloud of a run, one call per view, first point per voxel); mm3dgs_tsdf_reset / mm3dgs_tsdf_integrate /
        mm3dgs_tsdf_mesh_work_bytes / mm3dgs_tsdf_mesh_plan / mm3dgs_tsdf_mesh_emit (the run as a coloured triangle mesh: views fused into
        a truncated signed distance volume, marching tetrahedra over it); mm3dgs_nn_grid_work_bytes / mm3dgs_nn_grid_build /
        mm3dgs_nn_query_work_bytes / mm3dgs_nn_query / mm3dgs_mesh_sample_work_bytes / mm3dgs_mesh_sample_plan / mm3dgs_mesh_sample_emit
        (geometry scores of an export against a reference: exact truncated nearest-neighbour distances through a uniform grid, and
        area-uniform samples of a triangle mesh); mm3dgs_cull_mark_view / mm3dgs_cull_work_bytes / mm3dgs_cull_select (the rows of a
        point set that the views of a run could have seen, for the geometry scores); mm3dgs_mesh_clean_work_bytes / mm3dgs_mesh_components /
        mm3dgs_mesh_clean_plan / mm3dgs_mesh_clean_emit (the connected components of a triangle mesh and the mesh without its small
        pieces); mm3dgs_mesh_depth_work_bytes / mm3dgs_mesh_depth_render / mm3dgs_depth_compare_work_bytes / mm3dgs_depth_compare (a
        triangle mesh rendered to a depth image from a camera, and the depth L1 of two such images); mm3dgs_tsdf_blocks_table_bytes /
        mm3dgs_tsdf_blocks_reset / _reserve / _list / _index / _integrate / mm3dgs_tsdf_blocks_mesh_work_bytes / _mesh_plan / _mesh_emit
        (the mesh export's volume as hashed 8 x 8 x 8 voxel blocks, mesh.volume: sparse); mm3dgs_nn_query_index /
        mm3dgs_mesh_sample_emit_tri / mm3dgs_normal_consistency_work_bytes / mm3dgs_normal_consistency /
        mm3dgs_mesh_vertex_normals_work_bytes / mm3dgs_mesh_vertex_normals (normal consistency for the geometry scores, vertex normals
        for mesh.ply); mm3dgs_icp_work_bytes / mm3dgs_icp_point / mm3dgs_rows_move (point-to-point ICP of the estimate onto the reference
        for the geometry scores); a caller that needs them looks the symbols up */
#define MM3DGS_ABI_VERSION 213
int mm3dgs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MM3DGS_H */

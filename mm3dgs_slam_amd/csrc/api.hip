// C-ABI entry points of libmm3dgs_hip.so (declared in include/mm3dgs.h).  Plain pointers and sizes only; every
// launch goes to the caller's stream; no device allocation, no host synchronisation.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "mm3dgs_common.h"
#include <algorithm>
#include "fused_api.h"

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
static int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(-10, "%s: %s", what, hipGetErrorString(e));
  return 0;
}

// ---- optional per-kernel timing with HIP events on the caller's stream (bench.py's roofline leg) -------------------
#include <mutex>
#include <vector>
struct KernelProfile {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending, pool;
  unsigned long long launches = 0;
  double total_ms = 0.0;
};
static KernelProfile g_prof[MM3DGS_PROF_KERNELS];
static std::mutex g_prof_mu;
static int g_prof_on = 0;
struct ProfScope {
  int k; hipStream_t s; hipEvent_t e1 = nullptr; bool on;
  // g_prof_on: 0 off, 1 every kernel, 2 only the compositors (the roofline kernels) and only every 64th launch of
  // it: an event pair around EVERY launch costs ~4 % of the SLAM frame rate (measured), a 1-in-16 sample 0.7 % (measured, round 3), 1-in-64 0.2 %
  ProfScope(int k_, hipStream_t s_) : k(k_), s(s_), on(g_prof_on == 1 || (g_prof_on == 2 && (k_ == MM3DGS_PROF_COMPOSITE_BWD || k_ == MM3DGS_PROF_COMPOSITE_BWD_TRACK ||
                                                                                     k_ == MM3DGS_PROF_COMPOSITE_FWD || k_ == MM3DGS_PROF_TRACK_FWD_BWD))) {
    if (on && g_prof_on == 2) {
      static unsigned long long sample[MM3DGS_PROF_KERNELS] = {};
      on = (sample[k_]++ & 63ull) == 0ull;
    }
    if (!on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    std::pair<hipEvent_t, hipEvent_t> ev;
    if (!g_prof[k].pool.empty()) { ev = g_prof[k].pool.back(); g_prof[k].pool.pop_back(); }
    else { (void)hipEventCreate(&ev.first); (void)hipEventCreate(&ev.second); }
    g_prof[k].pending.push_back(ev);
    e1 = ev.second;
    (void)hipEventRecord(ev.first, s);
  }
  ~ProfScope() { if (on) (void)hipEventRecord(e1, s); }
};

__global__ void profile_null_kernel() {}

// compact.hip states its two work-buffer layouts beside the kernels that read them: the launchers' pointers and, from a null base, the size
uint32_t* compact_work(const void* work, size_t n, size_t* bytes = nullptr);
uint32_t* densify_work(const void* work, size_t P, uint8_t*& cls, size_t* bytes = nullptr);

extern "C" {

void mm3dgs_profile_enable(int on) { g_prof_on = on; }
// What an event pair adds to the interval it brackets: T1 = (event, kernel, event), T2 = (event, kernel, kernel, event) with an empty
// kernel; T2 - T1 is what one more launch costs, so 2 T1 - T2 is the part of T1 that is not the launch.  Synchronises the stream.
double mm3dgs_profile_event_overhead_ms(void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return 0.0;
  double t[2] = {0.0, 0.0};
  const int reps = 32;
  for (int n = 1; n <= 2; n++) {
    for (int r = 0; r < reps + 4; r++) {
      (void)hipEventRecord(a, s);
      for (int q = 0; q < n; q++) hipLaunchKernelGGL(profile_null_kernel, dim3(1), dim3(64), 0, s);
      (void)hipEventRecord(b, s);
      (void)hipEventSynchronize(b);
      float ms = 0.f;
      if (r >= 4 && hipEventElapsedTime(&ms, a, b) == hipSuccess) t[n - 1] += ms;
    }
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  const double o = (2.0 * t[0] - t[1]) / reps;
  return o > 0.0 ? o : 0.0;
}
int mm3dgs_profile_read(int kernel, uint64_t* launches, double* total_ms) {
  if (kernel < 0 || kernel >= MM3DGS_PROF_KERNELS) return fail(-1, "bad kernel id %d", kernel);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  KernelProfile& p = g_prof[kernel];
  for (auto& ev : p.pending) {
    if (hipEventSynchronize(ev.second) == hipSuccess) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { p.total_ms += ms; p.launches++; }
    }
    p.pool.push_back(ev);
  }
  p.pending.clear();
  if (launches) *launches = p.launches;
  if (total_ms) *total_ms = p.total_ms;
  p.launches = 0; p.total_ms = 0.0;
  return 0;
}

const char* mm3dgs_last_error(void) { return g_err; }
int mm3dgs_version(void) { return MM3DGS_ABI_VERSION; }   // (history in include/mm3dgs.h)

size_t mm3dgs_geom_bytes(int P) { return geom_bytes_impl(P > 0 ? P : 1); }
size_t mm3dgs_image_bytes(int H, int W) { return image_bytes_impl(H, W); }
size_t mm3dgs_binning_bytes(size_t N) { return binning_bytes_impl(N); }
size_t mm3dgs_backward_scratch_bytes(int P, size_t N) { return bwd_bytes_impl(P, N); }

static int check_common(const Mm3dgsCamera* cam, int P, int M, int C, const float* shs, const float* colors,
                        const float* scales, const float* rots, const float* cov3d) {
  if (!cam) return fail(-1, "camera is NULL");
  if (cam->image_height <= 0 || cam->image_width <= 0) return fail(-1, "bad image size %dx%d", cam->image_height, cam->image_width);
  if (cam->image_height > 16 * 65535 || cam->image_width > 16 * 65535) return fail(-1, "image too large for 16-bit tile coordinates");
  if (P < 0) return fail(-1, "P < 0");
  if (C < 1 || C > MM3DGS_MAX_CHANNELS) return fail(-1, "C=%d outside 1..%d", C, MM3DGS_MAX_CHANNELS);
  if (P == 0) return 0;  // nothing to validate: empty tensors arrive as NULL pointers
  if (!shs && !colors) return fail(-2, "Please provide excatly one of either SHs or precomputed colors!");
  if (shs) {
    if (C < 3) return fail(-2, "SH colour needs C >= 3");
    if (C > 3 && !colors) return fail(-2, "C=%d with SHs needs %d extra precomputed channels", C, C - 3);
    if (cam->sh_degree < 0 || cam->sh_degree > 3) return fail(-2, "sh_degree %d outside 0..3", cam->sh_degree);
    if (M < (cam->sh_degree + 1) * (cam->sh_degree + 1)) return fail(-2, "M=%d too small for sh_degree %d", M, cam->sh_degree);
  }
  if ((scales == nullptr || rots == nullptr) == (cov3d == nullptr))
    return fail(-2, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
  if (!cam->bg || !cam->viewmatrix || !cam->projmatrix || !cam->campos) return fail(-1, "camera device pointers missing");
  return 0;
}

int mm3dgs_forward_geom(const Mm3dgsCamera* cam, int P, int M, int C, const float* means3D, const float* shs,
                        const float* colors_precomp, const float* opacities, const float* scales,
                        const float* rotations, const float* cov3D_precomp, int32_t* radii, void* geom_state,
                        void* image_state, uint32_t* host_num_rendered, void* stream) {
  int rc = check_common(cam, P, M, C, shs, colors_precomp, scales, rotations, cov3D_precomp);
  if (rc) return rc;
  if (!geom_state || !image_state || (P > 0 && (!means3D || !opacities || !radii))) return fail(-1, "NULL buffer");
  hipStream_t s = (hipStream_t)stream;
  CamDev cd = cam_dev(cam);
  GeomView g = geom_view(geom_state, P > 0 ? P : 1);
  ImageView iv = image_view(image_state, cd.H, cd.W);
  if (hipMemsetAsync(image_state, 0, iv.zero_bytes, s) != hipSuccess) return fail(-10, "memset failed");
  { ProfScope ps(MM3DGS_PROF_PREPROCESS_FWD, s);
    launch_preprocess_fwd(cd, P, M, C, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii, g, iv, s); }
  { ProfScope ps(MM3DGS_PROF_SCAN, s); launch_scan_tiles(cd.gx * cd.gy, P, g, iv, s); }
  if (host_num_rendered)
    if (hipMemcpyAsync(host_num_rendered, &iv.hdr->num_rendered, sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
      return fail(-10, "num_rendered copy failed");
  return check_launch("forward_geom");
}

int mm3dgs_forward_raster(const Mm3dgsCamera* cam, int P, int C, const void* geom_state, void* image_state,
                          void* binning_state, size_t N_capacity, float* out_color, void* stream) {
  if (!cam || !geom_state || !image_state || !binning_state || !out_color) return fail(-1, "NULL buffer");
  if (C < 1 || C > MM3DGS_MAX_CHANNELS) return fail(-1, "C=%d outside 1..%d", C, MM3DGS_MAX_CHANNELS);
  hipStream_t s = (hipStream_t)stream;
  CamDev cd = cam_dev(cam);
  GeomView g = geom_view((void*)geom_state, P > 0 ? P : 1);
  ImageView iv = image_view(image_state, cd.H, cd.W);
  BinView b = bin_view(binning_state, N_capacity);
  { ProfScope ps(MM3DGS_PROF_BIN_SORT, s); launch_scatter_sort(cd, P, g, iv, b, N_capacity, nullptr, s); }
  { ProfScope ps(MM3DGS_PROF_COMPOSITE_FWD, s); launch_composite_fwd(cd, C, g, iv, b, N_capacity, out_color, s); }
  return check_launch("forward_raster");
}

int mm3dgs_forward(const Mm3dgsCamera* cam, int P, int M, int C, const float* means3D, const float* shs,
                   const float* colors_precomp, const float* opacities, const float* scales,
                   const float* rotations, const float* cov3D_precomp, float* out_color, int32_t* radii,
                   void* geom_state, void* image_state, void* binning_state, size_t N_capacity, void* stream) {
  int rc = mm3dgs_forward_geom(cam, P, M, C, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                               radii, geom_state, image_state, nullptr, stream);
  if (rc) return rc;
  return mm3dgs_forward_raster(cam, P, C, geom_state, image_state, binning_state, N_capacity, out_color, stream);
}

int mm3dgs_backward(const Mm3dgsCamera* cam, int P, int M, int C, const float* means3D, const float* shs,
                    const float* colors_precomp, const float* opacities, const float* scales,
                    const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                    const void* geom_state, const void* image_state, const void* binning_state,
                    size_t N_capacity, const float* dL_dout, void* backward_scratch, float* dL_dmeans3D,
                    float* dL_dmeans2D, float* dL_dshs, float* dL_dcolors_precomp, float* dL_dopacities,
                    float* dL_dscales, float* dL_drotations, float* dL_dcov3D, float* dL_dview, float* dL_dproj,
                    float* dL_dcampos, int flags, void* stream) {
  int rc = check_common(cam, P, M, C, shs, colors_precomp, scales, rotations, cov3D_precomp);
  if (rc) return rc;
  if (!geom_state || !image_state || !binning_state || !dL_dout || !backward_scratch || (P > 0 && !radii))
    return fail(-1, "NULL buffer");
  hipStream_t s = (hipStream_t)stream;
  CamDev cd = cam_dev(cam);
  GeomView g = geom_view((void*)geom_state, P > 0 ? P : 1);
  ImageView iv = image_view((void*)image_state, cd.H, cd.W);
  BinView b = bin_view((void*)binning_state, N_capacity);
  BwdView bw = bwd_view(backward_scratch, P, N_capacity);
  { ProfScope ps(MM3DGS_PROF_COMPOSITE_BWD, s); launch_composite_bwd(cd, C, g, iv, b, N_capacity, dL_dout, bw.dsub, s); }
  ProfScope ps_pb(MM3DGS_PROF_PREPROCESS_BWD, s);
  bool want_cam = dL_dview || dL_dproj || dL_dcampos;
  launch_preprocess_bwd(cd, P, M, C, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii, g, b,
                        N_capacity, bw, dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dcolors_precomp, dL_dopacities, dL_dscales, dL_drotations,
                        dL_dcov3D, want_cam, flags, s);
  if (want_cam) launch_camgrad_finish(bw, dL_dview, dL_dproj, dL_dcampos, s);
  return check_launch("backward");
}

// ---- developer switches (environment) ---------------------------------------------------------------------------------------
// Every switch the library reads is listed in include/mm3dgs.h ("Environment").  They exist for the bit-identity / equivalence tests and for same-box
// A/Bs; one left set in a user's environment silently changes which kernels run -- so the first SLAM entry point of a process says which are set.
static void warn_env_once() {
  static const bool done = [] {
    static const char* const names[] = {"MM3DGS_NO_DIRECT_BINS", "MM3DGS_NO_FUSED_SORT", "MM3DGS_NO_FUSED_SCAN", "MM3DGS_NO_FUSED_TRACK", "MM3DGS_NO_FOLDED_LOSS",
                                        "MM3DGS_NO_FORWARD_ROWS", "MM3DGS_NO_FUSED_PROJECT", "MM3DGS_NO_TILE_ORDER", "MM3DGS_NO_POSE_CHAIN", "MM3DGS_TILEMAP",
                                        "MM3DGS_DIRECT_MAX_TILES", "MM3DGS_STATS", "MM3DGS_SLAM_LDS_PAD", "MM3DGS_FWD_LDS_PAD", "MM3DGS_BWD_LDS_PAD"};
    for (const char* n : names) {
      const char* v = getenv(n);
      if (v && *v) fprintf(stderr, "mm3dgs: developer switch %s=%s is set in the environment: it changes which kernels run (include/mm3dgs.h, \"Environment\")\n", n, v);
    }
    return true;
  }();
  (void)done;
}

// ---- fused SLAM iteration ----------------------------------------------------------------------------------------
// Every entry point below checks ALL of its arguments first and launches afterwards: a refused call has enqueued nothing.
static SlamIn slam_in(const Mm3dgsSlamInputs* in) {
  SlamIn s;
  s.pose = in->pose; s.xyz = in->xyz; s.f_dc = in->f_dc; s.opacity = in->opacity; s.scaling = in->scaling;
  s.rotation = in->rotation; s.isotropic = in->isotropic; s.world = in->world_means;
  s.sh_deg = (in->f_rest && in->sh_degree > 0) ? in->sh_degree : 0;
  s.f_rest = s.sh_deg ? in->f_rest : nullptr; s.n_rest = s.sh_deg ? in->n_rest : 0;
  s.sh_dir = s.sh_deg ? in->sh_dir : 0;
  return s;
}
// need_pose = false: the mapping loop, which renders its views' poses and ignores in->pose
static int check_slam(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, bool need_pose = true) {
  warn_env_once();
  if (!cam || !in) return fail(-1, "NULL argument");
  if (cam->image_height <= 0 || cam->image_width <= 0) return fail(-1, "bad image size");
  if (P < 0) return fail(-1, "P < 0");
  if (!cam->bg || !cam->projmatrix) return fail(-1, "camera device pointers missing");
  if (need_pose && !in->pose) return fail(-1, "pose is NULL");
  if (P > 0 && (!in->xyz || !in->f_dc || !in->opacity || !in->scaling || !in->rotation)) return fail(-1, "NULL Gaussian parameter");
  if (in->sh_degree < 0 || in->sh_degree > 3) return fail(-2, "sh_degree %d outside 0..3", in->sh_degree);
  if (in->sh_dir < 0 || in->sh_dir > 2) return fail(-2, "sh_dir %d outside 0..2", in->sh_dir);
  if (in->sh_degree > 0) {
    if (P > 0 && !in->f_rest) return fail(-2, "sh_degree %d needs the f_rest rows", in->sh_degree);
    if (in->n_rest < (in->sh_degree + 1) * (in->sh_degree + 1) - 1 || in->n_rest > 15) return fail(-2, "n_rest = %d does not hold sh_degree %d (or exceeds 15)", in->n_rest, in->sh_degree);
    // (ABI 211) the direction source must match the means' frame: world-frame means see the Gaussians from the camera centre
    if (in->world_means && in->sh_dir != 2) return fail(-2, "world_means = 1 needs sh_dir = 2 (direction from the camera centre), got sh_dir = %d", in->sh_dir);
    if (in->sh_dir == 2 && !in->world_means) return fail(-2, "sh_dir = 2 (direction from the camera centre) needs world_means = 1");
  }
  return 0;
}

static bool slam_fused_sort(int flags) {
  static const int no_fused_sort = env_flag("MM3DGS_NO_FUSED_SORT", 0);
  return (flags & MM3DGS_FWD_SHORT_LISTS) && !no_fused_sort;
}

// direct bins (MM3DGS_FWD_DIRECT_BINS): one decision for the forward and the backward of a render
struct DirectBins { bool on; uint32_t bin_cap, trec_cap; int nblocks, slot_bits; };
static DirectBins slam_direct_bins(int flags, const CamDev& cd, int P, size_t N_capacity) {
  static const int no_direct = env_flag("MM3DGS_NO_DIRECT_BINS", 0);
  static const int no_fused_scan = env_flag("MM3DGS_NO_FUSED_SCAN", 0);
  static const int max_tiles = env_flag("MM3DGS_DIRECT_MAX_TILES", 11264);   // the binning kernel keeps one LDS word per tile beside 18 KB of static LDS: 62 KB at this limit (1920x1080 = 8160 tiles, 1920x1440 = 10800)
  DirectBins d;
  const int T = cd.gx * cd.gy;
  d.nblocks = (P + 255) / 256;
  const size_t nb = (size_t)std::max(d.nblocks, 1);
  d.slot_bits = direct_slot_bits(P);
  d.bin_cap = (uint32_t)std::min<size_t>(N_capacity / (size_t)std::max(T, 1), (size_t)((1u << std::max(d.slot_bits, 1)) - 1u));
  // per-tile records (one per pair) per projection workgroup: the region holds N_capacity of them
  d.trec_cap = (uint32_t)std::min<size_t>(N_capacity / nb, 0xffffffffull / nb);
  d.on = (flags & MM3DGS_FWD_DIRECT_BINS) && (flags & MM3DGS_FWD_STATE_CLEAN) && slam_fused_sort(flags) && !no_direct && !no_fused_scan &&
         P > 0 && d.slot_bits >= DIRECT_SLOT_BITS_MIN && T <= max_tiles && T <= MAX_LDS_TILES && d.bin_cap >= 32 && d.trec_cap >= 256 &&
         N_capacity >= 4 * (size_t)P;
  return d;
}

// What the launches of one C call share, built and checked once per call (slam_call); the loops only move in.pose.
struct SlamCall {
  hipStream_t s; int P; size_t N_cap; int flags;
  CamDev cd;         // with the SLAM fields every launch sees: bg_extras, tile_table, trec_cap
  CamDev cd_fwd;     // cd + what the forward's binning launches read: sort_single, state_clean, fused_scan
  SlamIn in;         // in.pose: the view the next launch renders
  GeomView g; ImageView iv; BinView b;
  BwdView bw;        // (zero without a backward scratch)
  DirectBins db; bool fused_sort;
  float* out_color; int32_t* radii;
  bool sh() const { return in.sh_deg > 0; }   // an ACTIVE SH degree: standalone loss kernels, mapping-mode compositor, sixth Adam group
};
// what a call needs beside the three state buffers and radii: out_color | backward_scratch; SLAM_POSE_LATER: in->pose is not read (check_slam)
enum { SLAM_OUT = 1, SLAM_SCRATCH = 2, SLAM_POSE_LATER = 4 };
static int slam_call(SlamCall& c, const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, float* out_color, int32_t* radii, void* geom_state,
                     void* image_state, void* binning_state, size_t N_capacity, void* backward_scratch, int flags, void* stream, int need) {
  if (int rc = check_slam(cam, P, in, !(need & SLAM_POSE_LATER))) return rc;
  if (!geom_state || !image_state || !binning_state || (P > 0 && !radii) || ((need & SLAM_OUT) && !out_color) ||
      ((need & SLAM_SCRATCH) && !backward_scratch)) return fail(-1, "NULL buffer");
  c.s = (hipStream_t)stream; c.P = P; c.N_cap = N_capacity; c.flags = flags;
  c.in = slam_in(in);
  c.out_color = out_color; c.radii = radii;
  c.cd = cam_dev(cam);
  c.g = geom_view(geom_state, P > 0 ? P : 1);
  c.iv = image_view(image_state, c.cd.H, c.cd.W);
  c.b = bin_view(binning_state, N_capacity);
  c.bw = backward_scratch ? bwd_view(backward_scratch, P, N_capacity) : BwdView{};
  c.cd.bg_extras = 1;
  // image_state's load-balanced workgroup -> tile table (binning.hip): the compositors honour it while the header says it matches the grid
  // (persistent state only: a per-call memset clears it)
  c.cd.tile_table = ((flags & MM3DGS_FWD_STATE_CLEAN) && !env_flag("MM3DGS_NO_TILE_ORDER", 0)) ? 1 : 0;
  // short lists (the SLAM regime): the per-tile sort runs inside the forward compositing launch
  c.fused_sort = slam_fused_sort(flags);
  // direct bins: the host sized the binning state as T x (per-tile capacity), so projection and binning are one launch
  c.db = slam_direct_bins(flags, c.cd, P, N_capacity);
  c.cd.trec_cap = c.db.on ? c.db.trec_cap : 0u;
  c.cd_fwd = c.cd;
  c.cd_fwd.sort_single = (flags & MM3DGS_FWD_SHORT_LISTS) ? 1 : 0;
  c.cd_fwd.state_clean = (flags & MM3DGS_FWD_STATE_CLEAN) ? 1 : 0;
  // persistent clean state + a tile grid that fits two LDS words per tile: fold the scan into the scatter workgroups
  c.cd_fwd.fused_scan = ((flags & MM3DGS_FWD_STATE_CLEAN) && P > 0 && c.cd.gx * c.cd.gy <= MAX_FUSED_SCAN_TILES && !env_flag("MM3DGS_NO_FUSED_SCAN", 0)) ? 1 : 0;
  return 0;
}

// The SLAM loops rebuild the workgroup -> tile table once per call, from the list lengths of the last render.
static void slam_refresh_tile_order(const SlamCall& c) {
  if (!c.cd.tile_table || (c.flags & MM3DGS_FWD_KEEP_TILE_ORDER)) return;      // (a table left by an earlier call is honoured while its key matches the image size)
  launch_tile_order(c.cd.gx * c.cd.gy, c.cd.H, c.cd.W, c.iv, c.s);
}

struct SlamFwd {
  const TrackLoss* tl = nullptr;    // loss folded into the compositor's epilogue (needs the fused sort path)
  float* track_dsub = nullptr;      // tracking: the backward compositor runs in the forward launch and writes here
  bool projected = false;           // an earlier launch already projected and binned this view (slam_bwd_project / slam_adam_project; direct bins only)
  bool pose_chain = false;
};
static int slam_forward(const SlamCall& c, const SlamFwd& o) {
  const CamDev& cd = c.cd_fwd;
  const hipStream_t s = c.s;
  if (o.tl && !c.fused_sort) return fail(-1, "internal: folded tracking loss needs the fused sort path");
  if (!cd.state_clean)
    if (hipMemsetAsync(c.iv.hdr, 0, c.iv.zero_bytes, s) != hipSuccess) return fail(-10, "memset failed");
  const int prof_fwd = (c.fused_sort && o.track_dsub) ? MM3DGS_PROF_TRACK_FWD_BWD : MM3DGS_PROF_COMPOSITE_FWD;
  if (c.db.on) {
    const DirectBins& db = c.db;
    if (!o.projected) { ProfScope ps(MM3DGS_PROF_PREPROCESS_FWD, s); launch_slam_project_bin(cd, c.P, c.in, c.radii, c.g, c.iv, c.b, db.bin_cap, db.slot_bits, s, o.pose_chain); }
    { ProfScope ps(prof_fwd, s);
      if (o.track_dsub) launch_sort_composite_fwd_bwd_track(cd, c.g, c.iv, c.b, c.N_cap, c.out_color, 1, s, *o.tl, db.nblocks, o.track_dsub, db.bin_cap, db.slot_bits, o.pose_chain);
      else launch_sort_composite_fwd6(cd, c.g, c.iv, c.b, c.N_cap, c.out_color, 1, s, o.tl, db.nblocks, db.bin_cap, db.slot_bits); }
    return check_launch("slam_forward");
  }
  const int clean = (cd.fused_scan || cd.state_clean) ? 1 : 0;
  { ProfScope ps(MM3DGS_PROF_PREPROCESS_FWD, s); launch_slam_preprocess_fwd(cd, c.P, c.in, c.radii, c.g, c.iv, s, nullptr, false, o.pose_chain); }
  if (!cd.fused_scan) { ProfScope ps(MM3DGS_PROF_SCAN, s); launch_scan_tiles(cd.gx * cd.gy, c.P, c.g, c.iv, s, cd.state_clean); }
  { ProfScope ps(MM3DGS_PROF_BIN_SORT, s); launch_scatter_sort(cd, c.P, c.g, c.iv, c.b, c.N_cap, nullptr, s, c.fused_sort); }
  { ProfScope ps(prof_fwd, s);
    if (c.fused_sort && o.track_dsub) launch_sort_composite_fwd_bwd_track(cd, c.g, c.iv, c.b, c.N_cap, c.out_color, clean, s, *o.tl, 0, o.track_dsub, 0, DIRECT_SLOT_BITS_MAX, o.pose_chain);
    else if (c.fused_sort) launch_sort_composite_fwd6(cd, c.g, c.iv, c.b, c.N_cap, c.out_color, clean, s, o.tl);
    else launch_composite_fwd(cd, 6, c.g, c.iv, c.b, c.N_cap, c.out_color, s); }
  return check_launch("slam_forward");
}

int mm3dgs_slam_visibility(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, int32_t* radii, uint32_t* seen_count, void* geom_state,
                           void* stream) {
  if (int rc = check_slam(cam, P, in)) return rc;
  if (!geom_state || (P > 0 && !radii)) return fail(-1, "NULL buffer");
  launch_slam_preprocess_fwd(cam_dev(cam), P, slam_in(in), radii, geom_view(geom_state, P > 0 ? P : 1), ImageView{}, (hipStream_t)stream, seen_count, true);
  return check_launch("slam_visibility");
}

int mm3dgs_slam_forward(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, float* out_color, int32_t* radii,
                        void* geom_state, void* image_state, void* binning_state, size_t N_capacity, int flags, void* stream) {
  SlamCall c;
  if (int rc = slam_call(c, cam, P, in, out_color, radii, geom_state, image_state, binning_state, N_capacity, nullptr, flags, stream, SLAM_OUT)) return rc;
  return slam_forward(c, {.projected = (flags & MM3DGS_FWD_PROJECTED) != 0});
}

// ---- ABI structs -> the kernels' structs, with their rules (NULL: all zero) ----
// sh: the gradient outputs need d_f_rest too; stats: take the densification statistics (mm3dgs_slam_adam_project ignores them)
static int slam_grads_dev(const Mm3dgsSlamGrads* grads, bool sh, bool stats, SlamGrads& sg) {
  sg = {};
  if (!grads) return 0;
  const bool any = grads->d_xyz || grads->d_f_dc || grads->d_opacity || grads->d_scaling || grads->d_rotation;
  const bool all = grads->d_xyz && grads->d_f_dc && grads->d_opacity && grads->d_scaling && grads->d_rotation;
  if (any && !all) return fail(-2, "Gaussian gradient outputs must be all set or all NULL");
  if (all && sh && !grads->d_f_rest) return fail(-2, "sh_degree > 0: the gradient outputs need d_f_rest too");
  sg.d_xyz = grads->d_xyz; sg.d_f_dc = grads->d_f_dc; sg.d_opacity = grads->d_opacity; sg.d_scaling = grads->d_scaling;
  sg.d_rotation = grads->d_rotation; sg.d_f_rest = (all && sh) ? grads->d_f_rest : nullptr;
  if (!stats) return 0;
  if (grads->max_radii2D && (!grads->grad_accum || !grads->denom)) return fail(-2, "statistics outputs must be all set or all NULL");
  sg.max_radii2D = grads->max_radii2D; sg.grad_accum = grads->grad_accum; sg.denom = grads->denom;
  return 0;
}
// (pose_adam NULL or without a pose: no step)
static int pose_adam_dev(const Mm3dgsPoseAdam* pose_adam, PoseAdam& pa) {
  pa = {};
  if (!pose_adam || !pose_adam->pose) return 0;
  if (!pose_adam->m || !pose_adam->v || !pose_adam->step) return fail(-2, "pose Adam state missing");
  pa.pose = pose_adam->pose; pa.m = pose_adam->m; pa.v = pose_adam->v; pa.step = pose_adam->step;
  pa.lr_q = pose_adam->lr_q; pa.lr_t = pose_adam->lr_t; pa.beta1 = pose_adam->beta1; pa.beta2 = pose_adam->beta2; pa.eps = (float)pose_adam->eps;
  if (pose_adam->prior_pose && (pose_adam->prior_w_t != 0.f || pose_adam->prior_w_q != 0.f)) {
    pa.prior = pose_adam->prior_pose; pa.prior_w_t = pose_adam->prior_w_t; pa.prior_w_q = pose_adam->prior_w_q;
  }
  pa.best = pose_adam->best;
  return 0;
}
// Mm3dgsMapAdam -> the kernels' scalars: formed in double, rounded once to float (torch.optim.Adam does this arithmetic on Python floats)
static int map_adam_dev(const Mm3dgsMapAdam* map_adam, bool sh, MapAdam& ma) {
  ma = {};
  if (map_adam->step < 1) return fail(-1, "map Adam step must be >= 1");
  for (int i = 0; i < 5; i++) {
    if (!map_adam->param[i] || !map_adam->exp_avg[i] || !map_adam->exp_avg_sq[i]) return fail(-2, "map Adam group %d has a NULL pointer", i);
    ma.p[i] = map_adam->param[i]; ma.m[i] = map_adam->exp_avg[i]; ma.v[i] = map_adam->exp_avg_sq[i];
    ma.step_size[i] = (float)(map_adam->lr[i] / (1.0 - pow(map_adam->beta1, (double)map_adam->step)));
  }
  ma.omb1 = (float)(1.0 - map_adam->beta1); ma.beta2 = (float)map_adam->beta2; ma.omb2 = (float)(1.0 - map_adam->beta2);
  ma.eps = (float)map_adam->eps;
  ma.bc2s = (float)sqrt(1.0 - pow(map_adam->beta2, (double)map_adam->step));
  ma.opt_mask = map_adam->opt_mask;
  ma.rp = map_adam->rest_param; ma.rm = map_adam->rest_exp_avg; ma.rv = map_adam->rest_exp_avg_sq;
  if (sh && !ma.rp) return fail(-2, "sh_degree > 0: the map Adam state needs the f_rest group (rest_param / rest_exp_avg / rest_exp_avg_sq)");
  if (ma.rp && (!ma.rm || !ma.rv)) return fail(-2, "map Adam: the f_rest group has a NULL moment pointer");
  ma.rest_step_size = (float)(map_adam->rest_lr / (1.0 - pow(map_adam->beta1, (double)map_adam->step)));
  ma.on = 1;
  return 0;
}

struct SlamBwd {
  const float* dL_dout = nullptr;
  SlamGrads grads = {}; float* dL_dpose = nullptr; PoseAdam pose_adam = {}; MapAdam map_adam = {};
  const TrackLoss* tl = nullptr;     // loss folded into the compositor's prologue
  float* prior_loss4 = nullptr;      // tracking: where the pose finish adds the pose prior's loss
  int dl_planes = 6;                 // (launch_composite_bwd_slam)
  bool compositor_done = false;      // the forward launch already ran the backward compositor (SlamFwd::track_dsub)
  const float* next_pose = nullptr;  // the next mapping view: this launch may project and bin it too
  bool pose_chain = false;
};
// Returns < 0: error | 0 | 1: the launch also projected and binned the view at o.next_pose (its forward is SlamFwd::projected).
static int slam_backward(const SlamCall& c, const SlamBwd& o) {
  const CamDev& cd = c.cd;
  const hipStream_t s = c.s;
  const TrackLoss* tl = o.tl;
  const MapAdam& ma = o.map_adam;
  PoseLossScale pls = {nullptr, 0, 0.f, nullptr};
  if (tl && tl->defer_scale) { pls.rows = tl->partial; pls.nrows = ((tl->cfg.W + 15) / 16) * ((tl->cfg.H + 15) / 16); pls.w_l1 = tl->cfg.w_l1; pls.loss4 = tl->loss4; }
  // (an active SH degree > 0: the pose gradient runs through the colours' viewing direction, so even a tracking iteration needs the colour sums of
  //  the mapping-layout records)
  const bool tracking = o.grads.d_xyz == nullptr && !ma.on && !c.sh();
  if (tl && !tracking && !tl->dmaps) return fail(-1, "internal: a loss folded into the mapping backward needs the SSIM maps");
  if (o.pose_chain && !tracking) return fail(-1, "internal: the pose chain is a tracking-mode path");
  if (!o.compositor_done)
  { ProfScope ps(tracking ? MM3DGS_PROF_COMPOSITE_BWD_TRACK : MM3DGS_PROF_COMPOSITE_BWD, s);
    launch_composite_bwd_slam(cd, tracking, c.g, c.iv, c.b, c.N_cap, o.dL_dout, c.bw.dsub, s, tl, o.dl_planes, o.pose_chain); }
  if (o.pose_chain) {
    // the tracking compositor applied the pose chain per (block, splat) and left one pose-gradient row per TILE at the head of the scratch: no
    // gradient records, no backward projection -- the pose finish sums the rows (GeomView.poserec, composite.hip)
    ProfScope ps(MM3DGS_PROF_PREPROCESS_BWD, s);
    launch_slam_pose_finish(c.bw.dsub, cd.gx * cd.gy, c.in.pose, o.dL_dpose, o.pose_adam, s, pls.rows ? &pls : nullptr, o.prior_loss4, &c.iv.hdr->overflow);
    return check_launch("slam_backward");
  }
  // mapping run, direct bins, in-kernel Adam, no pose step: this launch also projects and bins the NEXT iteration's view
  const bool fuse = o.next_pose && !tracking && ma.on && c.db.on && !o.dL_dpose && !o.pose_adam.pose && !o.grads.d_xyz && !c.sh();
  { ProfScope ps(MM3DGS_PROF_PREPROCESS_BWD, s);
    if (fuse) launch_slam_bwd_project(cd, c.P, c.in, c.radii, c.g, c.iv, c.b, c.N_cap, c.bw, o.grads, ma, o.next_pose, c.db.bin_cap, c.db.slot_bits, s);
    else launch_slam_preprocess_bwd(cd, c.P, c.in, c.radii, c.g, c.b, c.N_cap, c.bw, o.grads, o.dL_dpose, o.pose_adam, ma, s, pls.rows ? &pls : nullptr, o.prior_loss4, c.db.on, &c.iv.hdr->overflow); }
  const int rc = check_launch("slam_backward");
  return rc ? rc : (fuse ? 1 : 0);
}

int mm3dgs_slam_backward(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, const int32_t* radii,
                         const void* geom_state, const void* image_state, const void* binning_state, size_t N_capacity,
                         const float* dL_dout, void* backward_scratch, const Mm3dgsSlamGrads* grads, float* dL_dpose,
                         const Mm3dgsPoseAdam* pose_adam, const Mm3dgsMapAdam* map_adam, int flags, void* stream) {
  SlamCall c;
  if (int rc = slam_call(c, cam, P, in, nullptr, (int32_t*)radii, (void*)geom_state, (void*)image_state, (void*)binning_state, N_capacity, backward_scratch,
                         flags, stream, SLAM_SCRATCH)) return rc;
  if (!dL_dout) return fail(-1, "NULL buffer");
  SlamBwd o = {.dL_dout = dL_dout, .dL_dpose = dL_dpose};
  if (int rc = slam_grads_dev(grads, c.sh(), true, o.grads)) return rc;
  if (int rc = pose_adam_dev(pose_adam, o.pose_adam)) return rc;
  if (map_adam)
    if (int rc = map_adam_dev(map_adam, c.sh(), o.map_adam)) return rc;
  return std::min(slam_backward(c, o), 0);
}

// ---- image losses; work buffer: sums (256 B) | dmaps [9,H,W] float | partial [16x16 tiles][12] double ----
static size_t loss_rows(int H, int W) { return (size_t)((W + 15) / 16) * ((H + 15) / 16); }
static size_t loss_dmaps_bytes(int H, int W) { return align_up((size_t)9 * H * W * 4, 256); }
size_t mm3dgs_loss_work_bytes(int H, int W) { return 256 + loss_dmaps_bytes(H, W) + align_up(loss_rows(H, W) * 12 * 8, 256); }
struct LossWork { double* sums; float* dmaps; double* partial; };
static LossWork loss_work_view(void* work, int H, int W) {
  char* c = (char*)work;
  return {(double*)c, (float*)(c + 256), (double*)(c + 256 + loss_dmaps_bytes(H, W))};
}
static LossCfg loss_cfg_dev(const Mm3dgsLossConfig* c) {
  LossCfg lc;
  lc.H = c->H; lc.W = c->W; lc.w_l1 = c->w_l1; lc.w_ssim = c->w_ssim; lc.w_pearson = c->w_pearson; lc.l1_mask = c->l1_mask;
  lc.pearson_mask = c->pearson_mask; lc.pearson_invert = c->pearson_invert; lc.sil_thr = c->sil_thr;
  for (int i = 0; i < 11; i++) lc.window[i] = c->window[i];
  lc.w_depth = c->w_depth_l1; lc.depth_mask = c->depth_l1_mask; lc.l1_sum = c->l1_sum;
  return lc;
}
// the splatam forms of the losses (depth-L1 term, colour L1 over { ref > 0 }, sums instead of means) exist in the standalone loss
// kernels only: a configuration that uses them is never folded into the compositors
static bool loss_is_variant(const Mm3dgsLossConfig* c) { return c->w_depth_l1 != 0.f || c->l1_sum != 0 || (c->l1_mask & 2) != 0; }
static int loss_cfg_check(const Mm3dgsLossConfig* c, const float* ref) {
  if (c->w_pearson != 0.f && !ref) return fail(-2, "Pearson term needs a reference depth");
  if ((c->w_depth_l1 != 0.f || (c->l1_mask & 2)) && !ref) return fail(-2, "depth-L1 term / { ref > 0 } mask needs a reference depth");
  if (c->w_depth_l1 != 0.f && c->w_pearson != 0.f) return fail(-2, "the depth-L1 and Pearson terms are exclusive");
  return 0;
}
// what the standalone loss kernels (launch_loss) ask of the image size
static int loss_size_check(const Mm3dgsLossConfig* c) {
  if (c->H <= 0 || c->W <= 0) return fail(-1, "bad image size");
  if ((double)c->H * c->W * 36.0 >= 4294967296.0) return fail(-1, "image too large for the loss kernels' 32-bit offsets");
  return 0;
}
static int slam_loss(const LossCfg& lc, const float* out6, const float* gt_color, const float* ref, const LossWork& w, float* dL, float* loss4, hipStream_t s) {
  ProfScope ps(MM3DGS_PROF_LOSS, s);
  launch_loss(lc, out6, gt_color, ref, w.dmaps, w.sums, w.partial, dL, loss4, s);
  return check_launch("loss");
}

int mm3dgs_loss(const Mm3dgsLossConfig* c, const float* out6, const float* gt_color, const float* ref, void* work, float* dL,
                float* loss4, void* stream) {
  if (!c || !out6 || !gt_color || !work || !dL) return fail(-1, "NULL argument");
  if (int rc = loss_size_check(c)) return rc;
  if (int rc = loss_cfg_check(c, ref)) return rc;
  return slam_loss(loss_cfg_dev(c), out6, gt_color, ref, loss_work_view(work, c->H, c->W), dL, loss4, (hipStream_t)stream);
}

int mm3dgs_slam_track(int n_iter, const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, float* out_color, int32_t* radii,
                      void* geom_state, void* image_state, void* binning_state, size_t N_capacity, int fwd_flags,
                      const Mm3dgsLossConfig* loss_cfg, const float* gt_color, const float* ref, void* loss_work, float* dL_dout,
                      float* loss4, void* backward_scratch, const Mm3dgsPoseAdam* pose_adam, void* stream) {
  if (n_iter < 0) return fail(-1, "n_iter < 0");
  if (!loss_cfg || !gt_color || !loss_work || !dL_dout) return fail(-1, "NULL argument");
  SlamCall c;
  if (int rc = slam_call(c, cam, P, in, out_color, radii, geom_state, image_state, binning_state, N_capacity, backward_scratch, fwd_flags, stream,
                         SLAM_OUT | SLAM_SCRATCH)) return rc;
  PoseAdam pa;
  if (int rc = pose_adam_dev(pose_adam, pa)) return rc;
  if (!pa.pose) return fail(-2, "tracking needs the pose Adam state");
  if (int rc = loss_cfg_check(loss_cfg, ref)) return rc;
  // The per-call developer switches are read here, once per call: tests compare both sides of each in one process.
  // fold: without SSIM every loss term is per pixel, so the loss runs inside the compositors (two launches and the gradient image round trip
  // less per iteration); needs the sort + forward-composite kernel (its workgroup = one 16x16 loss tile).  An active SH degree keeps the
  // standalone loss kernels, the mapping-mode compositor and the gradient records (slam_backward).
  const bool fold = !env_flag("MM3DGS_NO_FOLDED_LOSS", 0) && !c.sh() && !loss_is_variant(loss_cfg) && loss_cfg->w_ssim == 0.f && c.fused_sort;
  // masked L1 only: no loss-finish launch, 1/n goes to the pose gradient ...
  const bool defer_scale = fold && loss_cfg->w_pearson == 0.f;
  // ... and the backward compositor runs in the forward launch
  const bool fuse_track = defer_scale && !env_flag("MM3DGS_NO_FUSED_TRACK", 0);
  // the pose chain: the projection writes every splat's { Kp, Kq, x }, the tracking compositor applies it per (block, splat) and leaves one pose row
  // per tile: no gradient records, no per-tile combine, no backward-projection launch (three launches per iteration).  The shipped mode only (means
  // pre-transformed: the world-frame mode's pose gradient also runs through the covariance rotation)
  const bool pose_chain = !c.in.world && !c.sh() && !env_flag("MM3DGS_NO_POSE_CHAIN", 0) &&
                          bwd_bytes_impl(P, N_capacity) >= (size_t)c.cd.gx * c.cd.gy * 32 * sizeof(float);
  if (fold && (loss_cfg->H != c.cd.H || loss_cfg->W != c.cd.W)) return fail(-1, "loss and camera image sizes differ");
  if (!fold)
    if (int rc = loss_size_check(loss_cfg)) return rc;
  const LossCfg lc = loss_cfg_dev(loss_cfg);
  const LossWork lw = loss_work_view(loss_work, loss_cfg->H, loss_cfg->W);
  TrackLoss tl = {};
  tl.cfg = lc; tl.gt = gt_color; tl.ref = ref; tl.out = out_color; tl.sums = lw.sums; tl.partial = lw.partial; tl.loss4 = loss4;
  tl.defer_scale = defer_scale ? 1 : 0;
  const SlamFwd fwd = {.tl = fold ? &tl : nullptr, .track_dsub = fuse_track ? c.bw.dsub : nullptr, .pose_chain = pose_chain};
  const SlamBwd bwd = {.dL_dout = dL_dout, .pose_adam = pa, .tl = fwd.tl, .prior_loss4 = loss4, .compositor_done = fuse_track, .pose_chain = pose_chain};
  if (n_iter > 0) slam_refresh_tile_order(c);
  for (int it = 0; it < n_iter; it++) {
    if (int rc = slam_forward(c, fwd)) return rc;
    if (!fold) {
      if (int rc = slam_loss(lc, out_color, gt_color, ref, lw, dL_dout, loss4, c.s)) return rc;
    } else if (!defer_scale) {
      ProfScope ps(MM3DGS_PROF_LOSS, c.s);
      launch_loss_finish(lc, lw.sums, lw.partial, c.s);
    }
    if (int rc = slam_backward(c, bwd); rc < 0) return rc;
  }
  return 0;
}

int mm3dgs_slam_map(int n_iter, const Mm3dgsMapView* views, const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, float* out_color,
                    int32_t* radii, void* geom_state, void* image_state, void* binning_state, size_t N_capacity, int fwd_flags,
                    const Mm3dgsLossConfig* loss_cfg, void* loss_work, float* dL_dout, float* loss4, void* backward_scratch,
                    const Mm3dgsSlamGrads* grads_stats, const Mm3dgsMapAdam* map_adam, void* stream) {
  if (n_iter < 0) return fail(-1, "n_iter < 0");
  if (!views || !loss_cfg || !loss_work || !dL_dout) return fail(-1, "NULL argument");
  SlamCall c;
  if (int rc = slam_call(c, cam, P, in, out_color, radii, geom_state, image_state, binning_state, N_capacity, backward_scratch, fwd_flags, stream,
                         SLAM_OUT | SLAM_SCRATCH | SLAM_POSE_LATER)) return rc;
  if (n_iter > 0 && !map_adam && !(grads_stats && grads_stats->d_xyz)) return fail(-1, "neither an Adam state nor gradient outputs");
  SlamBwd bwd = {.dL_dout = dL_dout};
  if (int rc = slam_grads_dev(grads_stats, c.sh(), true, bwd.grads)) return rc;
  Mm3dgsMapAdam ad = {};      // (the caller's, with the step counter this loop advances)
  if (map_adam) {
    ad = *map_adam;
    if (int rc = map_adam_dev(&ad, c.sh(), bwd.map_adam)) return rc;
  }
  for (int it = 0; it < n_iter; it++) {
    const Mm3dgsMapView& v = views[it];
    if (!v.pose || !v.gt_color) return fail(-1, "view %d: NULL pose or colour target", it);
    if (v.pose_adam_or_null && v.dpose_out_or_null) return fail(-2, "view %d: either a pose step or a pose-gradient output", it);
    if (int rc = loss_cfg_check(loss_cfg, v.ref_depth_or_null)) return rc;
    if (int rc = pose_adam_dev(v.pose_adam_or_null, bwd.pose_adam)) return rc;
  }
  // The per-call developer switches are read here, once per call: tests compare both sides of each in one process.
  // rows: SSIM losses on the fused-sort path (the shipped mapping loss): the forward compositor's epilogue writes the per-tile L1 / Pearson rows,
  // the SSIM kernel's extra workgroup reduces them, and the gradient image has four planes: two launches per iteration for the loss instead of
  // three (no finishing launch), the loss values only once, at the end of the run
  const bool rows = !env_flag("MM3DGS_NO_FORWARD_ROWS", 0) && !loss_is_variant(loss_cfg) && loss_cfg->w_ssim != 0.f && c.fused_sort &&
                    loss_cfg->H == c.cd.H && loss_cfg->W == c.cd.W;
  // ... and the gradient-image pass itself runs in the backward compositor's prologue (TrackLoss::dmaps)
  const bool fold_grad = rows && !env_flag("MM3DGS_NO_FOLDED_LOSS", 0);
  // the backward launch of iteration `it` projects and bins the view of iteration `it + 1` when nothing stands between them (direct bins,
  // in-kernel Adam, neither view steps its pose or hands its pose gradient out: slam_backward has the rest of the rule)
  const bool fuse_proj = rows && map_adam && !env_flag("MM3DGS_NO_FUSED_PROJECT", 0);
  if (!rows)
    if (int rc = loss_size_check(loss_cfg)) return rc;
  const LossCfg lc = loss_cfg_dev(loss_cfg);
  const LossWork lw = loss_work_view(loss_work, loss_cfg->H, loss_cfg->W);
  TrackLoss tl = {};
  tl.cfg = lc; tl.out = out_color; tl.sums = lw.sums; tl.partial = lw.partial; tl.dmaps = fold_grad ? lw.dmaps : nullptr;
  bwd.tl = fold_grad ? &tl : nullptr;
  bwd.dl_planes = rows ? 4 : 6;
  bool projected = (fwd_flags & MM3DGS_FWD_PROJECTED) != 0;     // (view 0 only: mm3dgs_slam_adam_project launched its projection + binning)
  if (n_iter > 0) slam_refresh_tile_order(c);
  for (int it = 0; it < n_iter; it++) {
    const Mm3dgsMapView& v = views[it];
    c.in.pose = v.pose;
    tl.gt = v.gt_color; tl.ref = v.ref_depth_or_null;
    if (int rc = slam_forward(c, {.tl = rows ? &tl : nullptr, .projected = projected})) return rc;
    if (rows) {
      { ProfScope ps(MM3DGS_PROF_LOSS, c.s);
        launch_loss_after_forward_rows(lc, out_color, tl.gt, tl.ref, lw.dmaps, lw.sums, lw.partial, fold_grad ? nullptr : dL_dout, c.s); }
      if (loss4 && it == n_iter - 1) launch_loss_finish(lc, lw.sums, lw.partial, c.s, loss4);
      if (int rc = check_launch("loss")) return rc;
    } else if (int rc = slam_loss(lc, out_color, tl.gt, tl.ref, lw, dL_dout, loss4, c.s)) return rc;
    bwd.dL_dpose = v.dpose_out_or_null;
    (void)pose_adam_dev(v.pose_adam_or_null, bwd.pose_adam);      // (checked above)
    if (map_adam)
      if (int rc = map_adam_dev(&ad, c.sh(), bwd.map_adam)) return rc;
    ad.step++;
    bwd.next_pose = (fuse_proj && it + 1 < n_iter && !v.pose_adam_or_null && !views[it + 1].pose_adam_or_null && !v.dpose_out_or_null) ? views[it + 1].pose : nullptr;
    const int rc = slam_backward(c, bwd);
    if (rc < 0) return rc;
    projected = rc == 1;
  }
  return 0;
}

int mm3dgs_adam(const Mm3dgsAdamGroup* groups, int n_groups, int step, double beta1, double beta2, double eps, void* stream) {
  if (!groups || n_groups < 0 || n_groups > 8) return fail(-1, "bad group table");
  if (step < 1) return fail(-1, "step must be >= 1");
  AdamArgs a;
  a.ngroups = n_groups; a.omb1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
  const double bc1 = 1.0 - pow(beta1, (double)step);
  a.bc2s = (float)sqrt(1.0 - pow(beta2, (double)step));
  for (int i = 0; i < n_groups; i++) {
    if (groups[i].n && (!groups[i].param || !groups[i].grad || !groups[i].exp_avg || !groups[i].exp_avg_sq)) return fail(-1, "NULL in group %d", i);
    a.grp[i].p = groups[i].param; a.grp[i].g = groups[i].grad; a.grp[i].m = groups[i].exp_avg; a.grp[i].v = groups[i].exp_avg_sq;
    a.grp[i].n = groups[i].n; a.grp[i].step_size = (float)(groups[i].lr / bc1);
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MM3DGS_PROF_ADAM, s);
  launch_fused_adam(a, s);
  return check_launch("adam");
}

int mm3dgs_slam_direct_bins(const Mm3dgsCamera* cam, int P, size_t N_capacity, int fwd_flags) {
  if (!cam || P <= 0 || cam->image_height <= 0 || cam->image_width <= 0) return 0;
  return slam_direct_bins(fwd_flags, cam_dev(cam), P, N_capacity).on ? 1 : 0;
}

int mm3dgs_slam_adam_project(const Mm3dgsCamera* cam, int P, const Mm3dgsSlamInputs* in, const Mm3dgsSlamGrads* grads, const Mm3dgsMapAdam* adam,
                             int32_t* radii, void* geom_state, void* image_state, void* binning_state, size_t N_capacity, int fwd_flags, void* stream) {
  SlamCall c;
  if (int rc = slam_call(c, cam, P, in, nullptr, radii, geom_state, image_state, binning_state, N_capacity, nullptr, fwd_flags, stream, 0)) return rc;
  if (!grads || !adam) return fail(-1, "NULL argument");
  // (ABI 212) an active SH degree: the sixth group -- its gradient array and its Adam state -- or nothing is launched
  SlamGrads sg;
  if (int rc = slam_grads_dev(grads, c.sh(), false, sg)) return rc;
  if (!sg.d_xyz) return fail(-2, "all five gradient arrays are needed");
  MapAdam ma;
  if (int rc = map_adam_dev(adam, c.sh(), ma)) return rc;
  if (!c.db.on) return fail(-3, "mm3dgs_slam_adam_project needs direct bins (flags / map size / capacity)");
  { ProfScope ps(MM3DGS_PROF_ADAM, c.s);
    launch_slam_adam_project(c.cd, P, c.in, radii, c.g, c.iv, c.b, sg, ma, c.in.pose, c.db.bin_cap, c.db.slot_bits, c.s); }
  return check_launch("slam_adam_project");
}

// ---- map surgery (compact.hip) -----------------------------------------------------------------------------------------
int mm3dgs_covisibility_ratio(int H, int W, const float* depth, const float* silhouette, const float* keyframe_pose, const float* current_pose,
                              float fx, float fy, float cx, float cy, uint32_t* counts, void* stream) {
  if (H < 0 || W < 0 || !depth || !silhouette || !keyframe_pose || !current_pose || !counts) return fail(-1, "covisibility_ratio: bad argument");
  launch_covisibility_ratio(H, W, depth, silhouette, keyframe_pose, current_pose, fx, fy, cx, cy, counts, (hipStream_t)stream);
  return check_launch("covisibility_ratio");
}

int mm3dgs_propagate_const_vel(const float* pose_m1, const float* pose_m2, float* out_pose, void* stream) {
  if (!pose_m1 || !pose_m2 || !out_pose) return fail(-1, "propagate_const_vel: NULL argument");
  launch_propagate_const_vel(pose_m1, pose_m2, out_pose, (hipStream_t)stream);
  return check_launch("propagate_const_vel");
}

int mm3dgs_propagate_imu(const float* pose_m1, const float* pose_m2, const float* imu6, int n, const float* c2i, double dt_cam, double dt_imu,
                         double gx, double gy, double gz, float* out_pose, void* stream) {
  if (!pose_m1 || !pose_m2 || !c2i || !out_pose) return fail(-1, "propagate_imu: NULL argument");
  if (n < 0) return fail(-2, "propagate_imu: n = %d < 0", n);
  if (n > 0 && !imu6) return fail(-1, "propagate_imu: imu6 is NULL with n = %d samples", n);
  if (!isfinite(dt_cam) || !isfinite(dt_imu) || dt_cam == 0.0) return fail(-2, "propagate_imu: dt_cam = %g (finite, not 0) / dt_imu = %g (finite)", dt_cam, dt_imu);
  if (!isfinite(gx) || !isfinite(gy) || !isfinite(gz)) return fail(-2, "propagate_imu: gravity (%g, %g, %g) is not finite", gx, gy, gz);
  launch_propagate_imu(pose_m1, pose_m2, imu6, n, c2i, dt_cam, dt_imu, gx, gy, gz, out_pose, (hipStream_t)stream);
  return check_launch("propagate_imu");
}

size_t mm3dgs_align_depth_work_bytes(int H, int W) { return (H > 0 && W > 0) ? align_depth_work_bytes(H, W) : 0; }

int mm3dgs_align_depth(int H, int W, const float* est, const float* depth, const float* silhouette_or_null, float sil_min, float est_min,
                       void* work, double* fit, float* out_or_null, void* stream) {
  if (H <= 0 || W <= 0) return fail(-1, "align_depth: H = %d, W = %d (both must be positive)", H, W);
  if (!est || !depth || !work || !fit) return fail(-1, "align_depth: NULL argument (est, depth, work and fit are required)");
  if (((uintptr_t)work | (uintptr_t)fit) & 7) return fail(-1, "align_depth: work and fit must be 8-byte aligned");
  launch_align_depth(H, W, est, depth, silhouette_or_null, sil_min, est_min, (double*)work, fit, out_or_null, (hipStream_t)stream);
  return check_launch("align_depth");
}

static bool eval_shape_ok(int H, int W) { return H > 0 && W > 0 && (size_t)H * (size_t)W <= ((size_t)1 << 28); }

size_t mm3dgs_eval_image_work_bytes(int H, int W) { return eval_shape_ok(H, W) ? eval_image_work_bytes(H, W) : 0; }

int mm3dgs_eval_image(int H, int W, const float* image, const float* gt, const float* depth_or_null, const float* gt_depth_or_null,
                      const float* window, void* work, double* row, void* stream) {
  if (H <= 0 || W <= 0) return fail(-1, "eval_image: H = %d, W = %d (both must be positive)", H, W);
  if (!eval_shape_ok(H, W)) return fail(-1, "eval_image: %d x %d has more than 2^28 pixels", H, W);
  if (!image || !gt || !window || !work || !row) return fail(-1, "eval_image: NULL argument (image, gt, window, work and row are required)");
  if ((depth_or_null != nullptr) != (gt_depth_or_null != nullptr))
    return fail(-1, "eval_image: depth and gt_depth must both be given or both be NULL");
  if (((uintptr_t)work | (uintptr_t)row) & 7) return fail(-1, "eval_image: work and row must be 8-byte aligned");
  if (((uintptr_t)image | (uintptr_t)gt | (uintptr_t)depth_or_null | (uintptr_t)gt_depth_or_null) & 3)
    return fail(-1, "eval_image: the images must be 4-byte aligned");
  launch_eval_image(H, W, image, gt, depth_or_null, gt_depth_or_null, window, (double*)work, row, (hipStream_t)stream);
  return check_launch("eval_image");
}

// ---- fused point cloud (pointcloud.hip) ------------------------------------------------------------------------------------
static bool pointcloud_slots_ok(uint64_t slots) { return slots >= 64 && slots <= ((uint64_t)1 << 40) && (slots & (slots - 1)) == 0; }

size_t mm3dgs_pointcloud_work_bytes(int H, int W) { return eval_shape_ok(H, W) ? pointcloud_work_bytes(H, W) : 0; }

int mm3dgs_pointcloud_reset(void* table_or_null, uint64_t slots, uint64_t* counters, void* stream) {
  if (!counters) return fail(-1, "pointcloud_reset: counters is NULL");
  if ((uintptr_t)counters & 7) return fail(-1, "pointcloud_reset: counters must be 8-byte aligned");
  if (table_or_null && !pointcloud_slots_ok(slots))
    return fail(-1, "pointcloud_reset: slots = %llu (a power of two, at least 64, at most 2^40)", (unsigned long long)slots);
  if ((uintptr_t)table_or_null & 15) return fail(-1, "pointcloud_reset: table must be 16-byte aligned");
  launch_pointcloud_reset(table_or_null, slots, counters, (hipStream_t)stream);
  return check_launch("pointcloud_reset");
}

// the checks of one posed pinhole camera, shared by every call that takes one (`who` names the call), and its struct; the NULL and alignment
// tests of the pose stay with each call, whose messages name its other pointers
static int view_check(const char* who, int H, int W, double fx, double fy, double cx, double cy, const float* pose, PinholeView& out) {
  if (H <= 0 || W <= 0) return fail(-1, "%s: H = %d, W = %d (both must be positive)", who, H, W);
  if (!eval_shape_ok(H, W)) return fail(-1, "%s: %d x %d has more than 2^28 pixels", who, H, W);
  if (!isfinite(fx) || !isfinite(fy) || fx == 0.0 || fy == 0.0) return fail(-1, "%s: fx = %g, fy = %g (finite, not 0)", who, fx, fy);
  if (!isfinite(cx) || !isfinite(cy)) return fail(-1, "%s: cx = %g, cy = %g (must be finite)", who, cx, cy);
  out.H = H; out.W = W; out.fx = fx; out.fy = fy; out.cx = cx; out.cy = cy; out.pose = pose;
  return 0;
}

int mm3dgs_pointcloud_add_view(int H, int W, double fx, double fy, double cx, double cy, const float* pose, const float* color, const float* depth,
                               const float* silhouette_or_null, float sil_min, float depth_max, double voxel, uint32_t view, void* rows,
                               uint64_t cap, void* table_or_null, uint64_t slots, uint64_t* counters, void* work, void* stream) {
  PointCloudView v;
  if (int rc = view_check("pointcloud_add_view", H, W, fx, fy, cx, cy, pose, v)) return rc;
  if (!color || !depth || !pose || !rows || !counters || !work)
    return fail(-1, "pointcloud_add_view: NULL argument (color, depth, pose, rows, counters and work are required)");
  if (!(voxel >= 0.0) || !isfinite(voxel)) return fail(-1, "pointcloud_add_view: voxel = %g (must be finite and not negative)", voxel);
  if (voxel > 0.0 && !table_or_null) return fail(-1, "pointcloud_add_view: voxel = %g needs a table", voxel);
  if (voxel > 0.0 && !pointcloud_slots_ok(slots))
    return fail(-1, "pointcloud_add_view: slots = %llu (a power of two, at least 64, at most 2^40)", (unsigned long long)slots);
  if (((uintptr_t)rows | (uintptr_t)table_or_null) & 15) return fail(-1, "pointcloud_add_view: rows and table must be 16-byte aligned");
  if (((uintptr_t)counters | (uintptr_t)work) & 7) return fail(-1, "pointcloud_add_view: counters and work must be 8-byte aligned");
  if (((uintptr_t)color | (uintptr_t)depth | (uintptr_t)silhouette_or_null | (uintptr_t)pose) & 3)
    return fail(-1, "pointcloud_add_view: the images and the pose must be 4-byte aligned");
  v.color = color; v.depth = depth; v.sil = silhouette_or_null;
  v.sil_min = sil_min; v.depth_max = depth_max; v.voxel = voxel; v.view = view;
  v.table = voxel > 0.0 ? (unsigned long long*)table_or_null : nullptr;      // voxel == 0: no thinning, a table is ignored
  v.slots = v.table ? slots : 0;
  v.hash_shift = 64;
  for (uint64_t s = v.slots; s > 1; s >>= 1) v.hash_shift--;
  launch_pointcloud_add_view(v, rows, cap, counters, work, (hipStream_t)stream);
  return check_launch("pointcloud_add_view");
}

// ---- coloured triangle mesh (tsdf.hip) ---------------------------------------------------------------------------------------
static bool tsdf_lattice_ok(int nx, int ny, int nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (size_t)nx * (size_t)ny <= ((size_t)1 << 30) && (size_t)nx * (size_t)ny * (size_t)nz <= ((size_t)1 << 30);
}
static bool tsdf_origin_ok(const double* o) { return o && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]); }

// the checks every TSDF call with a view shares beyond view_check, dense or blocks; `who` names the call, `color` is NULL for a call that
// reads none, and a block call (max_trunc_voxels > 0) bounds the truncation distance in voxels
static int tsdf_view(const char* who, int H, int W, double fx, double fy, double cx, double cy, const float* pose, const float* color, const float* depth,
                     const float* sil, float sil_min, float depth_max, const double* origin, double voxel, double trunc, double max_trunc_voxels, TsdfView& v) {
  if (int rc = view_check(who, H, W, fx, fy, cx, cy, pose, v)) return rc;
  if (!depth || !pose || !origin) return fail(-1, "%s: NULL argument (depth, pose and the origin or anchor are required)", who);
  if (!(voxel > 0.0) || !isfinite(voxel) || !(trunc > 0.0) || !isfinite(trunc)) return fail(-1, "%s: voxel = %g, trunc = %g (both must be finite and positive)", who, voxel, trunc);
  if (max_trunc_voxels > 0.0 && !(trunc <= max_trunc_voxels * voxel))
    return fail(-1, "%s: trunc = %g is more than %g voxel = %g", who, trunc, max_trunc_voxels, max_trunc_voxels * voxel);
  if (!tsdf_origin_ok(origin)) return fail(-1, "%s: the origin or anchor must be finite", who);
  if (((uintptr_t)color | (uintptr_t)depth | (uintptr_t)sil | (uintptr_t)pose) & 3) return fail(-1, "%s: the images and the pose must be 4-byte aligned", who);
  v.color = color; v.depth = depth; v.sil = sil;
  v.sil_min = sil_min; v.depth_max = depth_max;
  v.o[0] = origin[0]; v.o[1] = origin[1]; v.o[2] = origin[2]; v.voxel = voxel; v.trunc = trunc;
  v.nx = v.ny = v.nz = 0;
  return 0;
}

int mm3dgs_tsdf_reset(int nx, int ny, int nz, void* tsdf_w, void* rgb_w, uint64_t* counters, void* stream) {
  if (!tsdf_lattice_ok(nx, ny, nz)) return fail(-1, "tsdf_reset: lattice %d x %d x %d (every size at least 2, at most 2^30 samples)", nx, ny, nz);
  if (!tsdf_w || !rgb_w || !counters) return fail(-1, "tsdf_reset: NULL argument (tsdf_w, rgb_w and counters are required)");
  if (((uintptr_t)tsdf_w | (uintptr_t)counters) & 7) return fail(-1, "tsdf_reset: tsdf_w and counters must be 8-byte aligned");
  if ((uintptr_t)rgb_w & 15) return fail(-1, "tsdf_reset: rgb_w must be 16-byte aligned");
  const size_t n = (size_t)nx * (size_t)ny * (size_t)nz;
  if (hipMemsetAsync(tsdf_w, 0, n * 8, (hipStream_t)stream) != hipSuccess || hipMemsetAsync(rgb_w, 0, n * 16, (hipStream_t)stream) != hipSuccess ||
      hipMemsetAsync(counters, 0, 64, (hipStream_t)stream) != hipSuccess)
    return fail(-3, "tsdf_reset: hipMemsetAsync failed");
  return 0;
}

int mm3dgs_tsdf_integrate(int H, int W, double fx, double fy, double cx, double cy, const float* pose, const float* color, const float* depth,
                          const float* silhouette_or_null, float sil_min, float depth_max, const double* origin, double voxel, double trunc, int nx,
                          int ny, int nz, void* tsdf_w, void* rgb_w, uint64_t* counters, void* stream) {
  TsdfView v;
  if (int rc = tsdf_view("tsdf_integrate", H, W, fx, fy, cx, cy, pose, color, depth, silhouette_or_null, sil_min, depth_max, origin, voxel, trunc, 0.0, v)) return rc;
  if (!tsdf_lattice_ok(nx, ny, nz)) return fail(-1, "tsdf_integrate: lattice %d x %d x %d (every size at least 2, at most 2^30 samples)", nx, ny, nz);
  if (!color || !tsdf_w || !rgb_w || !counters) return fail(-1, "tsdf_integrate: NULL argument (color, tsdf_w, rgb_w and counters are required)");
  if ((uintptr_t)rgb_w & 15) return fail(-1, "tsdf_integrate: rgb_w must be 16-byte aligned");
  if (((uintptr_t)tsdf_w | (uintptr_t)counters) & 7) return fail(-1, "tsdf_integrate: tsdf_w and counters must be 8-byte aligned");
  v.nx = nx; v.ny = ny; v.nz = nz;
  launch_tsdf_integrate(v, tsdf_w, rgb_w, counters, (hipStream_t)stream);
  return check_launch("tsdf_integrate");
}

size_t mm3dgs_tsdf_mesh_work_bytes(int nx, int ny, int nz) { return tsdf_lattice_ok(nx, ny, nz) ? tsdf_mesh_work_bytes(nx, ny, nz) : 0; }

int mm3dgs_tsdf_mesh_plan(int nx, int ny, int nz, const void* tsdf_w, float min_weight, void* work, uint64_t* counters, void* stream) {
  if (!tsdf_lattice_ok(nx, ny, nz)) return fail(-1, "tsdf_mesh_plan: lattice %d x %d x %d (every size at least 2, at most 2^30 samples)", nx, ny, nz);
  if (!tsdf_w || !work || !counters) return fail(-1, "tsdf_mesh_plan: NULL argument (tsdf_w, work and counters are required)");
  if (!(min_weight == min_weight)) return fail(-1, "tsdf_mesh_plan: min_weight is not a number");
  if (((uintptr_t)tsdf_w | (uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "tsdf_mesh_plan: tsdf_w, work and counters must be 8-byte aligned");
  launch_tsdf_mesh_plan(nx, ny, nz, tsdf_w, min_weight, work, counters, (hipStream_t)stream);
  return check_launch("tsdf_mesh_plan");
}

int mm3dgs_tsdf_mesh_emit(int nx, int ny, int nz, const void* tsdf_w, const void* rgb_w, const double* origin, double voxel, const void* work,
                          void* rows, uint64_t vcap, void* triangles, uint64_t tcap, uint64_t* counters, void* stream) {
  if (!tsdf_lattice_ok(nx, ny, nz)) return fail(-1, "tsdf_mesh_emit: lattice %d x %d x %d (every size at least 2, at most 2^30 samples)", nx, ny, nz);
  if (!tsdf_w || !rgb_w || !origin || !work || !counters || (!rows && vcap) || (!triangles && tcap))
    return fail(-1, "tsdf_mesh_emit: NULL argument (tsdf_w, rgb_w, origin, work and counters are required; rows and triangles unless their cap is 0)");
  if (!(voxel > 0.0) || !isfinite(voxel)) return fail(-1, "tsdf_mesh_emit: voxel = %g (must be finite and positive)", voxel);
  if (!tsdf_origin_ok(origin)) return fail(-1, "tsdf_mesh_emit: the origin must be finite");
  if (((uintptr_t)rgb_w | (uintptr_t)rows) & 15) return fail(-1, "tsdf_mesh_emit: rgb_w and rows must be 16-byte aligned");
  if (((uintptr_t)tsdf_w | (uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "tsdf_mesh_emit: tsdf_w, work and counters must be 8-byte aligned");
  if ((uintptr_t)triangles & 3) return fail(-1, "tsdf_mesh_emit: triangles must be 4-byte aligned");
  launch_tsdf_mesh_emit(nx, ny, nz, tsdf_w, rgb_w, origin, voxel, work, rows, vcap, triangles, tcap, counters, (hipStream_t)stream);
  return check_launch("tsdf_mesh_emit");
}

// ---- the same as a voxel-block volume (tsdf_sparse.hip) ----------------------------------------------------------------------------
#define TSDF_MAX_BLOCKS ((uint64_t)1 << 21)      // 2^30 samples: 32-bit bases, int32 indices
#define TSDF_BLOCKS_MAX_TRUNC 16.0                // voxels: a pixel's box of blocks stays within BLK_MAX_BOX (tsdf_sparse.hip)
static bool tsdf_blocks_ok(uint64_t n) { return n >= 1 && n <= TSDF_MAX_BLOCKS; }
size_t mm3dgs_tsdf_blocks_table_bytes(uint64_t max_blocks) { return tsdf_blocks_ok(max_blocks) ? tsdf_blocks_table_bytes(max_blocks, nullptr) : 0; }

int mm3dgs_tsdf_blocks_reset(void* table, uint64_t max_blocks, uint64_t* counters, void* stream) {
  if (!tsdf_blocks_ok(max_blocks)) return fail(-1, "tsdf_blocks_reset: max_blocks = %llu (1 .. 2^21)", (unsigned long long)max_blocks);
  if (!table || !counters) return fail(-1, "tsdf_blocks_reset: NULL argument (table and counters are required)");
  if (((uintptr_t)table | (uintptr_t)counters) & 7) return fail(-1, "tsdf_blocks_reset: table and counters must be 8-byte aligned");
  launch_tsdf_blocks_reset(table, max_blocks, counters, (hipStream_t)stream);
  return check_launch("tsdf_blocks_reset");
}

int mm3dgs_tsdf_blocks_reserve(int H, int W, double fx, double fy, double cx, double cy, const float* pose, const float* depth, const float* silhouette_or_null,
                               float sil_min, float depth_max, const double* anchor, double voxel, double trunc, const int* clip_or_null, void* table,
                               uint64_t max_blocks, uint64_t* counters, void* stream) {
  TsdfView v;
  if (int rc = tsdf_view("tsdf_blocks_reserve", H, W, fx, fy, cx, cy, pose, nullptr, depth, silhouette_or_null, sil_min, depth_max, anchor, voxel, trunc, TSDF_BLOCKS_MAX_TRUNC, v)) return rc;
  if (!tsdf_blocks_ok(max_blocks)) return fail(-1, "tsdf_blocks_reserve: max_blocks = %llu (1 .. 2^21)", (unsigned long long)max_blocks);
  if (!table || !counters) return fail(-1, "tsdf_blocks_reserve: NULL argument (table and counters are required)");
  if (((uintptr_t)table | (uintptr_t)counters) & 7) return fail(-1, "tsdf_blocks_reserve: table and counters must be 8-byte aligned");
  TsdfBlockClip clip;
  for (int a = 0; a < 3; a++) {
    clip.lo[a] = clip_or_null ? clip_or_null[a] : -(1 << 20);
    clip.hi[a] = clip_or_null ? clip_or_null[3 + a] : (1 << 20);
  }
  launch_tsdf_blocks_reserve(v, clip, table, max_blocks, counters, (hipStream_t)stream);
  return check_launch("tsdf_blocks_reserve");
}

int mm3dgs_tsdf_blocks_list(void* table, uint64_t max_blocks, uint64_t* keys, uint64_t cap, void* stream) {
  if (!tsdf_blocks_ok(max_blocks)) return fail(-1, "tsdf_blocks_list: max_blocks = %llu (1 .. 2^21)", (unsigned long long)max_blocks);
  if (!table || (!keys && cap)) return fail(-1, "tsdf_blocks_list: NULL argument (table is required; keys unless cap is 0)");
  if (((uintptr_t)table | (uintptr_t)keys) & 7) return fail(-1, "tsdf_blocks_list: table and keys must be 8-byte aligned");
  launch_tsdf_blocks_list(table, max_blocks, keys, cap, (hipStream_t)stream);
  return check_launch("tsdf_blocks_list");
}

int mm3dgs_tsdf_blocks_index(void* table, uint64_t max_blocks, const uint64_t* keys, uint64_t n, int32_t* neighbours, uint64_t* counters, void* stream) {
  if (!tsdf_blocks_ok(max_blocks) || !tsdf_blocks_ok(n))
    return fail(-1, "tsdf_blocks_index: max_blocks = %llu, n = %llu (both 1 .. 2^21)", (unsigned long long)max_blocks, (unsigned long long)n);
  if (!table || !keys || !neighbours || !counters) return fail(-1, "tsdf_blocks_index: NULL argument (table, keys, neighbours and counters are required)");
  if (((uintptr_t)table | (uintptr_t)keys | (uintptr_t)counters) & 7) return fail(-1, "tsdf_blocks_index: table, keys and counters must be 8-byte aligned");
  if ((uintptr_t)neighbours & 3) return fail(-1, "tsdf_blocks_index: neighbours must be 4-byte aligned");
  launch_tsdf_blocks_index(table, max_blocks, keys, n, neighbours, counters, (hipStream_t)stream);
  return check_launch("tsdf_blocks_index");
}

int mm3dgs_tsdf_blocks_integrate(int H, int W, double fx, double fy, double cx, double cy, const float* pose, const float* color, const float* depth,
                                 const float* silhouette_or_null, float sil_min, float depth_max, const double* anchor, double voxel, double trunc,
                                 const uint64_t* keys, uint64_t n, void* tsdf_w, void* rgb_w, uint64_t* counters, void* stream) {
  TsdfView v;
  if (int rc = tsdf_view("tsdf_blocks_integrate", H, W, fx, fy, cx, cy, pose, color, depth, silhouette_or_null, sil_min, depth_max, anchor, voxel, trunc, TSDF_BLOCKS_MAX_TRUNC, v)) return rc;
  if (!tsdf_blocks_ok(n)) return fail(-1, "tsdf_blocks_integrate: n = %llu blocks (1 .. 2^21)", (unsigned long long)n);
  if (!color || !keys || !tsdf_w || !rgb_w || !counters) return fail(-1, "tsdf_blocks_integrate: NULL argument (color, keys, tsdf_w, rgb_w and counters are required)");
  if ((uintptr_t)rgb_w & 15) return fail(-1, "tsdf_blocks_integrate: rgb_w must be 16-byte aligned");
  if (((uintptr_t)tsdf_w | (uintptr_t)keys | (uintptr_t)counters) & 7) return fail(-1, "tsdf_blocks_integrate: tsdf_w, keys and counters must be 8-byte aligned");
  launch_tsdf_blocks_integrate(v, keys, n, tsdf_w, rgb_w, counters, (hipStream_t)stream);
  return check_launch("tsdf_blocks_integrate");
}

size_t mm3dgs_tsdf_blocks_mesh_work_bytes(uint64_t n) { return tsdf_blocks_ok(n) ? tsdf_blocks_mesh_work_bytes(n) : 0; }

int mm3dgs_tsdf_blocks_mesh_plan(uint64_t n, const int32_t* neighbours, const void* tsdf_w, float min_weight, void* work, uint64_t* counters, void* stream) {
  if (!tsdf_blocks_ok(n)) return fail(-1, "tsdf_blocks_mesh_plan: n = %llu blocks (1 .. 2^21)", (unsigned long long)n);
  if (!neighbours || !tsdf_w || !work || !counters) return fail(-1, "tsdf_blocks_mesh_plan: NULL argument (neighbours, tsdf_w, work and counters are required)");
  if (!(min_weight == min_weight)) return fail(-1, "tsdf_blocks_mesh_plan: min_weight is not a number");
  if (((uintptr_t)tsdf_w | (uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "tsdf_blocks_mesh_plan: tsdf_w, work and counters must be 8-byte aligned");
  if ((uintptr_t)neighbours & 3) return fail(-1, "tsdf_blocks_mesh_plan: neighbours must be 4-byte aligned");
  launch_tsdf_blocks_mesh_plan(n, neighbours, tsdf_w, min_weight, work, counters, (hipStream_t)stream);
  return check_launch("tsdf_blocks_mesh_plan");
}

int mm3dgs_tsdf_blocks_mesh_emit(uint64_t n, const uint64_t* keys, const int32_t* neighbours, const void* tsdf_w, const void* rgb_w, const double* anchor,
                                 double voxel, const void* work, void* rows, uint64_t vcap, void* triangles, uint64_t tcap, uint64_t* counters, void* stream) {
  if (!tsdf_blocks_ok(n)) return fail(-1, "tsdf_blocks_mesh_emit: n = %llu blocks (1 .. 2^21)", (unsigned long long)n);
  if (!keys || !neighbours || !tsdf_w || !rgb_w || !anchor || !work || !counters || (!rows && vcap) || (!triangles && tcap))
    return fail(-1, "tsdf_blocks_mesh_emit: NULL argument (keys, neighbours, tsdf_w, rgb_w, anchor, work and counters are required; rows and triangles unless their cap is 0)");
  if (!(voxel > 0.0) || !isfinite(voxel)) return fail(-1, "tsdf_blocks_mesh_emit: voxel = %g (must be finite and positive)", voxel);
  if (!tsdf_origin_ok(anchor)) return fail(-1, "tsdf_blocks_mesh_emit: the anchor must be finite");
  if (((uintptr_t)rgb_w | (uintptr_t)rows) & 15) return fail(-1, "tsdf_blocks_mesh_emit: rgb_w and rows must be 16-byte aligned");
  if (((uintptr_t)tsdf_w | (uintptr_t)keys | (uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "tsdf_blocks_mesh_emit: tsdf_w, keys, work and counters must be 8-byte aligned");
  if (((uintptr_t)triangles | (uintptr_t)neighbours) & 3) return fail(-1, "tsdf_blocks_mesh_emit: triangles and neighbours must be 4-byte aligned");
  launch_tsdf_blocks_mesh_emit(n, keys, neighbours, tsdf_w, rgb_w, anchor, voxel, work, rows, vcap, triangles, tcap, counters, (hipStream_t)stream);
  return check_launch("tsdf_blocks_mesh_emit");
}

// ---- geometry scores (geometry.hip) ----------------------------------------------------------------------------------------------
#define NN_MAX_ROWS ((uint64_t)1 << 30)
#define NN_MAX_CELLS ((size_t)1 << 26)
#define NN_MAX_RINGS 1048576.0      // ceil(max_dist / cell) at most 2^20
static bool nn_grid_ok(int gx, int gy, int gz) {
  return gx >= 1 && gy >= 1 && gz >= 1 && (size_t)gx * (size_t)gy <= NN_MAX_CELLS && (size_t)gx * (size_t)gy * (size_t)gz <= NN_MAX_CELLS;
}
static bool nn_origin_ok(const int64_t* o) {
  const int64_t lim = (int64_t)1 << 40;
  return o && o[0] > -lim && o[0] < lim && o[1] > -lim && o[1] < lim && o[2] > -lim && o[2] < lim;
}
static NnGrid nn_grid(double cell, const int64_t* o, int gx, int gy, int gz) {
  NnGrid g;
  g.cell = cell; g.o[0] = (double)o[0]; g.o[1] = (double)o[1]; g.o[2] = (double)o[2]; g.gx = gx; g.gy = gy; g.gz = gz;
  return g;
}

size_t mm3dgs_nn_grid_work_bytes(uint64_t n_ref, int gx, int gy, int gz) {
  return (n_ref >= 1 && n_ref <= NN_MAX_ROWS && nn_grid_ok(gx, gy, gz)) ? nn_grid_work_bytes(n_ref, gx, gy, gz) : 0;
}

int mm3dgs_nn_grid_build(uint64_t n_ref, const void* rows, double cell, const int64_t* origin_cell, int gx, int gy, int gz, uint32_t* cell_start,
                         void* sorted, uint64_t* counters, void* work, void* stream) {
  if (n_ref < 1 || n_ref > NN_MAX_ROWS) return fail(-1, "nn_grid_build: n_ref = %llu (1 .. 2^30)", (unsigned long long)n_ref);
  if (!nn_grid_ok(gx, gy, gz)) return fail(-1, "nn_grid_build: grid %d x %d x %d (every size at least 1, at most 2^26 cells)", gx, gy, gz);
  if (!(cell > 0.0) || !isfinite(cell)) return fail(-1, "nn_grid_build: cell = %g (must be finite and positive)", cell);
  if (!nn_origin_ok(origin_cell)) return fail(-1, "nn_grid_build: origin_cell is NULL or beyond +-2^40");
  if (!rows || !cell_start || !sorted || !counters || !work)
    return fail(-1, "nn_grid_build: NULL argument (rows, cell_start, sorted, counters and work are required)");
  if (((uintptr_t)rows | (uintptr_t)sorted) & 15) return fail(-1, "nn_grid_build: rows and sorted must be 16-byte aligned");
  if (((uintptr_t)counters | (uintptr_t)work) & 7) return fail(-1, "nn_grid_build: counters and work must be 8-byte aligned");
  if ((uintptr_t)cell_start & 3) return fail(-1, "nn_grid_build: cell_start must be 4-byte aligned");
  launch_nn_grid_build(nn_grid(cell, origin_cell, gx, gy, gz), n_ref, rows, cell_start, sorted, counters, work, (hipStream_t)stream);
  return check_launch("nn_grid_build");
}

size_t mm3dgs_nn_query_work_bytes(uint64_t n_q) { return (n_q >= 1 && n_q <= NN_MAX_ROWS) ? nn_query_work_bytes(n_q) : 0; }

// mm3dgs_nn_query and mm3dgs_nn_query_index: one body; want_index adds index_out to the required and to the 4-byte aligned pointers.
// want_index only words the checks: behind them index_out is non-NULL exactly when it is set (mm3dgs_nn_query passes NULL), and the
// launcher goes by the pointer alone
static int nn_query_call(const char* who, uint64_t n_q, const void* q_rows, uint64_t n_ref, double cell, const int64_t* origin_cell, int gx, int gy, int gz,
                         const uint32_t* cell_start, const void* sorted, double max_dist, double threshold, float* dist_out, double* row, void* work,
                         void* stream, uint32_t* index_out, bool want_index) {
  if (n_q < 1 || n_q > NN_MAX_ROWS) return fail(-1, "%s: n_q = %llu (1 .. 2^30)", who, (unsigned long long)n_q);
  if (n_ref < 1 || n_ref > NN_MAX_ROWS) return fail(-1, "%s: n_ref = %llu (1 .. 2^30)", who, (unsigned long long)n_ref);
  if (!nn_grid_ok(gx, gy, gz)) return fail(-1, "%s: grid %d x %d x %d (every size at least 1, at most 2^26 cells)", who, gx, gy, gz);
  if (!(cell > 0.0) || !isfinite(cell)) return fail(-1, "%s: cell = %g (must be finite and positive)", who, cell);
  if (!(max_dist > 0.0) || !isfinite(max_dist)) return fail(-1, "%s: max_dist = %g (must be finite and positive)", who, max_dist);
  if (!(threshold >= 0.0) || !isfinite(threshold)) return fail(-1, "%s: threshold = %g (must be finite and not negative)", who, threshold);
  const double rings = ceil(max_dist / cell);
  if (!(rings <= NN_MAX_RINGS)) return fail(-1, "%s: max_dist / cell = %g (at most 2^20 rings)", who, max_dist / cell);
  if (!nn_origin_ok(origin_cell)) return fail(-1, "%s: origin_cell is NULL or beyond +-2^40", who);
  if (!q_rows || !cell_start || !sorted || !dist_out || (want_index && !index_out) || !row || !work)
    return fail(-1, "%s: NULL argument (q_rows, cell_start, sorted, dist_out, %srow and work are required)", who, want_index ? "index_out, " : "");
  if (((uintptr_t)q_rows | (uintptr_t)sorted) & 15) return fail(-1, "%s: q_rows and sorted must be 16-byte aligned", who);
  if (((uintptr_t)row | (uintptr_t)work) & 7) return fail(-1, "%s: row and work must be 8-byte aligned", who);
  if (((uintptr_t)cell_start | (uintptr_t)dist_out | (uintptr_t)index_out) & 3)
    return fail(-1, "%s: cell_start%s must be 4-byte aligned", who, want_index ? ", dist_out and index_out" : " and dist_out");
  launch_nn_query(nn_grid(cell, origin_cell, gx, gy, gz), n_q, q_rows, n_ref, cell_start, sorted, max_dist, threshold, (int)(rings < 1.0 ? 1.0 : rings),
                  dist_out, index_out, row, work, (hipStream_t)stream);
  return check_launch(who);
}

int mm3dgs_nn_query(uint64_t n_q, const void* q_rows, uint64_t n_ref, double cell, const int64_t* origin_cell, int gx, int gy, int gz,
                    const uint32_t* cell_start, const void* sorted, double max_dist, double threshold, float* dist_out, double* row, void* work,
                    void* stream) {
  return nn_query_call("nn_query", n_q, q_rows, n_ref, cell, origin_cell, gx, gy, gz, cell_start, sorted, max_dist, threshold, dist_out, row, work, stream,
                       nullptr, false);
}

#define MS_MAX_TRIANGLES ((uint64_t)1 << 30)
size_t mm3dgs_mesh_sample_work_bytes(uint64_t m) { return (m >= 1 && m <= MS_MAX_TRIANGLES) ? mesh_sample_work_bytes(m) : 0; }

static int mesh_sample_check(const char* who, uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* tris, double density, const void* work,
                             const uint64_t* counters) {
  if (m < 1 || m > MS_MAX_TRIANGLES) return fail(-1, "%s: m = %llu triangles (1 .. 2^30)", who, (unsigned long long)m);
  if (n_vertices < 1 || n_vertices > ((uint64_t)1 << 31) - 1) return fail(-1, "%s: n_vertices = %llu (1 .. 2^31 - 1)", who, (unsigned long long)n_vertices);
  if (!(density > 0.0) || !isfinite(density)) return fail(-1, "%s: density = %g (must be finite and positive)", who, density);
  if (!vrows || !tris || !work || !counters) return fail(-1, "%s: NULL argument (vrows, triangles, work and counters are required)", who);
  if ((uintptr_t)vrows & 15) return fail(-1, "%s: vrows must be 16-byte aligned", who);
  if (((uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "%s: work and counters must be 8-byte aligned", who);
  if ((uintptr_t)tris & 3) return fail(-1, "%s: triangles must be 4-byte aligned", who);
  return 0;
}
static MeshSample mesh_sample(uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* tris, double density, uint32_t seed) {
  MeshSample ms;
  ms.vrows = (const uint4*)vrows; ms.n_vertices = (uint32_t)n_vertices; ms.tris = tris; ms.m = (uint32_t)m; ms.density = density; ms.seed = seed;
  return ms;
}

int mm3dgs_mesh_sample_plan(uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* triangles, double density, uint32_t seed, void* work,
                            uint64_t* counters, void* stream) {
  if (mesh_sample_check("mesh_sample_plan", n_vertices, vrows, m, triangles, density, work, counters)) return -1;
  launch_mesh_sample_plan(mesh_sample(n_vertices, vrows, m, triangles, density, seed), work, counters, (hipStream_t)stream);
  return check_launch("mesh_sample_plan");
}

// mm3dgs_mesh_sample_emit and mm3dgs_mesh_sample_emit_tri: one body; want_tri adds tri_out to the pointers a cap above 0 needs and only
// words the checks: the launcher goes by the pointer alone.  _emit_tri with a cap of 0 may pass a NULL tri_out and then runs the kernel
// without triangle ids: with no sample to write, the two instantiations write the same two counters
static int mesh_sample_emit_call(const char* who, uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* triangles, double density, uint32_t seed,
                                 const void* work, void* rows, uint64_t cap, uint64_t* counters, void* stream, uint32_t* tri_out, bool want_tri) {
  if (mesh_sample_check(who, n_vertices, vrows, m, triangles, density, work, counters)) return -1;
  if (cap > ((uint64_t)1 << 31)) return fail(-1, "%s: cap = %llu (at most 2^31)", who, (unsigned long long)cap);
  if ((!rows || (want_tri && !tri_out)) && cap) return fail(-1, "%s: rows %sis NULL with a cap above 0", who, want_tri ? "or tri_out " : "");
  if ((uintptr_t)rows & 15) return fail(-1, "%s: rows must be 16-byte aligned", who);
  if ((uintptr_t)tri_out & 3) return fail(-1, "%s: tri_out must be 4-byte aligned", who);
  launch_mesh_sample_emit(mesh_sample(n_vertices, vrows, m, triangles, density, seed), work, rows, tri_out, cap, counters, (hipStream_t)stream);
  return check_launch(who);
}

int mm3dgs_mesh_sample_emit(uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* triangles, double density, uint32_t seed, const void* work,
                            void* rows, uint64_t cap, uint64_t* counters, void* stream) {
  return mesh_sample_emit_call("mesh_sample_emit", n_vertices, vrows, m, triangles, density, seed, work, rows, cap, counters, stream, nullptr, false);
}

// ---- normals (geometry.hip): the two calls above with an index / a triangle per row, normal consistency, vertex normals ----------------
int mm3dgs_nn_query_index(uint64_t n_q, const void* q_rows, uint64_t n_ref, double cell, const int64_t* origin_cell, int gx, int gy, int gz,
                          const uint32_t* cell_start, const void* sorted, double max_dist, double threshold, float* dist_out, uint32_t* index_out,
                          double* row, void* work, void* stream) {
  return nn_query_call("nn_query_index", n_q, q_rows, n_ref, cell, origin_cell, gx, gy, gz, cell_start, sorted, max_dist, threshold, dist_out, row, work,
                       stream, index_out, true);
}

int mm3dgs_mesh_sample_emit_tri(uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* triangles, double density, uint32_t seed, const void* work,
                                void* rows, uint32_t* tri_out, uint64_t cap, uint64_t* counters, void* stream) {
  return mesh_sample_emit_call("mesh_sample_emit_tri", n_vertices, vrows, m, triangles, density, seed, work, rows, cap, counters, stream, tri_out, true);
}

// the size and pointer checks of one mesh argument (density and seed are not used by these calls)
static int normals_mesh_check(const char* who, const char* side, uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* tris) {
  if (m < 1 || m > MS_MAX_TRIANGLES) return fail(-1, "%s: m%s = %llu triangles (1 .. 2^30)", who, side, (unsigned long long)m);
  if (n_vertices < 1 || n_vertices > ((uint64_t)1 << 31) - 1) return fail(-1, "%s: n_vertices%s = %llu (1 .. 2^31 - 1)", who, side, (unsigned long long)n_vertices);
  if (!vrows || !tris) return fail(-1, "%s: NULL argument (vrows%s and triangles%s are required)", who, side, side);
  if ((uintptr_t)vrows & 15) return fail(-1, "%s: vrows%s must be 16-byte aligned", who, side);
  if ((uintptr_t)tris & 3) return fail(-1, "%s: triangles%s must be 4-byte aligned", who, side);
  return 0;
}

size_t mm3dgs_normal_consistency_work_bytes(uint64_t n_q) { return (n_q >= 1 && n_q <= NN_MAX_ROWS) ? normal_consistency_work_bytes(n_q) : 0; }

int mm3dgs_normal_consistency(uint64_t n_q, const uint32_t* tri_q, const uint32_t* index, uint64_t n_r, const uint32_t* tri_r, uint64_t n_vertices_q,
                              const void* vrows_q, uint64_t m_q, const int32_t* triangles_q, uint64_t n_vertices_r, const void* vrows_r, uint64_t m_r,
                              const int32_t* triangles_r, float* dot_out, double* row, void* work, void* stream) {
  if (n_q < 1 || n_q > NN_MAX_ROWS) return fail(-1, "normal_consistency: n_q = %llu (1 .. 2^30)", (unsigned long long)n_q);
  if (n_r < 1 || n_r > NN_MAX_ROWS) return fail(-1, "normal_consistency: n_r = %llu (1 .. 2^30)", (unsigned long long)n_r);
  if (normals_mesh_check("normal_consistency", "_q", n_vertices_q, vrows_q, m_q, triangles_q)) return -1;
  if (normals_mesh_check("normal_consistency", "_r", n_vertices_r, vrows_r, m_r, triangles_r)) return -1;
  if (!tri_q || !index || !tri_r || !dot_out || !row || !work)
    return fail(-1, "normal_consistency: NULL argument (tri_q, index, tri_r, dot_out, row and work are required)");
  if (((uintptr_t)row | (uintptr_t)work) & 7) return fail(-1, "normal_consistency: row and work must be 8-byte aligned");
  if (((uintptr_t)tri_q | (uintptr_t)index | (uintptr_t)tri_r | (uintptr_t)dot_out) & 3)
    return fail(-1, "normal_consistency: tri_q, index, tri_r and dot_out must be 4-byte aligned");
  launch_normal_consistency(n_q, tri_q, index, n_r, tri_r, mesh_sample(n_vertices_q, vrows_q, m_q, triangles_q, 1.0, 0u),
                            mesh_sample(n_vertices_r, vrows_r, m_r, triangles_r, 1.0, 0u), dot_out, row, work, (hipStream_t)stream);
  return check_launch("normal_consistency");
}

size_t mm3dgs_mesh_vertex_normals_work_bytes(uint64_t n_vertices) {
  return (n_vertices >= 1 && n_vertices <= ((uint64_t)1 << 31) - 1) ? mesh_vertex_normals_work_bytes(n_vertices) : 0;
}

int mm3dgs_mesh_vertex_normals(uint64_t n_vertices, const void* vrows, uint64_t m, const int32_t* triangles, float* normals, void* work, uint64_t* counters,
                               void* stream) {
  if (normals_mesh_check("mesh_vertex_normals", "", n_vertices, vrows, m, triangles)) return -1;
  if (!normals || !work || !counters) return fail(-1, "mesh_vertex_normals: NULL argument (normals, work and counters are required)");
  if (((uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "mesh_vertex_normals: work and counters must be 8-byte aligned");
  if ((uintptr_t)normals & 3) return fail(-1, "mesh_vertex_normals: normals must be 4-byte aligned");
  launch_mesh_vertex_normals(mesh_sample(n_vertices, vrows, m, triangles, 1.0, 0u), normals, work, counters, (hipStream_t)stream);
  return check_launch("mesh_vertex_normals");
}

// ---- point-to-point ICP (geometry.hip) -----------------------------------------------------------------------------------------------
size_t mm3dgs_icp_work_bytes(uint64_t n_q) { return (n_q >= 1 && n_q <= NN_MAX_ROWS) ? icp_work_bytes(n_q) : 0; }

int mm3dgs_icp_point(uint64_t n_q, const void* q_rows, uint64_t n_ref, double cell, const int64_t* origin_cell, int gx, int gy, int gz,
                     const uint32_t* cell_start, const void* sorted, double max_dist, int iters, double rel_fitness, double rel_rmse, double* state, double* log,
                     float* dist_out, uint32_t* index_out, void* work, void* stream) {
  if (n_q < 1 || n_q > NN_MAX_ROWS) return fail(-1, "icp_point: n_q = %llu (1 .. 2^30)", (unsigned long long)n_q);
  if (n_ref < 1 || n_ref > NN_MAX_ROWS) return fail(-1, "icp_point: n_ref = %llu (1 .. 2^30)", (unsigned long long)n_ref);
  if (!nn_grid_ok(gx, gy, gz)) return fail(-1, "icp_point: grid %d x %d x %d (every size at least 1, at most 2^26 cells)", gx, gy, gz);
  if (!(cell > 0.0) || !isfinite(cell)) return fail(-1, "icp_point: cell = %g (must be finite and positive)", cell);
  if (!(max_dist > 0.0) || !isfinite(max_dist)) return fail(-1, "icp_point: max_dist = %g (must be finite and positive)", max_dist);
  const double rings = ceil(max_dist / cell);
  if (!(rings <= NN_MAX_RINGS)) return fail(-1, "icp_point: max_dist / cell = %g (at most 2^20 rings)", max_dist / cell);
  if (iters < 1 || iters > 1000) return fail(-1, "icp_point: iters = %d (1 .. 1000)", iters);
  if (!(rel_fitness >= 0.0) || !(rel_rmse >= 0.0)) return fail(-1, "icp_point: rel_fitness = %g, rel_rmse = %g (neither may be negative or not a number)", rel_fitness, rel_rmse);
  if (!nn_origin_ok(origin_cell)) return fail(-1, "icp_point: origin_cell is NULL or beyond +-2^40");
  if (!q_rows || !cell_start || !sorted || !state || !log || !work)
    return fail(-1, "icp_point: NULL argument (q_rows, cell_start, sorted, state, log and work are required)");
  if (((uintptr_t)q_rows | (uintptr_t)sorted) & 15) return fail(-1, "icp_point: q_rows and sorted must be 16-byte aligned");
  if (((uintptr_t)state | (uintptr_t)log | (uintptr_t)work) & 7) return fail(-1, "icp_point: state, log and work must be 8-byte aligned");
  if (((uintptr_t)cell_start | (uintptr_t)dist_out | (uintptr_t)index_out) & 3) return fail(-1, "icp_point: cell_start, dist_out and index_out must be 4-byte aligned");
  launch_icp_point(nn_grid(cell, origin_cell, gx, gy, gz), n_q, q_rows, n_ref, cell_start, sorted, max_dist, (int)(rings < 1.0 ? 1.0 : rings), iters, rel_fitness,
                   rel_rmse, state, log, dist_out, index_out, work, (hipStream_t)stream);
  return check_launch("icp_point");
}

int mm3dgs_rows_move(uint64_t n, const void* rows_in, const double* T, void* rows_out, void* stream) {
  if (n < 1 || n > NN_MAX_ROWS) return fail(-1, "rows_move: n = %llu (1 .. 2^30)", (unsigned long long)n);
  if (!rows_in || !T || !rows_out) return fail(-1, "rows_move: NULL argument (rows_in, T and rows_out are required)");
  if (((uintptr_t)rows_in | (uintptr_t)rows_out) & 15) return fail(-1, "rows_move: rows_in and rows_out must be 16-byte aligned");
  if ((uintptr_t)T & 7) return fail(-1, "rows_move: T must be 8-byte aligned");
  launch_rows_move(n, rows_in, T, rows_out, (hipStream_t)stream);
  return check_launch("rows_move");
}

// ---- visibility culling (cull.hip) -------------------------------------------------------------------------------------------------
size_t mm3dgs_cull_work_bytes(uint64_t n) { return n <= NN_MAX_ROWS ? cull_work_bytes(n) : 0; }

int mm3dgs_cull_mark_view(int H, int W, double fx, double fy, double cx, double cy, const float* pose, const float* depth_or_null, float depth_max,
                          double z_near, double z_far, double eps, uint64_t n, const void* rows, uint32_t* seen, uint64_t* counters, void* stream) {
  CullView v;
  if (int rc = view_check("cull_mark_view", H, W, fx, fy, cx, cy, pose, v)) return rc;
  if (n > NN_MAX_ROWS) return fail(-1, "cull_mark_view: n = %llu (at most 2^30)", (unsigned long long)n);
  if (!pose || !counters || (n && (!rows || !seen))) return fail(-1, "cull_mark_view: NULL argument (pose and counters are required; rows and seen unless n is 0)");
  if (!(z_near >= 0.0) || !isfinite(z_near) || !(z_far >= 0.0) || !isfinite(z_far) || !(eps >= 0.0) || !isfinite(eps))
    return fail(-1, "cull_mark_view: near = %g, far = %g, eps = %g (each must be finite and not negative)", z_near, z_far, eps);
  if (!(depth_max == depth_max)) return fail(-1, "cull_mark_view: depth_max is not a number");
  if ((uintptr_t)rows & 15) return fail(-1, "cull_mark_view: rows must be 16-byte aligned");
  if ((uintptr_t)counters & 7) return fail(-1, "cull_mark_view: counters must be 8-byte aligned");
  if (((uintptr_t)seen | (uintptr_t)depth_or_null | (uintptr_t)pose) & 3) return fail(-1, "cull_mark_view: seen, the depth image and the pose must be 4-byte aligned");
  v.depth = depth_or_null; v.depth_max = depth_max;
  v.z_near = z_near; v.z_far = z_far; v.eps = eps;
  launch_cull_mark_view(v, n, rows, seen, counters, (hipStream_t)stream);
  return check_launch("cull_mark_view");
}

int mm3dgs_cull_select(uint64_t n, const void* rows, const uint32_t* seen, uint32_t min_views, void* out_rows, uint64_t cap, uint32_t* index_or_null,
                       void* work, uint64_t* counters, void* stream) {
  if (n > NN_MAX_ROWS) return fail(-1, "cull_select: n = %llu (at most 2^30)", (unsigned long long)n);
  if (min_views < 1) return fail(-1, "cull_select: min_views = 0 (at least 1)");
  if (cap > ((uint64_t)1 << 31)) return fail(-1, "cull_select: cap = %llu (at most 2^31)", (unsigned long long)cap);
  if (!work || !counters || (n && (!rows || !seen)) || (n && cap && !out_rows))
    return fail(-1, "cull_select: NULL argument (work and counters are required; rows and seen unless n is 0; out_rows unless n or cap is 0)");
  if (((uintptr_t)rows | (uintptr_t)out_rows) & 15) return fail(-1, "cull_select: rows and out_rows must be 16-byte aligned");
  if (((uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "cull_select: work and counters must be 8-byte aligned");
  if (((uintptr_t)seen | (uintptr_t)index_or_null) & 3) return fail(-1, "cull_select: seen and index must be 4-byte aligned");
  launch_cull_select(n, rows, seen, min_views, out_rows, cap, index_or_null, work, counters, (hipStream_t)stream);
  return check_launch("cull_select");
}

// ---- mesh cleaning (meshclean.hip) ------------------------------------------------------------------------------------------------------
static bool mesh_clean_sizes_ok(uint64_t V, uint64_t T) { return V <= NN_MAX_ROWS && T <= NN_MAX_ROWS; }
size_t mm3dgs_mesh_clean_work_bytes(uint64_t V, uint64_t T) { return mesh_clean_sizes_ok(V, T) ? mesh_clean_work_bytes(V, T) : 0; }

int mm3dgs_mesh_components(uint64_t V, uint64_t T, const int32_t* triangles, uint32_t* label, uint32_t* tri_count, uint64_t* counters, void* stream) {
  if (!mesh_clean_sizes_ok(V, T)) return fail(-1, "mesh_components: V = %llu, T = %llu (each at most 2^30)", (unsigned long long)V, (unsigned long long)T);
  if (!counters || (V && (!label || !tri_count)) || (T && !triangles))
    return fail(-1, "mesh_components: NULL argument (counters is required; label and tri_count unless V is 0; triangles unless T is 0)");
  if ((uintptr_t)counters & 7) return fail(-1, "mesh_components: counters must be 8-byte aligned");
  if (((uintptr_t)triangles | (uintptr_t)label | (uintptr_t)tri_count) & 3) return fail(-1, "mesh_components: triangles, label and tri_count must be 4-byte aligned");
  launch_mesh_components(V, T, triangles, label, tri_count, counters, (hipStream_t)stream);
  return check_launch("mesh_components");
}

int mm3dgs_mesh_clean_plan(uint64_t V, uint64_t T, const int32_t* triangles, const uint32_t* label, const uint32_t* tri_count, int mode, uint32_t min_triangles,
                           void* work, uint64_t* counters, void* stream) {
  if (!mesh_clean_sizes_ok(V, T)) return fail(-1, "mesh_clean_plan: V = %llu, T = %llu (each at most 2^30)", (unsigned long long)V, (unsigned long long)T);
  if (mode != MM3DGS_MESH_CLEAN_SMALL && mode != MM3DGS_MESH_CLEAN_LARGEST) return fail(-1, "mesh_clean_plan: mode = %d (1 small, 2 largest)", mode);
  if (mode == MM3DGS_MESH_CLEAN_SMALL && min_triangles < 1) return fail(-1, "mesh_clean_plan: min_triangles = 0 in mode small (at least 1)");
  if (!work || !counters || (V && (!label || !tri_count)) || (T && !triangles))
    return fail(-1, "mesh_clean_plan: NULL argument (work and counters are required; label and tri_count unless V is 0; triangles unless T is 0)");
  if (((uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "mesh_clean_plan: work and counters must be 8-byte aligned");
  if (((uintptr_t)triangles | (uintptr_t)label | (uintptr_t)tri_count) & 3) return fail(-1, "mesh_clean_plan: triangles, label and tri_count must be 4-byte aligned");
  launch_mesh_clean_plan(V, T, triangles, label, tri_count, mode, min_triangles, work, counters, (hipStream_t)stream);
  return check_launch("mesh_clean_plan");
}

int mm3dgs_mesh_clean_emit(uint64_t V, uint64_t T, const void* rows, const int32_t* triangles, const void* work, void* out_rows, uint64_t vcap,
                           int32_t* out_triangles, uint64_t tcap, uint32_t* index_or_null, uint64_t* counters, void* stream) {
  if (!mesh_clean_sizes_ok(V, T)) return fail(-1, "mesh_clean_emit: V = %llu, T = %llu (each at most 2^30)", (unsigned long long)V, (unsigned long long)T);
  if (vcap > ((uint64_t)1 << 31) || tcap > ((uint64_t)1 << 31))
    return fail(-1, "mesh_clean_emit: vcap = %llu, tcap = %llu (each at most 2^31)", (unsigned long long)vcap, (unsigned long long)tcap);
  if (!work || !counters || (V && !rows) || (T && !triangles) || (V && T && vcap && !out_rows) || (V && T && tcap && !out_triangles))
    return fail(-1, "mesh_clean_emit: NULL argument (work and counters are required; rows unless V is 0; triangles unless T is 0; out_rows and "
                    "out_triangles unless V, T or their cap is 0)");
  if (((uintptr_t)rows | (uintptr_t)out_rows) & 15) return fail(-1, "mesh_clean_emit: rows and out_rows must be 16-byte aligned");
  if (((uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "mesh_clean_emit: work and counters must be 8-byte aligned");
  if (((uintptr_t)triangles | (uintptr_t)out_triangles | (uintptr_t)index_or_null) & 3)
    return fail(-1, "mesh_clean_emit: triangles, out_triangles and index must be 4-byte aligned");
  launch_mesh_clean_emit(V, T, rows, triangles, work, out_rows, vcap, out_triangles, tcap, index_or_null, counters, (hipStream_t)stream);
  return check_launch("mesh_clean_emit");
}

// ---- mesh depth (meshdepth.hip) -----------------------------------------------------------------------------------------------------------
#define MD_MAX_PAIRS ((uint64_t)1 << 31)
static bool mesh_depth_sizes_ok(uint64_t V, uint64_t T, int H, int W, uint64_t max_pairs) {
  return V <= NN_MAX_ROWS && T <= NN_MAX_ROWS && H > 0 && W > 0 && eval_shape_ok(H, W) && max_pairs <= MD_MAX_PAIRS;
}
size_t mm3dgs_mesh_depth_work_bytes(uint64_t V, uint64_t T, int H, int W, uint64_t max_pairs) {
  return mesh_depth_sizes_ok(V, T, H, W, max_pairs) ? mesh_depth_work_bytes(V, T, H, W, max_pairs) : 0;
}

int mm3dgs_mesh_depth_render(int H, int W, double fx, double fy, double cx, double cy, const float* pose, double z_near, double z_far, uint64_t V,
                             const void* vrows, uint64_t T, const int32_t* triangles, uint64_t max_pairs, float* depth_out, int32_t* tri_out_or_null, void* work,
                             uint64_t* counters, void* stream) {
  MeshDepthView v;
  if (int rc = view_check("mesh_depth_render", H, W, fx, fy, cx, cy, pose, v)) return rc;
  if (V > NN_MAX_ROWS || T > NN_MAX_ROWS) return fail(-1, "mesh_depth_render: V = %llu, T = %llu (each at most 2^30)", (unsigned long long)V, (unsigned long long)T);
  if (max_pairs > MD_MAX_PAIRS) return fail(-1, "mesh_depth_render: max_pairs = %llu (at most 2^31)", (unsigned long long)max_pairs);
  if (!pose || !depth_out || !work || !counters || (V && !vrows) || (T && !triangles))
    return fail(-1, "mesh_depth_render: NULL argument (pose, depth_out, work and counters are required; vrows unless V is 0; triangles unless T is 0)");
  if (!(z_near >= 0.0) || !isfinite(z_near) || !(z_far >= 0.0) || !isfinite(z_far))
    return fail(-1, "mesh_depth_render: near = %g, far = %g (each must be finite and not negative)", z_near, z_far);
  if ((uintptr_t)vrows & 15) return fail(-1, "mesh_depth_render: vrows must be 16-byte aligned");
  if (((uintptr_t)work | (uintptr_t)counters) & 7) return fail(-1, "mesh_depth_render: work and counters must be 8-byte aligned");
  if (((uintptr_t)triangles | (uintptr_t)depth_out | (uintptr_t)tri_out_or_null | (uintptr_t)pose) & 3)
    return fail(-1, "mesh_depth_render: triangles, depth_out, tri_out and the pose must be 4-byte aligned");
  v.z_near = z_near; v.z_far = z_far;
  launch_mesh_depth_render(v, V, vrows, T, triangles, max_pairs, depth_out, tri_out_or_null, work, counters, (hipStream_t)stream);
  return check_launch("mesh_depth_render");
}

size_t mm3dgs_depth_compare_work_bytes(int H, int W) { return (H > 0 && W > 0 && eval_shape_ok(H, W)) ? depth_compare_work_bytes(H, W) : 0; }

int mm3dgs_depth_compare(int H, int W, const float* a, const float* b, void* work, double* row, void* stream) {
  if (H <= 0 || W <= 0) return fail(-1, "depth_compare: H = %d, W = %d (both must be positive)", H, W);
  if (!eval_shape_ok(H, W)) return fail(-1, "depth_compare: %d x %d has more than 2^28 pixels", H, W);
  if (!a || !b || !work || !row) return fail(-1, "depth_compare: NULL argument (a, b, work and row are required)");
  if (((uintptr_t)work | (uintptr_t)row) & 7) return fail(-1, "depth_compare: work and row must be 8-byte aligned");
  if (((uintptr_t)a | (uintptr_t)b) & 3) return fail(-1, "depth_compare: the images must be 4-byte aligned");
  launch_depth_compare(H, W, a, b, work, row, (hipStream_t)stream);
  return check_launch("depth_compare");
}

int mm3dgs_ingest_frame(int Hs, int Ws, const uint8_t* rgb, const uint16_t* depth_or_null, double png_depth_scale, int H, int W,
                        float* out_color, float* out_depth_or_null, void* stream) {
  if (Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return fail(-1, "ingest_frame: source %d x %d, output %d x %d (all must be positive)", Hs, Ws, H, W);
  if ((size_t)Hs * (size_t)Ws > ((size_t)1 << 30) || (size_t)H * (size_t)W > ((size_t)1 << 30))
    return fail(-1, "ingest_frame: source %d x %d or output %d x %d has more than 2^30 pixels", Hs, Ws, H, W);
  if (!rgb || !out_color) return fail(-1, "ingest_frame: NULL argument (rgb and out_color are required)");
  if ((depth_or_null != nullptr) != (out_depth_or_null != nullptr))
    return fail(-1, "ingest_frame: depth and out_depth must both be given or both be NULL");
  if (!(png_depth_scale > 0.0) || !isfinite(png_depth_scale)) return fail(-1, "ingest_frame: png_depth_scale = %g (must be finite and positive)", png_depth_scale);
  if (((uintptr_t)depth_or_null & 1) || (((uintptr_t)out_color | (uintptr_t)out_depth_or_null) & 3))
    return fail(-1, "ingest_frame: depth must be 2-byte aligned, out_color and out_depth 4-byte aligned");
  launch_ingest_frame(Hs, Ws, rgb, depth_or_null, png_depth_scale, H, W, out_color, out_depth_or_null, (hipStream_t)stream);
  return check_launch("ingest_frame");
}

int mm3dgs_ingest_est(int Hs, int Ws, const void* est, int dtype, double scale, int H, int W, float* out, void* stream) {
  if (Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return fail(-1, "ingest_est: source %d x %d, output %d x %d (all must be positive)", Hs, Ws, H, W);
  if ((size_t)Hs * (size_t)Ws > ((size_t)1 << 30) || (size_t)H * (size_t)W > ((size_t)1 << 30))
    return fail(-1, "ingest_est: source %d x %d or output %d x %d has more than 2^30 pixels", Hs, Ws, H, W);
  if (!est || !out) return fail(-1, "ingest_est: NULL argument (est and out are required)");
  if (dtype < 0 || dtype > 2) return fail(-1, "ingest_est: dtype = %d (0 float32, 1 float16, 2 uint16)", dtype);
  if (!(scale > 0.0) || !isfinite(scale)) return fail(-1, "ingest_est: scale = %g (must be finite and positive)", scale);
  if (((uintptr_t)est & (dtype == 0 ? 3 : 1)) || ((uintptr_t)out & 3))
    return fail(-1, "ingest_est: est must be aligned to its element size (%d bytes), out to 4 bytes", dtype == 0 ? 4 : 2);
  launch_ingest_est(Hs, Ws, est, dtype, scale, H, W, out, (hipStream_t)stream);
  return check_launch("ingest_est");
}

static bool mosaic_shape_ok(int H, int W, int rows, int cols) {
  return H > 0 && W > 0 && rows > 0 && cols > 0 && rows * (long long)cols <= MOSAIC_MAX_PANELS &&
         (size_t)rows * (size_t)H * (size_t)cols * (size_t)W <= ((size_t)1 << 28);
}

size_t mm3dgs_mosaic_work_bytes(int H, int W, int rows, int cols) { return mosaic_shape_ok(H, W, rows, cols) ? mosaic_work_bytes(rows, cols) : 0; }

int mm3dgs_mosaic(int H, int W, int rows, int cols, const int32_t* kind, const float* const* a, const float* const* b, const uint8_t* lut, int quant,
                  int bgr, void* work, uint8_t* out, void* stream) {
  if (H <= 0 || W <= 0 || rows <= 0 || cols <= 0) return fail(-1, "mosaic: %d x %d panels of %d x %d (all must be positive)", rows, cols, H, W);
  if (!mosaic_shape_ok(H, W, rows, cols))
    return fail(-1, "mosaic: %d x %d panels of %d x %d (at most %d panels and 2^28 pixels)", rows, cols, H, W, MOSAIC_MAX_PANELS);
  if (!kind || !a || !work || !out) return fail(-1, "mosaic: NULL argument (kind, a, work and out are required)");
  if (quant != 0 && quant != 1) return fail(-1, "mosaic: quant = %d (0 truncate, 1 round)", quant);
  if ((uintptr_t)work & 7) return fail(-1, "mosaic: work must be 8-byte aligned");
  MosaicPanels panels = {};
  for (int p = 0; p < rows * cols; p++) {
    if (kind[p] < 0 || kind[p] > 2) return fail(-1, "mosaic: panel %d has kind %d (0 colour, 1 absolute difference, 2 depth)", p, kind[p]);
    if (!a[p] || (kind[p] == 1 && !(b && b[p]))) return fail(-1, "mosaic: panel %d (kind %d) has a NULL image", p, kind[p]);
    if (kind[p] == 2 && !lut) return fail(-1, "mosaic: panel %d is a depth panel and lut is NULL", p);
    if (((uintptr_t)a[p] & 3) || (kind[p] == 1 && ((uintptr_t)b[p] & 3))) return fail(-1, "mosaic: panel %d has an image that is not 4-byte aligned", p);
    panels.kind[p] = kind[p];
    panels.a[p] = a[p];
    panels.b[p] = kind[p] == 1 ? b[p] : nullptr;
  }
  launch_mosaic(H, W, rows, cols, panels, lut, quant, bgr != 0, work, out, (hipStream_t)stream);
  return check_launch("mosaic");
}

int mm3dgs_prune_mask(int P, const float* opacity, const float* log_scales, const float* max_radii2D, float min_opacity, float max_scale,
                      float max_screen_size, uint8_t* keep, uint32_t* n_pruned_accum, void* stream) {
  if (P < 0) return fail(-1, "P < 0");
  if (P > 0 && (!opacity || !log_scales || !keep || !n_pruned_accum)) return fail(-1, "NULL argument");
  launch_prune_mask(P, opacity, log_scales, max_radii2D, min_opacity, max_scale, max_screen_size, max_radii2D ? 1 : 0, keep, n_pruned_accum,
                    (hipStream_t)stream);
  return check_launch("prune_mask");
}
size_t mm3dgs_compact_work_bytes(size_t n) { size_t b; compact_work(nullptr, n, &b); return b; }
int mm3dgs_compact_plan(size_t n, const uint8_t* keep, void* work, uint32_t* n_keep, void* stream) {
  if (n > 0x7fffffffull) return fail(-1, "n too large");
  if (!work || !n_keep || (n > 0 && !keep)) return fail(-1, "NULL argument");
  launch_compact_plan((int)n, keep, compact_work(work, n), n_keep, (hipStream_t)stream);
  return check_launch("compact_plan");
}
int mm3dgs_compact_rows(size_t n, const uint8_t* keep, const void* work, const Mm3dgsCompactArray* arrays, int n_arrays, void* stream) {
  if (n > 0x7fffffffull) return fail(-1, "n too large");
  if (n_arrays < 0 || n_arrays > 32) return fail(-1, "at most 32 arrays per call");
  if (n > 0 && (!keep || !work || (n_arrays > 0 && !arrays))) return fail(-1, "NULL argument");
  CompactTable t;
  t.n_arrays = 0;
  for (int a = 0; a < n_arrays; a++) {
    if (arrays[a].width < 0) return fail(-1, "array %d: negative width", a);
    if (arrays[a].width == 0) continue;     // empty rows (e.g. f_rest at SH degree 0)
    if (!arrays[a].src || !arrays[a].dst) return fail(-1, "array %d: NULL pointer", a);
    t.src[t.n_arrays] = arrays[a].src; t.dst[t.n_arrays] = arrays[a].dst; t.width[t.n_arrays] = arrays[a].width; t.n_arrays++;
  }
  launch_compact_rows((int)n, keep, compact_work(work, n), t, (hipStream_t)stream);
  return check_launch("compact_rows");
}
int mm3dgs_seed_gaussians(int H, int W, const float* color, const float* depth, const uint8_t* keep, const void* work, const float* pose, float fx,
                          float fy, float cx, float cy, uint32_t row0, const Mm3dgsSeedOutputs* out, int n_rest, void* stream) {
  if (H <= 0 || W <= 0 || (double)H * W > 2147483647.0) return fail(-1, "bad image size");
  if (!color || !depth || !keep || !work || !pose || !out) return fail(-1, "NULL argument");
  if (!out->xyz || !out->f_dc || !out->opacity || !out->scaling || !out->rotation || !out->rgb || (n_rest > 0 && !out->f_rest))
    return fail(-1, "NULL output array");
  SeedOut o = {out->xyz, out->f_dc, out->f_rest, out->opacity, out->scaling, out->rotation, out->rgb, n_rest > 0 ? n_rest : 0};
  launch_seed_gaussians(H, W, color, depth, keep, compact_work(work, (size_t)H * (size_t)W), pose, fx, fy, cx, cy, row0, o, (hipStream_t)stream);
  return check_launch("seed_gaussians");
}

// densification (slam/gaussian_model.py:490-592)
size_t mm3dgs_densify_work_bytes(size_t P) { uint8_t* cls; size_t b; densify_work(nullptr, P, cls, &b); return b; }
int mm3dgs_densify_plan(size_t P, const float* grad_accum, const float* denom, const float* log_scales, float max_grad, float max_clone_scale,
                        void* work, uint32_t* counts, void* stream) {
  if (P > 0x7fffffffull) return fail(-1, "P too large");
  if (!work || !counts || (P > 0 && (!grad_accum || !denom || !log_scales))) return fail(-1, "NULL argument");
  uint8_t* cls;
  uint32_t* block_counts = densify_work(work, P, cls);
  launch_densify_plan((int)P, grad_accum, denom, log_scales, max_grad, max_clone_scale, cls, block_counts, counts, (hipStream_t)stream);
  return check_launch("densify_plan");
}
int mm3dgs_densify_rows(size_t P, const void* work, uint32_t n_keep, uint32_t n_clone, uint32_t n_split, int N, uint32_t seed,
                        const Mm3dgsDensifyState* st, void* stream) {
  if (P > 0x7fffffffull) return fail(-1, "P too large");
  if (N < 1 || N > 64) return fail(-1, "N out of range");
  // (the destination rows are placed by these counts: they must be the plan's)
  if ((uint64_t)n_keep + n_split != P || n_clone > n_keep) return fail(-1, "counts do not describe a plan of %zu rows", P);
  if ((uint64_t)n_keep + n_clone + (uint64_t)N * n_split > 0x7fffffffull) return fail(-1, "densified map too large");
  if (P == 0) return 0;
  if (!work || !st || !st->grad_accum || !st->denom || !st->max_radii2D) return fail(-1, "NULL argument");
  DensifyTable t = {};
  for (int a = 0; a < 7; a++) {
    const Mm3dgsDensifyGroup& g = st->group[a];
    if (g.width < 0) return fail(-1, "group %d: negative width", a);
    if (g.width > 0 && (!g.src || !g.dst)) return fail(-1, "group %d: NULL pointer", a);
    if ((g.m_dst && !g.m_src) || (g.v_dst && !g.v_src)) return fail(-1, "group %d: moment destination without source", a);
    t.src[a] = g.src; t.dst[a] = g.dst; t.m_src[a] = g.m_src; t.m_dst[a] = g.m_dst; t.v_src[a] = g.v_src; t.v_dst[a] = g.v_dst; t.width[a] = g.width;
  }
  if (n_split > 0 && (t.width[0] != 3 || t.width[4] != 3 || t.width[5] != 4)) return fail(-1, "split needs xyz[3], scaling[3], rotation[4]");
  t.grad_accum = st->grad_accum; t.denom = st->denom; t.max_radii2D = st->max_radii2D; t.parent = st->parent;
  uint8_t* cls;
  uint32_t* block_counts = densify_work(work, P, cls);
  launch_densify_rows((int)P, cls, block_counts, n_keep, n_clone, n_split, N, seed, (float)(0.8 * (double)N), t, (hipStream_t)stream);
  return check_launch("densify_rows");
}

int mm3dgs_mark_visible(const Mm3dgsCamera* cam, int P, const float* means3D, uint8_t* visible, void* stream) {
  if (!cam || !cam->viewmatrix || (P > 0 && (!means3D || !visible))) return fail(-1, "NULL buffer");
  launch_mark_visible(cam_dev(cam), P, means3D, visible, (hipStream_t)stream);
  return check_launch("mark_visible");
}

}  // extern "C"

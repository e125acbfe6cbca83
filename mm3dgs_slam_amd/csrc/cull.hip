// Visibility culling of a point set against the views of a run (mm3dgs_cull_mark_view / mm3dgs_cull_work_bytes / mm3dgs_cull_select; host
// statement: cull.cull_host).  Rows are the cloud's 16-byte rows {float x, y, z; uint32 rgba}; seen is one uint32 per row, zeroed by the caller.
//
//   cull_mark_kernel     one launch per view, one lane per row and step, a workgroup walking 8 steps of 256 consecutive rows.  One lane per
//                        workgroup builds the Rigid into LDS.  A lane loads its row once and walks the rule in double through view_pixel.h's
//                        statements (the ones tsdf_sample.h calls): finite, z_c > near, z_c <= far (far > 0), the pixel inside the image, and with
//                        a depth image the pixel's validity (no silhouette) and z_c <= (double)d + eps.  Only a row that is seen touches the
//                        depth image (one scattered 4-byte load) and seen[i] (plain load, add, store: the row belongs to this lane and views are
//                        ordered on the stream).  Counters: [0] views, [1] sightings -- one integer add per workgroup (tsdf.hip's header: one
//                        per wave on one word is what a view cost there).  The adds all land on one word and are what bounds the launch: with
//                        one step per workgroup (3907 adds at 10^6 rows) a view took 54.7 us in either mode and at either image size, 14 ns
//                        per add, the 16 MB of rows nowhere near a memory rate; hence the 8 steps (profiles/r17_cull.jsonl).
//   cull_count_kernel    per 256 rows: kept rows (finite and seen >= min_views) and skipped rows (a coordinate that is not finite).
//   cull_scan_kernel     one workgroup of 1024: the skipped total, scan_block_counts over the kept counts, counters [2..7].
//   cull_scatter_kernel  kept rows to out_rows / index at block prefix + block_rank, below cap.  No atomic decides a position: the same inputs
//                        give the same bytes on every call.
#include <math.h>
#include "block_ops.h"
#include "fused_api.h"
#include "view_pixel.h"

#define CB 256
#define CULL_CHUNKS 8      // 256-row steps per workgroup of the mark kernel: one add per 2048 rows on the sightings word (see below)

static size_t cull_nb(size_t n) { return (n + CB - 1) / CB; }

// work = [uint32 kept rows per 256][uint32 skipped rows per 256] (at least one word each: n = 0 is a valid size)
struct CullWork { uint32_t* kcounts; uint32_t* scounts; };
static CullWork cull_work(void* base, size_t n, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  CullWork w;
  const size_t nb = cull_nb(n) ? cull_nb(n) : 1;
  w.kcounts = c.take<uint32_t>(nb);
  w.scounts = c.take<uint32_t>(nb);
  if (bytes) *bytes = c.at;
  return w;
}
size_t cull_work_bytes(uint64_t n) { size_t b; cull_work(nullptr, (size_t)n, &b); return b; }

__global__ void __launch_bounds__(CB)
cull_mark_kernel(CullView v, const uint4* __restrict__ rows, uint32_t n, uint32_t* __restrict__ seen, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  __shared__ Rigid g;
  __shared__ uint32_t wcnt[1][CB / 64];
  view_rigid_shared(v.pose, g);
  uint32_t nhit = 0;
  for (int k = 0; k < CULL_CHUNKS; k++) {      // 256 consecutive rows per step: every load of a wave is one contiguous KiB
    const size_t i = ((size_t)blockIdx.x * CULL_CHUNKS + k) * CB + threadIdx.x;
    if (i >= n) break;
    const uint4 r = rows[i];      // one 16-byte load
    const float xf = __uint_as_float(r.x), yf = __uint_as_float(r.y), zf = __uint_as_float(r.z);
    if (!view_finite(xf, yf, zf)) continue;
    double x, y, z;
    size_t pix;
    view_to_camera(g, (double)xf, (double)yf, (double)zf, x, y, z);      // (x and y are needed only behind the test of z)
    if (!(z > v.z_near) || (v.z_far > 0.0 && !(z <= v.z_far))) continue;      // (a NaN fails the first test)
    if (!view_pixel_index(v, x, y, z, pix)) continue;
    if (v.depth) {      // occlusion: a hole in the depth image sees nothing
      float d;
      if (!view_pixel_valid(v.depth, nullptr, 0.f, v.depth_max, pix, d) || !(z <= (double)d + v.eps)) continue;
    }
    seen[i] = seen[i] + 1u;
    nhit++;
  }
  const uint32_t nn[1] = {nhit};
  const uint32_t t = block_sums_u32(nn, wcnt);      // (every lane is here)
  if (threadIdx.x == 0 && t) atomicAdd(counters + 1, (unsigned long long)t);
  if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(counters, 1ull);
}

void launch_cull_mark_view(const CullView& v, uint64_t n, const void* rows, uint32_t* seen, uint64_t* counters, hipStream_t s) {
  const size_t per = (size_t)CB * CULL_CHUNKS;
  const size_t nb = n ? ((size_t)n + per - 1) / per : 1;      // n = 0: the view is still counted
  hipLaunchKernelGGL(cull_mark_kernel, dim3((unsigned)nb), dim3(CB), 0, s, v, (const uint4*)rows, (uint32_t)n, seen, (unsigned long long*)counters);
}

// kept / skipped of row i (i < n)
__device__ __forceinline__ bool cull_kept(const uint4* __restrict__ rows, const uint32_t* __restrict__ seen, uint32_t min_views, uint32_t i, uint4& r, bool& skipped) {
  r = rows[i];
  skipped = !view_finite(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z));
  return !skipped && seen[i] >= min_views;
}

__global__ void __launch_bounds__(CB)
cull_count_kernel(const uint4* __restrict__ rows, const uint32_t* __restrict__ seen, uint32_t n, uint32_t min_views, uint32_t* __restrict__ kcounts,
                  uint32_t* __restrict__ scounts) {
  __shared__ uint32_t wcnt[2][CB / 64];
  const uint32_t i = blockIdx.x * CB + threadIdx.x;
  bool kept = false, skipped = false;
  uint4 r;
  if (i < n) kept = cull_kept(rows, seen, min_views, i, r, skipped);
  const bool is[2] = {kept, skipped};
  const uint32_t t = block_flag_counts(is, wcnt);
  if (threadIdx.x == 0) kcounts[blockIdx.x] = t;
  if (threadIdx.x == 1) scounts[blockIdx.x] = t;
}

__global__ void __launch_bounds__(1024)
cull_scan_kernel(int nb, uint32_t* __restrict__ kcounts, const uint32_t* __restrict__ scounts, unsigned long long cap, unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long sh[16];
  __shared__ uint32_t kept;
  const unsigned long long skipped = block_array_sum(nb, scounts, sh);
  scan_block_counts(nb, kcounts, &kept);
  if (threadIdx.x == 0) {      // (lane 0 wrote `kept` itself)
    const unsigned long long k = kept, written = k < cap ? k : cap;
    counters[2] = k;
    counters[3] = written;
    counters[4] = k - written;
    counters[5] = skipped;
    counters[6] = 0ull;
    counters[7] = 0ull;
  }
}

__global__ void __launch_bounds__(CB)
cull_scatter_kernel(const uint4* __restrict__ rows, const uint32_t* __restrict__ seen, uint32_t n, uint32_t min_views, const uint32_t* __restrict__ kpre,
                    unsigned long long cap, uint4* __restrict__ out_rows, uint32_t* __restrict__ index) {
  __shared__ uint32_t wsum[CB / 64];
  const uint32_t i = blockIdx.x * CB + threadIdx.x;
  bool kept = false, skipped = false;
  uint4 r;
  if (i < n) kept = cull_kept(rows, seen, min_views, i, r, skipped);
  const uint32_t pos = block_rank(kept, kpre[blockIdx.x], wsum);      // (every lane is here)
  if (kept && (unsigned long long)pos < cap) {
    out_rows[pos] = r;      // one 16-byte store
    if (index) index[pos] = i;
  }
}

void launch_cull_select(uint64_t n, const void* rows, const uint32_t* seen, uint32_t min_views, void* out_rows, uint64_t cap, uint32_t* index, void* work,
                        uint64_t* counters, hipStream_t s) {
  const CullWork w = cull_work(work, (size_t)n);
  const unsigned nb = (unsigned)cull_nb((size_t)n);
  if (nb) hipLaunchKernelGGL(cull_count_kernel, dim3(nb), dim3(CB), 0, s, (const uint4*)rows, seen, (uint32_t)n, min_views, w.kcounts, w.scounts);
  hipLaunchKernelGGL(cull_scan_kernel, dim3(1), dim3(1024), 0, s, (int)nb, w.kcounts, w.scounts, (unsigned long long)cap, (unsigned long long*)counters);
  if (nb) hipLaunchKernelGGL(cull_scatter_kernel, dim3(nb), dim3(CB), 0, s, (const uint4*)rows, seen, (uint32_t)n, min_views, w.kcounts, (unsigned long long)cap,
                             (uint4*)out_rows, index);
}

// A triangle mesh rendered to a depth image from a camera, and the comparison of two depth images (mm3dgs_mesh_depth_work_bytes /
// mm3dgs_mesh_depth_render / mm3dgs_depth_compare_work_bytes / mm3dgs_depth_compare; host statement: mesh_depth.render_host /
// compare_rows_host).  Vertex rows are the cloud's 16-byte rows {float x, y, z; uint32 rgba}, triangles int32 [T][3].  The rule is homogeneous
// rasterization in double, no contraction: edge normals n0 = b x c, n1 = c x a, n2 = a x b and det = a . n0 from the camera-space corners, per
// pixel E_i = n_i . (dx, dy, 1), S = E0 + E1 + E2, inside when the three E_i share S's sign, z = det / S -- no clipping at the camera plane.
//
// One view is five launches on the caller's stream:
//   md_vertex_kernel    one lane per vertex: p_c (3 doubles, view_to_camera) to the work buffer; the same lanes zero the tile counts, cursors.
//   md_setup_kernel     one lane per triangle: invalid / behind / drawn (block_flag_counts, one add per workgroup and class), the setup
//                       record (n0, n1, n2, det: 80 B) and the pixel rectangle -- floor(min) - 1 .. ceil(max) + 1 of the projections when
//                       all three corners lie in front and project finitely, else the whole image: only ever a superset of the hits --,
//                       kept as a rectangle of 16 x 16-pixel tiles, with one integer atomicAdd per touched tile on that tile's count (a
//                       rectangle of more than 32 tiles is walked by its whole wave: md_for_tiles).
//   md_scan_kernel      one workgroup of 1024: the pair total (64-bit) and scan_block_counts over the tile counts; counters [4] [5].
//   md_scatter_kernel   one lane per triangle: a slot in each touched tile's list through the tile's cursor (atomicAdd), below max_pairs.
//   md_raster_kernel    one workgroup of 256 per tile, one lane per pixel: the tile's list in batches of 256 records staged through LDS
//                       (20 KB), (z, index) in registers, one 4-byte store per output image.  No atomic touches a pixel, and a tile with
//                       an empty list writes its zeros: the caller clears nothing.
// The order inside a tile's list depends on the order the atomics arrive in.  The images do not: a pixel takes the minimum over (z, index),
// which is order-free.  Counts are integers.  So the same inputs give the same bytes on every call.
//
//   dc_pixel_kernel     per 256 pixels one partial row: sum |a - b|, sum of squares (block_sums_f64's tree), max, and the four counts.
//   dc_finish_kernel    one workgroup: lane t adds the partial rows t, t + 256, ... in order, the 256 lanes are added in order
//                       (geometry.kernel_order_sum states this order); no float atomic anywhere.
#include <math.h>
#include "block_ops.h"
#include "fused_api.h"
#include "view_pixel.h"

#define MB 256
#define MD_TILE 16
#define MD_REC 10      // doubles of a setup record: n0, n1, n2, det

static size_t md_nb(size_t n) { return (n + MB - 1) / MB; }
static size_t md_tiles(int H, int W) { return (size_t)((W + MD_TILE - 1) / MD_TILE) * (size_t)((H + MD_TILE - 1) / MD_TILE); }

// work = [3 doubles per vertex][10 doubles per triangle][int4 tile rectangle per triangle][uint32 per tile + 1: counts, then offsets]
//        [uint32 cursor per tile][uint32 per pair] (at least one element each: V = 0, T = 0 and max_pairs = 0 are valid sizes)
struct MdWork { double* pc; double* rec; int4* rect; uint32_t* counts; uint32_t* cursor; uint32_t* pairs; };
static MdWork md_work(void* base, size_t V, size_t T, size_t ntiles, size_t max_pairs, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  MdWork w;
  w.pc = c.take<double>(3 * (V ? V : 1));
  w.rec = c.take<double>(MD_REC * (T ? T : 1));
  w.rect = c.take<int4>(T ? T : 1);
  w.counts = c.take<uint32_t>(ntiles + 1);
  w.cursor = c.take<uint32_t>(ntiles);
  w.pairs = c.take<uint32_t>(max_pairs ? max_pairs : 1);
  if (bytes) *bytes = c.at;
  return w;
}
size_t mesh_depth_work_bytes(uint64_t V, uint64_t T, int H, int W, uint64_t max_pairs) {
  size_t b;
  md_work(nullptr, (size_t)V, (size_t)T, md_tiles(H, W), (size_t)max_pairs, &b);
  return b;
}

__device__ __forceinline__ bool md_finite(double x) { return fabs(x) < (double)INFINITY; }

__global__ void __launch_bounds__(MB)
md_vertex_kernel(MeshDepthView v, const uint4* __restrict__ vrows, uint32_t V, double* __restrict__ pc, uint32_t ntiles, uint32_t* __restrict__ counts,
                 uint32_t* __restrict__ cursor) {
#pragma clang fp contract(off)
  __shared__ Rigid g;
  view_rigid_shared(v.pose, g);
  const size_t i = (size_t)blockIdx.x * MB + threadIdx.x;
  if (i <= ntiles) counts[i] = 0u;
  if (i < ntiles) cursor[i] = 0u;
  if (i >= V) return;
  const uint4 r = vrows[i];      // one 16-byte load
  double c[3];
  view_to_camera(g, (double)__uint_as_float(r.x), (double)__uint_as_float(r.y), (double)__uint_as_float(r.z), c[0], c[1], c[2]);
  for (int k = 0; k < 3; k++) pc[3 * i + k] = c[k];
}

__device__ __forceinline__ void md_cross(const double* u, const double* w, double* o) {
#pragma clang fp contract(off)
  o[0] = u[1] * w[2] - u[2] * w[1];
  o[1] = u[2] * w[0] - u[0] * w[2];
  o[2] = u[0] * w[1] - u[1] * w[0];
}

// the clamped pixel range of one axis from the three projections: lo .. hi inclusive, hi < lo when nothing of the image is left
__device__ __forceinline__ void md_range(double p0, double p1, double p2, int size, int& lo, int& hi) {
  double mn = p0 < p1 ? p0 : p1, mx = p0 > p1 ? p0 : p1;
  mn = mn < p2 ? mn : p2;
  mx = mx > p2 ? mx : p2;
  double a = floor(mn) - 1.0, b = ceil(mx) + 1.0;
  a = a < 0.0 ? 0.0 : (a > (double)size ? (double)size : a);      // clamped in double: a projection may lie beyond any int
  b = b > (double)(size - 1) ? (double)(size - 1) : (b < -1.0 ? -1.0 : b);
  lo = (int)a;
  hi = (int)b;
}

// f(tile, triangle) once per tile of this lane's tile rectangle (empty: none); every lane of the wave calls.  A rectangle of more than 32
// tiles is spread over the whole wave (broadcast with readlane, as sweep_rect does for a huge splat): a wall-sized triangle, or one that
// crosses the camera plane, touches every tile of the image, and one lane walking them made a view of a 12-triangle room 664 us at
// 640x480 and 1577 us at 1200x680 (profiles/r19_mesh_depth.jsonl has the figures since)
template <typename F>
__device__ __forceinline__ void md_for_tiles(int4 tr, uint32_t t, int gx, F f) {
  const int w = tr.z - tr.x + 1, h = tr.w - tr.y + 1, area = (w > 0 && h > 0) ? w * h : 0, lane = threadIdx.x & 63;
  unsigned long long big = __ballot(area > 32);
  if (area > 0 && area <= 32)
    for (int ty = tr.y; ty <= tr.w; ty++)
      for (int tx = tr.x; tx <= tr.z; tx++) f((size_t)ty * gx + tx, t);
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    const int sx = __builtin_amdgcn_readlane(tr.x, src), sy = __builtin_amdgcn_readlane(tr.y, src), sw = __builtin_amdgcn_readlane(w, src);
    const int sarea = __builtin_amdgcn_readlane(area, src);
    const uint32_t st = __builtin_amdgcn_readlane(t, src);
    for (int k = lane; k < sarea; k += 64) f((size_t)(sy + k / sw) * gx + sx + k % sw, st);
  }
}

__global__ void __launch_bounds__(MB)
md_setup_kernel(MeshDepthView v, const double* __restrict__ pc, uint32_t V, const int* __restrict__ tris, uint32_t T, double* __restrict__ rec,
                int4* __restrict__ rect, int gx, uint32_t* __restrict__ counts, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  __shared__ uint32_t wcnt[3][MB / 64];
  const size_t t = (size_t)blockIdx.x * MB + threadIdx.x;
  bool drawn = false, invalid = false, behind = false;
  int4 tr = make_int4(0, 0, -1, -1);      // tiles x0, y0 .. x1, y1 inclusive; empty unless drawn
  if (t < T) {
    const int ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
    double a[3], b[3], c[3];
    invalid = !((uint32_t)ia < V && (uint32_t)ib < V && (uint32_t)ic < V);      // (a negative index is a uint32 above 2^31, V at most 2^30)
    if (!invalid) {
      for (int k = 0; k < 3; k++) { a[k] = pc[3 * (size_t)ia + k]; b[k] = pc[3 * (size_t)ib + k]; c[k] = pc[3 * (size_t)ic + k]; }
      for (int k = 0; k < 3; k++) invalid = invalid || !md_finite(a[k]) || !md_finite(b[k]) || !md_finite(c[k]);
    }
    if (!invalid) {
      behind = !(a[2] > v.z_near || b[2] > v.z_near || c[2] > v.z_near);
      drawn = !behind;
    }
    if (drawn) {
      double n0[3], n1[3], n2[3];
      md_cross(b, c, n0);
      md_cross(c, a, n1);
      md_cross(a, b, n2);
      const double det = a[0] * n0[0] + a[1] * n0[1] + a[2] * n0[2];
      double* o = rec + (size_t)MD_REC * t;
      for (int k = 0; k < 3; k++) { o[k] = n0[k]; o[3 + k] = n1[k]; o[6 + k] = n2[k]; }
      o[9] = det;
      int x0 = 0, y0 = 0, x1 = v.W - 1, y1 = v.H - 1;      // the whole image unless all three corners project
      if (a[2] > 0.0 && b[2] > 0.0 && c[2] > 0.0) {      // the unrounded projection bounds a rectangle: not view_pixel_index's nearest pixel (no + 0.5, no floor)
        const double pxa = v.fx * a[0] / a[2] + v.cx, pxb = v.fx * b[0] / b[2] + v.cx, pxc = v.fx * c[0] / c[2] + v.cx;
        const double pya = v.fy * a[1] / a[2] + v.cy, pyb = v.fy * b[1] / b[2] + v.cy, pyc = v.fy * c[1] / c[2] + v.cy;
        if (md_finite(pxa) && md_finite(pxb) && md_finite(pxc) && md_finite(pya) && md_finite(pyb) && md_finite(pyc)) {
          md_range(pxa, pxb, pxc, v.W, x0, x1);
          md_range(pya, pyb, pyc, v.H, y0, y1);
        }
      }
      if (x0 <= x1 && y0 <= y1) tr = make_int4(x0 / MD_TILE, y0 / MD_TILE, x1 / MD_TILE, y1 / MD_TILE);      // (0 <= x0 <= x1 < W here)
    }
    rect[t] = tr;
  }
  const bool is[3] = {drawn, invalid, behind};
  const uint32_t n = block_flag_counts(is, wcnt);      // (every lane is here)
  if (threadIdx.x < 3 && n) atomicAdd(counters + 1 + threadIdx.x, (unsigned long long)n);
  if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(counters, 1ull);
  md_for_tiles(tr, (uint32_t)t, gx, [&](size_t tile, uint32_t) { atomicAdd(&counts[tile], 1u); });      // (every lane is here)
}

__global__ void __launch_bounds__(1024)
md_scan_kernel(int ntiles, uint32_t* __restrict__ counts, unsigned long long max_pairs, unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long sh[16];
  __shared__ uint32_t total;
  const unsigned long long need = block_array_sum(ntiles, counts, sh);      // 64-bit: T triangles over every tile may pass 2^32
  scan_block_counts(ntiles, counts, &total);
  if (threadIdx.x == 0) {      // (lane 0 wrote `total` itself)
    counts[ntiles] = total;      // the end of the last list (modulo 2^32, as the offsets are: see md_raster_kernel)
    const unsigned long long pairs = need < max_pairs ? need : max_pairs;
    counters[4] += pairs;
    counters[5] += need - pairs;
  }
}

__global__ void __launch_bounds__(MB)
md_scatter_kernel(uint32_t T, const int4* __restrict__ rect, int gx, const uint32_t* __restrict__ offs, uint32_t* __restrict__ cursor,
                  uint32_t* __restrict__ pairs, unsigned long long max_pairs) {
  const size_t t = (size_t)blockIdx.x * MB + threadIdx.x;
  const int4 tr = t < T ? rect[t] : make_int4(0, 0, -1, -1);
  md_for_tiles(tr, (uint32_t)t, gx, [&](size_t tile, uint32_t tri) {      // (every lane is here)
    const unsigned long long slot = (unsigned long long)offs[tile] + atomicAdd(&cursor[tile], 1u);
    if (slot < max_pairs) pairs[slot] = tri;      // the rest is counted as dropped (md_scan_kernel)
  });
}

__global__ void __launch_bounds__(MB)
md_raster_kernel(MeshDepthView v, int gx, const uint32_t* __restrict__ offs, const uint32_t* __restrict__ pairs, unsigned long long max_pairs,
                 const double* __restrict__ rec, uint32_t T, float* __restrict__ depth, int* __restrict__ tri, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  __shared__ double srec[MB][MD_REC];
  __shared__ uint32_t sidx[MB];
  __shared__ uint32_t wcnt[1][MB / 64];
  const int tile = blockIdx.x, u = (tile % gx) * MD_TILE + (threadIdx.x & (MD_TILE - 1)), vv = (tile / gx) * MD_TILE + (threadIdx.x >> 4);
  const double dx = ((double)u - v.cx) / v.fx, dy = ((double)vv - v.cy) / v.fy;
  // the list [begin, begin + count) cut at max_pairs; with more than 2^32 pairs in all the offsets have wrapped: every read stays below
  // max_pairs and every index below T (a slot nothing wrote may hold anything), and counters[5] tells the caller the image is void
  const unsigned long long begin = offs[tile], count = (uint32_t)(offs[tile + 1] - offs[tile]);
  const unsigned long long end = begin + count < max_pairs ? begin + count : max_pairs;
  double bz = (double)INFINITY;
  uint32_t bi = 0xffffffffu;
  for (unsigned long long base = begin; base < end; base += MB) {
    __syncthreads();      // (the previous batch has been read)
    const unsigned long long k = base + threadIdx.x;
    if (k < end) {
      const uint32_t t = pairs[k];
      sidx[threadIdx.x] = t < T ? t : 0xffffffffu;
      if (t < T)
        for (int j = 0; j < MD_REC; j++) srec[threadIdx.x][j] = rec[(size_t)MD_REC * t + j];
    }
    __syncthreads();
    const int m = end - base < MB ? (int)(end - base) : MB;
    for (int j = 0; j < m; j++) {
      const uint32_t t = sidx[j];      // (the same address in every lane: a broadcast)
      if (t == 0xffffffffu) continue;
      const double* r = srec[j];
      const double E0 = r[0] * dx + r[1] * dy + r[2], E1 = r[3] * dx + r[4] * dy + r[5], E2 = r[6] * dx + r[7] * dy + r[8];
      const double S = E0 + E1 + E2;
      const bool inside = (E0 >= 0.0 && E1 >= 0.0 && E2 >= 0.0 && S > 0.0) || (E0 <= 0.0 && E1 <= 0.0 && E2 <= 0.0 && S < 0.0);
      if (!inside) continue;
      const double z = r[9] / S;
      if (!md_finite(z) || !(z > v.z_near) || (v.z_far > 0.0 && !(z <= v.z_far))) continue;
      if (z < bz || (z == bz && t < bi)) { bz = z; bi = t; }
    }
  }
  const bool hit = bi != 0xffffffffu && u < v.W && vv < v.H;
  if (u < v.W && vv < v.H) {
    const size_t pix = (size_t)vv * v.W + u;
    depth[pix] = hit ? (float)bz : 0.f;      // the one rounding
    if (tri) tri[pix] = hit ? (int)bi : -1;
  }
  const bool is[1] = {hit};
  const uint32_t n = block_flag_counts(is, wcnt);      // (every lane is here)
  if (threadIdx.x == 0 && n) atomicAdd(counters + 6, (unsigned long long)n);
}

void launch_mesh_depth_render(const MeshDepthView& v, uint64_t V, const void* vrows, uint64_t T, const int* tris, uint64_t max_pairs, float* depth, int* tri,
                              void* work, uint64_t* counters, hipStream_t s) {
  const size_t ntiles = md_tiles(v.H, v.W);
  const int gx = (v.W + MD_TILE - 1) / MD_TILE;
  const MdWork w = md_work(work, (size_t)V, (size_t)T, ntiles, (size_t)max_pairs);
  unsigned long long* c = (unsigned long long*)counters;
  const size_t first = (size_t)V > ntiles + 1 ? (size_t)V : ntiles + 1;
  const unsigned nbt = (unsigned)(T ? md_nb((size_t)T) : 1);      // T = 0: the view is still counted
  hipLaunchKernelGGL(md_vertex_kernel, dim3((unsigned)md_nb(first)), dim3(MB), 0, s, v, (const uint4*)vrows, (uint32_t)V, w.pc, (uint32_t)ntiles, w.counts, w.cursor);
  hipLaunchKernelGGL(md_setup_kernel, dim3(nbt), dim3(MB), 0, s, v, (const double*)w.pc, (uint32_t)V, tris, (uint32_t)T, w.rec, w.rect, gx, w.counts, c);
  hipLaunchKernelGGL(md_scan_kernel, dim3(1), dim3(1024), 0, s, (int)ntiles, w.counts, (unsigned long long)max_pairs, c);
  if (T) hipLaunchKernelGGL(md_scatter_kernel, dim3(nbt), dim3(MB), 0, s, (uint32_t)T, (const int4*)w.rect, gx, (const uint32_t*)w.counts, w.cursor, w.pairs,
                            (unsigned long long)max_pairs);
  hipLaunchKernelGGL(md_raster_kernel, dim3((unsigned)ntiles), dim3(MB), 0, s, v, gx, (const uint32_t*)w.counts, (const uint32_t*)w.pairs,
                     (unsigned long long)max_pairs, (const double*)w.rec, (uint32_t)T, depth, tri, c);
}

// ---- depth comparison --------------------------------------------------------------------------------------------------------------
#define DC_ROW 8
size_t depth_compare_work_bytes(int H, int W) { return md_nb((size_t)H * (size_t)W) * DC_ROW * sizeof(double); }

__device__ __forceinline__ bool dc_valid(float d) { return d > 0.f && d < INFINITY; }      // strict float32 tests: a NaN fails

__global__ void __launch_bounds__(MB)
dc_pixel_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[MB / 64][2];
  __shared__ double wmax[MB / 64];
  __shared__ uint32_t wcnt[4][MB / 64];
  const size_t i = (size_t)blockIdx.x * MB + threadIdx.x;
  bool both = false, only_b = false, only_a = false, neither = false;
  double d = 0.0;
  if (i < n) {
    const float x = a[i], y = b[i];
    const bool va = dc_valid(x), vb = dc_valid(y);
    both = va && vb; only_b = vb && !va; only_a = va && !vb; neither = !va && !vb;
    if (both) d = fabs((double)x - (double)y);
  }
  double mx = d;      // (not negative; a maximum has no order)
  for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(mx, off, 64); mx = o > mx ? o : mx; }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  double sums[2] = {d, d * d};
  block_sums_f64<2, false>(sums, wsum);      // (its barrier also publishes wmax)
  const bool is[4] = {both, only_b, only_a, neither};
  const uint32_t cnt = block_flag_counts(is, wcnt);
  double* row = partial + (size_t)blockIdx.x * DC_ROW;
  if (threadIdx.x < 4) row[3 + threadIdx.x] = (double)cnt;
  if (threadIdx.x == 0) {
    const double m01 = wmax[0] > wmax[1] ? wmax[0] : wmax[1], m23 = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
    row[0] = sums[0];
    row[1] = sums[1];
    row[2] = m01 > m23 ? m01 : m23;
    row[7] = 0.0;
  }
}

// one workgroup: lane t adds the partial rows t, t + 256, ... in index order, then the lanes are added in index order
__global__ void __launch_bounds__(MB) dc_finish_kernel(const double* __restrict__ partial, size_t nrows, double* __restrict__ row) {
  __shared__ double sh[MB][DC_ROW];
  double a[DC_ROW];
  for (int k = 0; k < DC_ROW; k++) a[k] = 0.0;
  for (size_t r = threadIdx.x; r < nrows; r += MB)
    for (int k = 0; k < DC_ROW; k++) {
      const double x = partial[r * DC_ROW + k];
      a[k] = k == 2 ? (x > a[k] ? x : a[k]) : a[k] + x;
    }
  for (int k = 0; k < DC_ROW; k++) sh[threadIdx.x][k] = a[k];
  __syncthreads();
  if (threadIdx.x < DC_ROW) {
    const int k = threadIdx.x;
    double t = 0.0;
    for (int l = 0; l < MB; l++) t = k == 2 ? (sh[l][k] > t ? sh[l][k] : t) : t + sh[l][k];
    sh[0][k] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = sh[0][0], sq = sh[0][1], mx = sh[0][2], n = sh[0][3];
    row[0] = n;
    row[1] = n > 0.0 ? sum / n : 0.0;
    row[2] = n > 0.0 ? sqrt(sq / n) : 0.0;
    row[3] = n > 0.0 ? mx : 0.0;
    row[4] = sh[0][4];
    row[5] = sh[0][5];
    row[6] = sh[0][6];
    row[7] = 0.0;
  }
}

void launch_depth_compare(int H, int W, const float* a, const float* b, void* work, double* row, hipStream_t s) {
  const size_t n = (size_t)H * (size_t)W, nb = md_nb(n);
  hipLaunchKernelGGL(dc_pixel_kernel, dim3((unsigned)nb), dim3(MB), 0, s, a, b, n, (double*)work);
  hipLaunchKernelGGL(dc_finish_kernel, dim3(1), dim3(MB), 0, s, (const double*)work, nb, row);
}

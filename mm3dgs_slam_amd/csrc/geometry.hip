// Geometry scores of an exported reconstruction against a reference surface (mm3dgs_nn_grid_build / mm3dgs_nn_query /
// mm3dgs_mesh_sample_plan / mm3dgs_mesh_sample_emit; host statement: geometry.nn_distances_host / geometry.sample_mesh_host).  Point sets
// are the cloud's 16-byte rows {float x, y, z; uint32 rgba}; the figures of one direction are one row of eight doubles on the device.
//
// Grid build (a uniform grid over the reference set, x fastest; cell = floor((double)x / cell) - origin_cell per axis):
//   ng_zero_kernel     the per-cell counts and the eight counters to zero.
//   ng_count_kernel    one lane per reference row: its cell (NN_NO_CELL for a row that is not finite or lies outside the box), one integer
//                      atomicAdd on the cell's count -- a count does not depend on the order of its adds.
//   ng_cellscan_kernel per 256 cells: the exclusive prefix inside the block and the block's total.
//   ng_scan_kernel     one workgroup of 1024: scan_block_counts over the block totals (block_ops.h), the total.
//   ng_base_kernel     cell_start = block prefix + local prefix; the same value into the cell's fill cursor.
//   ng_scatter_kernel  every row takes a slot of its cell (integer atomicAdd on the cursor) and stores one 16-byte record {x, y, z, row index}.
//                      The order inside a cell depends on the atomics; a minimum over the cell does not.
// Query (ng_query_kernel, one lane per query): the cells at Chebyshev ring r around the query's own cell, clipped to the grid, r = 0, 1, 2, ...;
//   a row of cells along x is one contiguous range of records, so rings 0 and 1 together are at most nine ranges; the lane stops after ring r
//   when best <= r cell (every unsearched record is farther), after ring ceil(max_dist / cell), or when no further ring touches the grid; a
//   query outside the grid starts at the first ring that touches it.  Distances in double from the float32 coordinates, no contraction,
//   rounded once at the store.  Per workgroup one row of partial sums in double, fixed lane order; ng_finish_kernel (one workgroup) adds the
//   partial rows in a fixed order and writes the eight figures.  No float atomic: the same inputs give the same bytes on every call.
// Sampler (area-uniform samples of a triangle mesh by stochastic rounding of area x density, a 32-bit integer mixer as the random source):
//   ms_plan_kernel     one lane per triangle: n_t, the exclusive prefix inside the 256-block, the block's total and its degenerate count.
//   ms_scan_kernel     one workgroup of 1024: scan_block_counts, the 64-bit total, the degenerate count, the counter block.
//   ms_base_kernel     prefix[t] += block prefix.
//   ms_emit_kernel     one lane per SAMPLE: binary search of its triangle in the exclusive prefix, then the sample's row.
// Normals (mm3dgs_nn_query_index / mm3dgs_mesh_sample_emit_tri / mm3dgs_normal_consistency / mm3dgs_mesh_vertex_normals; host statement:
//   geometry.nn_index_host / normal_row / vertex_normals_host): ng_query_kernel<true> also keeps the original row of the nearest record,
//   ms_emit_kernel<true> the triangle of every sample (the <false> instantiations are the calls above, byte for byte); ms_cross / ms_face
//   state the face cross product once; nc_dot_kernel and the four vn_* kernels are described where they stand.
// Registration (mm3dgs_icp_point / mm3dgs_rows_move; host statement: geometry.icp_host / move_rows_host): ng_search is the one per-query search
//   behind ng_query_kernel and icp_pass_kernel; the icp_* kernels and rows_move_kernel are described where they stand.
#include <math.h>
#include "block_ops.h"
#include "fused_api.h"
#include "view_pixel.h"      // view_finite

#define GB 256
#define NN_NO_CELL 0xffffffffu
#define NN_ROW 8      // doubles per partial row: sum d, sum d^2, max d, n, within, clamped, skipped, 0

static size_t ng_nb(size_t n) { return (n + GB - 1) / GB; }

// ---- grid build -------------------------------------------------------------------------------------------------------------------
// work = [uint32 cell per reference row][uint32 count, then fill cursor, per cell][uint32 per 256 cells]
struct NgWork { uint32_t* cellidx; uint32_t* cursor; uint32_t* bcounts; };
static NgWork ng_work(void* base, size_t n_ref, size_t nc, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  NgWork w;
  w.cellidx = c.take<uint32_t>(n_ref);
  w.cursor = c.take<uint32_t>(nc);
  w.bcounts = c.take<uint32_t>(ng_nb(nc));
  if (bytes) *bytes = c.at;
  return w;
}
size_t nn_grid_work_bytes(uint64_t n_ref, int gx, int gy, int gz) { size_t b; ng_work(nullptr, (size_t)n_ref, (size_t)gx * (size_t)gy * (size_t)gz, &b); return b; }

// the cell coordinates of a finite position, relative to the grid's origin cell, as doubles (they may lie outside the grid, or beyond an int)
__device__ __forceinline__ void ng_cell(const NnGrid& g, float x, float y, float z, double (&c)[3]) {
#pragma clang fp contract(off)
  c[0] = floor((double)x / g.cell) - g.o[0];
  c[1] = floor((double)y / g.cell) - g.o[1];
  c[2] = floor((double)z / g.cell) - g.o[2];
}

__global__ void __launch_bounds__(GB) ng_zero_kernel(uint32_t* __restrict__ counts, size_t nc, unsigned long long* __restrict__ counters) {
  const size_t step = (size_t)gridDim.x * GB;
  for (size_t i = (size_t)blockIdx.x * GB + threadIdx.x; i < nc; i += step) counts[i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x < 8) counters[threadIdx.x] = 0ull;
}

__global__ void __launch_bounds__(GB)
ng_count_kernel(NnGrid g, const uint4* __restrict__ rows, uint32_t n, uint32_t* __restrict__ cellidx, uint32_t* __restrict__ counts,
                unsigned long long* __restrict__ counters) {
  const uint32_t i = blockIdx.x * GB + threadIdx.x;
  bool bad = false, out = false;
  if (i < n) {
    const uint4 r = rows[i];
    const float x = __uint_as_float(r.x), y = __uint_as_float(r.y), z = __uint_as_float(r.z);
    uint32_t cell = NN_NO_CELL;
    if (!view_finite(x, y, z)) {
      bad = true;
    } else {
      double c[3];
      ng_cell(g, x, y, z, c);
      if (c[0] >= 0.0 && c[0] < (double)g.gx && c[1] >= 0.0 && c[1] < (double)g.gy && c[2] >= 0.0 && c[2] < (double)g.gz)
        cell = ((uint32_t)(int)c[2] * (uint32_t)g.gy + (uint32_t)(int)c[1]) * (uint32_t)g.gx + (uint32_t)(int)c[0];
      else
        out = true;
    }
    cellidx[i] = cell;
    if (cell != NN_NO_CELL) atomicAdd(&counts[cell], 1u);
  }
  const unsigned long long mb = __ballot(bad), mo = __ballot(out);
  if ((threadIdx.x & 63) == 0) {      // integer adds: the sums do not depend on their order
    if (mb) atomicAdd(counters + 1, (unsigned long long)__popcll(mb));
    if (mo) atomicAdd(counters + 2, (unsigned long long)__popcll(mo));
  }
}

__global__ void __launch_bounds__(GB)
ng_cellscan_kernel(const uint32_t* __restrict__ counts, size_t nc, uint32_t* __restrict__ cell_start, uint32_t* __restrict__ bcounts) {
  __shared__ uint32_t wtot[GB / 64];
  const size_t i = (size_t)blockIdx.x * GB + threadIdx.x;
  const uint32_t v = i < nc ? counts[i] : 0u;
  const uint32_t incl = block_scan_incl(v, wtot);
  if (i < nc) cell_start[i] = incl - v;
  if (threadIdx.x == GB - 1) bcounts[blockIdx.x] = incl;
}

__global__ void __launch_bounds__(1024)
ng_scan_kernel(int nb, uint32_t* __restrict__ bcounts, uint32_t* __restrict__ cell_end, unsigned long long* __restrict__ counters, unsigned long long nc) {
  __shared__ uint32_t total;
  scan_block_counts(nb, bcounts, &total);
  if (threadIdx.x == 0) {      // (lane 0 wrote `total` itself)
    *cell_end = total;
    counters[0] = total;
    counters[3] = nc;
  }
}

__global__ void __launch_bounds__(GB)
ng_base_kernel(size_t nc, const uint32_t* __restrict__ bpre, uint32_t* __restrict__ cell_start, uint32_t* __restrict__ cursor) {
  const size_t i = (size_t)blockIdx.x * GB + threadIdx.x;
  if (i >= nc) return;
  const uint32_t s = cell_start[i] + bpre[blockIdx.x];
  cell_start[i] = s;
  cursor[i] = s;
}

__global__ void __launch_bounds__(GB)
ng_scatter_kernel(const uint4* __restrict__ rows, uint32_t n, const uint32_t* __restrict__ cellidx, uint32_t* __restrict__ cursor, uint4* __restrict__ sorted) {
  const uint32_t i = blockIdx.x * GB + threadIdx.x;
  if (i >= n) return;
  const uint32_t cell = cellidx[i];
  if (cell == NN_NO_CELL) return;
  const uint32_t slot = atomicAdd(&cursor[cell], 1u);
  if (slot >= n) return;      // (cannot happen: the cursors start at the prefix of the same counts)
  const uint4 r = rows[i];
  sorted[slot] = make_uint4(r.x, r.y, r.z, i);      // one 16-byte store
}

void launch_nn_grid_build(const NnGrid& g, uint64_t n_ref, const void* rows, void* cell_start, void* sorted, uint64_t* counters, void* work, hipStream_t s) {
  const size_t nc = (size_t)g.gx * (size_t)g.gy * (size_t)g.gz;
  const NgWork w = ng_work(work, (size_t)n_ref, nc);
  const unsigned nbc = (unsigned)ng_nb(nc), nbr = (unsigned)ng_nb((size_t)n_ref);
  uint32_t* cs = (uint32_t*)cell_start;
  hipLaunchKernelGGL(ng_zero_kernel, dim3(nbc < 4096u ? nbc : 4096u), dim3(GB), 0, s, w.cursor, nc, (unsigned long long*)counters);
  hipLaunchKernelGGL(ng_count_kernel, dim3(nbr), dim3(GB), 0, s, g, (const uint4*)rows, (uint32_t)n_ref, w.cellidx, w.cursor, (unsigned long long*)counters);
  hipLaunchKernelGGL(ng_cellscan_kernel, dim3(nbc), dim3(GB), 0, s, w.cursor, nc, cs, w.bcounts);
  hipLaunchKernelGGL(ng_scan_kernel, dim3(1), dim3(1024), 0, s, (int)nbc, w.bcounts, cs + nc, (unsigned long long*)counters, (unsigned long long)nc);
  hipLaunchKernelGGL(ng_base_kernel, dim3(nbc), dim3(GB), 0, s, nc, w.bcounts, cs, w.cursor);
  hipLaunchKernelGGL(ng_scatter_kernel, dim3(nbr), dim3(GB), 0, s, (const uint4*)rows, (uint32_t)n_ref, w.cellidx, w.cursor, (uint4*)sorted);
}

// ---- query ------------------------------------------------------------------------------------------------------------------------
size_t nn_query_work_bytes(uint64_t n_q) { return align_up(ng_nb((size_t)n_q) * NN_ROW * sizeof(double), 256); }

struct NnQuery { double qx, qy, qz, best2; uint32_t besti, bestp; };      // besti: the original row of the best record, bestp: where it lies in `sorted` (INDEX only)

// the records [b, e) against the query: squared distance in double (each coordinate widened, then subtracted; three squares, a sum);
// INDEX: the minimum is lexicographic over (d2, original row), so neither the order inside a cell nor duplicates decide the row
template <bool INDEX>
__device__ __forceinline__ void ng_scan_records(const uint4* __restrict__ sorted, uint32_t b, uint32_t e, uint32_t n_ref, NnQuery& q) {
#pragma clang fp contract(off)
  e = e < n_ref ? e : n_ref;
  for (uint32_t p = b; p < e; p++) {
    const uint4 v = sorted[p];      // one 16-byte load per candidate
    const double dx = q.qx - (double)__uint_as_float(v.x), dy = q.qy - (double)__uint_as_float(v.y), dz = q.qz - (double)__uint_as_float(v.z);
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (INDEX && (d2 < q.best2 || (d2 == q.best2 && v.w < q.besti))) { q.besti = v.w; q.bestp = p; }
    q.best2 = d2 < q.best2 ? d2 : q.best2;
  }
}

__device__ __forceinline__ int ng_lo(int c, int r) { return c - r > 0 ? c - r : 0; }
__device__ __forceinline__ int ng_hi(int c, int r, int g) { return c + r < g - 1 ? c + r : g - 1; }

// every cell within Chebyshev distance r of (cx, cy, cz), clipped to the grid: one range of records per row of cells
template <bool INDEX>
__device__ __forceinline__ void ng_cube(const NnGrid& g, const uint32_t* __restrict__ cell_start, const uint4* __restrict__ sorted, uint32_t n_ref, int cx,
                                        int cy, int cz, int r, NnQuery& q) {
  const int x0 = ng_lo(cx, r), x1 = ng_hi(cx, r, g.gx);
  if (x0 > x1) return;
  for (int z = ng_lo(cz, r); z <= ng_hi(cz, r, g.gz); z++)
    for (int y = ng_lo(cy, r); y <= ng_hi(cy, r, g.gy); y++) {
      const size_t row = ((size_t)z * (size_t)g.gy + (size_t)y) * (size_t)g.gx;
      ng_scan_records<INDEX>(sorted, cell_start[row + x0], cell_start[row + x1 + 1], n_ref, q);
    }
}

// the cells at Chebyshev distance exactly r >= 1, clipped to the grid: whole rows on the four faces across y and z, two cells per row elsewhere
template <bool INDEX>
__device__ __forceinline__ void ng_ring(const NnGrid& g, const uint32_t* __restrict__ cell_start, const uint4* __restrict__ sorted, uint32_t n_ref, int cx,
                                        int cy, int cz, int r, NnQuery& q) {
  const int x0 = ng_lo(cx, r), x1 = ng_hi(cx, r, g.gx);
  for (int z = ng_lo(cz, r); z <= ng_hi(cz, r, g.gz); z++) {
    const bool fz = z - cz == r || cz - z == r;
    for (int y = ng_lo(cy, r); y <= ng_hi(cy, r, g.gy); y++) {
      const size_t row = ((size_t)z * (size_t)g.gy + (size_t)y) * (size_t)g.gx;
      if (fz || y - cy == r || cy - y == r) {
        if (x0 <= x1) ng_scan_records<INDEX>(sorted, cell_start[row + x0], cell_start[row + x1 + 1], n_ref, q);
      } else {
        const int xa = cx - r, xb = cx + r;
        if (xa >= 0 && xa < g.gx) ng_scan_records<INDEX>(sorted, cell_start[row + xa], cell_start[row + xa + 1], n_ref, q);
        if (xb >= 0 && xb < g.gx) ng_scan_records<INDEX>(sorted, cell_start[row + xb], cell_start[row + xb + 1], n_ref, q);
      }
    }
  }
}

// the search of one finite query (x, y, z): from its cell to the final q.best2 / q.besti (q.best2 +inf: nothing within rmax rings).  The one
// statement behind ng_query_kernel and icp_pass_kernel
template <bool INDEX>
__device__ __forceinline__ void ng_search(const NnGrid& g, const uint32_t* __restrict__ cell_start, const uint4* __restrict__ sorted, uint32_t n_ref, int rmax,
                                          float x, float y, float z, NnQuery& q) {
#pragma clang fp contract(off)
  q.qx = (double)x; q.qy = (double)y; q.qz = (double)z; q.best2 = (double)INFINITY; q.besti = NN_NO_CELL; q.bestp = 0u;
  double c[3];
  ng_cell(g, x, y, z, c);
  // the first ring that touches the grid, and the last one that does (as doubles: a far query's cell may not fit an int)
  const double gs[3] = {(double)g.gx, (double)g.gy, (double)g.gz};
  double r0 = 0.0, rfar = 0.0;
  for (int a = 0; a < 3; a++) {
    const double below = -c[a], above = c[a] - (gs[a] - 1.0);
    const double o = below > above ? below : above;      // > 0: cells outside the grid along this axis
    r0 = o > r0 ? o : r0;
    const double f = c[a] > (gs[a] - 1.0) - c[a] ? c[a] : (gs[a] - 1.0) - c[a];
    rfar = f > rfar ? f : rfar;
  }
  if (r0 <= (double)rmax) {      // (else: nothing within max_dist)
    const int cx = (int)c[0], cy = (int)c[1], cz = (int)c[2];      // |c| <= grid size + rmax here
    const int last = rfar < (double)rmax ? (int)rfar : rmax;
    int rr = r0 <= 1.0 ? 1 : (int)r0;
    if (rr == 1) ng_cube<INDEX>(g, cell_start, sorted, n_ref, cx, cy, cz, 1, q);      // rings 0 and 1: nine ranges
    else ng_ring<INDEX>(g, cell_start, sorted, n_ref, cx, cy, cz, rr, q);
    while (rr < last && !(sqrt(q.best2) <= (double)rr * g.cell)) {      // at most rmax trips
      rr++;
      ng_ring<INDEX>(g, cell_start, sorted, n_ref, cx, cy, cz, rr, q);
    }
  }
}

template <bool INDEX>
__global__ void __launch_bounds__(GB)
ng_query_kernel(NnGrid g, const uint4* __restrict__ qrows, uint32_t n_q, const uint32_t* __restrict__ cell_start, const uint4* __restrict__ sorted,
                uint32_t n_ref, double max_dist, float threshold, int rmax, float* __restrict__ dist_out, uint32_t* __restrict__ index_out, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[GB / 64][2];
  __shared__ uint32_t wcnt[4][GB / 64];
  __shared__ uint32_t smax;
  const uint32_t i = blockIdx.x * GB + threadIdx.x;
  if (threadIdx.x == 0) smax = 0u;
  __syncthreads();
  bool scored = false, skipped = false, clamped = false, within = false;
  double dd = 0.0;
  if (i < n_q) {
    const uint4 r = qrows[i];
    const float x = __uint_as_float(r.x), y = __uint_as_float(r.y), z = __uint_as_float(r.z);
    float out;
    uint32_t nearest = NN_NO_CELL;      // (INDEX) 0xffffffff: none
    if (!view_finite(x, y, z)) {
      skipped = true;
      out = __uint_as_float(0x7fc00000u);
    } else {
      NnQuery q;
      ng_search<INDEX>(g, cell_start, sorted, n_ref, rmax, x, y, z, q);
      const double d = sqrt(q.best2);
      clamped = !(d <= max_dist);
      if (INDEX && !clamped) nearest = q.besti;
      out = clamped ? (float)max_dist : (float)d;      // the one rounding
      within = out <= threshold;
      scored = true;
      dd = (double)out;
      atomicMax(&smax, __float_as_uint(out));      // LDS, integer: a non-negative float orders as its bits
    }
    dist_out[i] = out;
    if (INDEX) index_out[i] = nearest;
  }
  double sums[2] = {dd, dd * dd};
  block_sums_f64<2, false>(sums, wsum);
  const bool is[4] = {scored, within, clamped, skipped};
  const uint32_t cnt = block_flag_counts(is, wcnt);
  double* row = partial + (size_t)blockIdx.x * NN_ROW;
  if (threadIdx.x < 4) row[3 + threadIdx.x] = (double)cnt;
  if (threadIdx.x == 0) {
    row[0] = sums[0];
    row[1] = sums[1];
    row[2] = (double)__uint_as_float(smax);
    row[7] = 0.0;
  }
}

// the eight figures of one direction from the finished sums: distances, and normal consistency
__device__ __forceinline__ void ng_figures(const double* t, double* row) {
  const double sum = t[0], sq = t[1], mx = t[2], n = t[3], within = t[4], clamped = t[5], skipped = t[6];
  row[0] = n;
  row[1] = n > 0.0 ? sum / n : 0.0;
  row[2] = n > 0.0 ? sqrt(sq / n) : 0.0;
  row[3] = mx;
  row[4] = n > 0.0 ? within / n : 0.0;
  row[5] = clamped;
  row[6] = skipped;
  row[7] = 0.0;
}
__device__ __forceinline__ void nc_figures(const double* t, double* row) {
  const double sabs = t[0], sum = t[1], mn = t[2], n = t[3], none = t[5], bad = t[6];
  row[0] = n;
  row[1] = n > 0.0 ? sabs / n : 0.0;
  row[2] = n > 0.0 ? sum / n : 0.0;
  row[3] = n > 0.0 ? mn : 0.0;
  row[4] = 0.0;
  row[5] = none;
  row[6] = bad;
  row[7] = 0.0;
}

// one workgroup: lane t adds the partial rows t, t + 256, ... in index order, then the lanes are added in index order (geometry.kernel_order_sum
// states this order).  Column 2 is a maximum from 0 and the figures ng_figures' (NORMALS false: the distances), or a minimum from +inf and
// the figures nc_figures' (NORMALS true: nc_dot_kernel's rows)
template <bool NORMALS>
__global__ void __launch_bounds__(GB) ng_finish_kernel(const double* __restrict__ partial, int nrows, double* __restrict__ row) {
  __shared__ double sh[GB][NN_ROW];
  const double start = NORMALS ? (double)INFINITY : 0.0;
  double a[NN_ROW];
  for (int k = 0; k < NN_ROW; k++) a[k] = k == 2 ? start : 0.0;
  for (int r = threadIdx.x; r < nrows; r += GB)
    for (int k = 0; k < NN_ROW; k++) {
      const double v = partial[(size_t)r * NN_ROW + k];
      a[k] = k == 2 ? ((NORMALS ? v < a[k] : v > a[k]) ? v : a[k]) : a[k] + v;
    }
  for (int k = 0; k < NN_ROW; k++) sh[threadIdx.x][k] = a[k];
  __syncthreads();
  if (threadIdx.x < NN_ROW) {
    const int k = threadIdx.x;
    double t = k == 2 ? start : 0.0;
    for (int l = 0; l < GB; l++) t = k == 2 ? ((NORMALS ? sh[l][k] < t : sh[l][k] > t) ? sh[l][k] : t) : t + sh[l][k];
    sh[0][k] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (NORMALS) nc_figures(sh[0], row);
    else ng_figures(sh[0], row);
  }
}

// index_out_or_null selects ng_query_kernel<true>: the kernel is the same, byte for byte of dist_out and row
void launch_nn_query(const NnGrid& g, uint64_t n_q, const void* qrows, uint64_t n_ref, const void* cell_start, const void* sorted, double max_dist,
                     double threshold, int rmax, float* dist_out, uint32_t* index_out_or_null, double* row, void* work, hipStream_t s) {
  const unsigned nb = (unsigned)ng_nb((size_t)n_q);
  hipLaunchKernelGGL(index_out_or_null ? ng_query_kernel<true> : ng_query_kernel<false>, dim3(nb), dim3(GB), 0, s, g, (const uint4*)qrows, (uint32_t)n_q,
                     (const uint32_t*)cell_start, (const uint4*)sorted, (uint32_t)n_ref, max_dist, (float)threshold, rmax, dist_out, index_out_or_null, (double*)work);
  hipLaunchKernelGGL(ng_finish_kernel<false>, dim3(1), dim3(GB), 0, s, (const double*)work, (int)nb, row);
}

// ---- point-to-point ICP -----------------------------------------------------------------------------------------------------------
// mm3dgs_icp_point / mm3dgs_rows_move; host statement: geometry.icp_host / move_rows_host / _horn_solve.  Pass k = 0 .. iters is two
// launches, and no launch waits for the host: the stop is a word on the device that every later launch reads at entry.
//   icp_zero_kernel   the log, the header and state[12:16] to zero.
//   icp_pass_kernel   one lane per source row: the row moved by T (state[0:12]) and rounded once, ng_search<true> for the moved row, the 17
//                     terms {1, p, q, p_a q_b, d2} of a row with a correspondence (p: the ORIGINAL coordinates, so a solve gives the absolute
//                     transform); per workgroup one partial row of ICP_ROW doubles in block_sums_f64's order.  No float atomic.
//   icp_step_kernel   one workgroup adds the partial rows in ng_finish_kernel's order; lane 0: the figures of T, the stop rule, else Horn's
//                     closed form on the sums (icp_horn: the dominant eigenvector of N(S) by cyclic Jacobi rotations, + - x / sqrt only).
//   rows_move_kernel  one lane per row: the position moved by T from device memory, rounded once; rgba and a row that is not finite as they are.
// work = [ICP_HDR doubles: [0] done, [1] fitness and [2] rmse of the pass before, [3:7] the quaternion of the latest solve][one partial row
// per workgroup: the 17 sums, finite rows, rows with a correspondence, 0 x 5]
#define ICP_SUMS 17
#define ICP_COLS 19     // the columns of a partial row that are added
#define ICP_ROW 24      // doubles per partial row
#define ICP_HDR 32
#define ICP_LOG 16      // doubles per log row
#define ICP_SWEEPS 50   // icp_horn's cap (see there)

size_t icp_work_bytes(uint64_t n_q) { return ICP_HDR * sizeof(double) + align_up(ng_nb((size_t)n_q) * ICP_ROW * sizeof(double), 256); }

__global__ void __launch_bounds__(GB) icp_zero_kernel(double* __restrict__ state, double* __restrict__ log, size_t nlog, double* __restrict__ hdr) {
  const size_t step = (size_t)gridDim.x * GB;
  for (size_t i = (size_t)blockIdx.x * GB + threadIdx.x; i < nlog; i += step) log[i] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x < ICP_HDR) hdr[threadIdx.x] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x < 4) state[12 + threadIdx.x] = 0.0;
}

// one component of a moved position: ((R0 x + R1 y) + R2 z) + t in double, rounded once (T row-major [3][4], no contraction)
__device__ __forceinline__ float icp_move_axis(const double (&T)[12], int a, double x, double y, double z) {
#pragma clang fp contract(off)
  return (float)(((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3]);
}

// OUT: dist_out / index_out (either may be NULL) also get what mm3dgs_nn_query_index stores for the moved rows
template <bool OUT>
__global__ void __launch_bounds__(GB)
icp_pass_kernel(NnGrid g, const uint4* __restrict__ qrows, uint32_t n_q, const uint32_t* __restrict__ cell_start, const uint4* __restrict__ sorted,
                uint32_t n_ref, double max_dist, int rmax, const double* __restrict__ state, const double* __restrict__ hdr, float* __restrict__ dist_out,
                uint32_t* __restrict__ index_out, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[GB / 64][ICP_SUMS];
  __shared__ uint32_t wcnt[2][GB / 64];
  if (hdr[0] != 0.0) return;      // the loop has stopped (uniform: before any barrier)
  double T[12];
  for (int k = 0; k < 12; k++) T[k] = state[k];      // uniform loads
  const uint32_t i = blockIdx.x * GB + threadIdx.x;
  bool finite = false, paired = false;
  double v[ICP_SUMS];
  for (int k = 0; k < ICP_SUMS; k++) v[k] = 0.0;
  if (i < n_q) {
    const uint4 r = qrows[i];
    const float x = __uint_as_float(r.x), y = __uint_as_float(r.y), z = __uint_as_float(r.z);
    float out = __uint_as_float(0x7fc00000u);
    uint32_t nearest = NN_NO_CELL;
    if (view_finite(x, y, z)) {
      finite = true;
      const double p[3] = {(double)x, (double)y, (double)z};
      const float mx = icp_move_axis(T, 0, p[0], p[1], p[2]), my = icp_move_axis(T, 1, p[0], p[1], p[2]), mz = icp_move_axis(T, 2, p[0], p[1], p[2]);
      if (view_finite(mx, my, mz)) {      // (a moved row beyond float32 is a row that is not finite: skipped)
        NnQuery q;
        ng_search<true>(g, cell_start, sorted, n_ref, rmax, mx, my, mz, q);
        const double d = sqrt(q.best2);
        const bool clamped = !(d <= max_dist);
        out = clamped ? (float)max_dist : (float)d;
        if (!clamped && q.bestp < n_ref) {      // (bestp < n_ref always holds here: the record was read)
          paired = true;
          nearest = q.besti;
          const uint4 b = sorted[q.bestp];
          const double t[3] = {(double)__uint_as_float(b.x), (double)__uint_as_float(b.y), (double)__uint_as_float(b.z)};
          v[0] = 1.0;
          for (int a = 0; a < 3; a++) {
            v[1 + a] = p[a];
            v[4 + a] = t[a];
            for (int c = 0; c < 3; c++) v[7 + 3 * a + c] = p[a] * t[c];
          }
          v[16] = q.best2;
        }
      }
    }
    if (OUT && dist_out) dist_out[i] = out;
    if (OUT && index_out) index_out[i] = nearest;
  }
  block_sums_f64<ICP_SUMS, false>(v, wsum);
  const bool is[2] = {finite, paired};
  const uint32_t cnt = block_flag_counts(is, wcnt);
  double* row = partial + (size_t)blockIdx.x * ICP_ROW;
  if (threadIdx.x < 2) row[ICP_SUMS + threadIdx.x] = (double)cnt;
  if (threadIdx.x == 0) {
    for (int k = 0; k < ICP_SUMS; k++) row[k] = v[k];
    for (int k = ICP_COLS; k < ICP_ROW; k++) row[k] = 0.0;
  }
}

// Horn's closed form on the 17 sums s = {n, sum p, sum q, sum p_a q_b, -}: T (row-major [3][4]) with q ~ R p + t, and the unit quaternion
// (w >= 0) of R.  S = sum p q^T - sum p sum q^T / n, N(S) the symmetric 4 x 4 matrix of Horn 1987, its dominant eigenvector by cyclic Jacobi
// rotations in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  + - x / sqrt and comparisons only, no contraction: geometry._horn_solve is
// the same sequence of operations on the host, so the two agree bit for bit.  A sweep starts only while an off-diagonal element is not
// exactly zero; an element below the rounding of both its diagonal neighbours is set to zero from the fifth sweep on, so the sum reaches
// zero: quadratic convergence takes a 4 x 4 matrix there in well under ten sweeps (tests/test_icp.py counts them on random and on
// degenerate matrices), and ICP_SWEEPS = 50 is the classical cap that only bounds the loop
__device__ void icp_horn(const double* s, double (&T)[12], double (&quat)[4]) {
#pragma clang fp contract(off)
  const double n = s[0];
  double S[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) S[a][b] = s[7 + 3 * a + b] - (s[1 + a] * s[4 + b]) / n;
  double A[4][4], V[4][4];
  A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
  A[0][1] = S[1][2] - S[2][1];
  A[0][2] = S[2][0] - S[0][2];
  A[0][3] = S[0][1] - S[1][0];
  A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
  A[1][2] = S[0][1] + S[1][0];
  A[1][3] = S[2][0] + S[0][2];
  A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
  A[2][3] = S[1][2] + S[2][1];
  A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++) {
      if (b < a) A[a][b] = A[b][a];
      V[a][b] = a == b ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < ICP_SWEEPS; sweep++) {
    const double off = ((((fabs(A[0][1]) + fabs(A[0][2])) + fabs(A[0][3])) + fabs(A[1][2])) + fabs(A[1][3])) + fabs(A[2][3]);
    if (off == 0.0) break;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double gg = 100.0 * fabs(apq);
        if (sweep > 3 && fabs(A[p][p]) + gg == fabs(A[p][p]) && fabs(A[q][q]) + gg == fabs(A[q][q])) {
          A[p][q] = 0.0; A[q][p] = 0.0;
          continue;
        }
        const double h = A[q][q] - A[p][p];
        double t;
        if (fabs(h) + gg == fabs(h)) {
          t = apq / h;
        } else {
          const double theta = (0.5 * h) / apq;
          t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
          if (theta < 0.0) t = -t;
        }
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        A[p][p] = A[p][p] - t * apq;
        A[q][q] = A[q][q] + t * apq;
        A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if (r != p && r != q) {
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = c * arp - sn * arq; A[p][r] = A[r][p];
            A[r][q] = sn * arp + c * arq; A[q][r] = A[r][q];
          }
          const double vrp = V[r][p], vrq = V[r][q];
          V[r][p] = c * vrp - sn * vrq;
          V[r][q] = sn * vrp + c * vrq;
        }
      }
  }
  double top = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];      // the largest eigenvalue, the first one on a tie
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (A[k][k] > top) { top = A[k][k]; w = V[0][k]; x = V[1][k]; y = V[2][k]; z = V[3][k]; }
  if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
  const double len = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / len; x = x / len; y = y / len; z = z / len;
  quat[0] = w; quat[1] = x; quat[2] = y; quat[3] = z;
  const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  double R[3][3];
  R[0][0] = ((ww + xx) - yy) - zz; R[0][1] = 2.0 * (xy - wz);       R[0][2] = 2.0 * (xz + wy);
  R[1][0] = 2.0 * (xy + wz);       R[1][1] = ((ww - xx) + yy) - zz; R[1][2] = 2.0 * (yz - wx);
  R[2][0] = 2.0 * (xz - wy);       R[2][1] = 2.0 * (yz + wx);       R[2][2] = ((ww - xx) - yy) + zz;
  const double mp[3] = {s[1] / n, s[2] / n, s[3] / n};
  for (int a = 0; a < 3; a++) {
    T[4 * a] = R[a][0]; T[4 * a + 1] = R[a][1]; T[4 * a + 2] = R[a][2];
    T[4 * a + 3] = s[4 + a] / n - ((R[a][0] * mp[0] + R[a][1] * mp[1]) + R[a][2] * mp[2]);
  }
}

__global__ void __launch_bounds__(GB)
icp_step_kernel(const double* __restrict__ partial, int nrows, int k, int iters, double rel_fitness, double rel_rmse, double* __restrict__ state,
                double* __restrict__ hdr, double* __restrict__ log) {
#pragma clang fp contract(off)
  __shared__ double sh[GB][ICP_COLS];
  if (hdr[0] != 0.0) return;      // (uniform: before any barrier; lane 0 writes the word behind two of them)
  double a[ICP_COLS];
#pragma unroll
  for (int c = 0; c < ICP_COLS; c++) a[c] = 0.0;
  for (int r = threadIdx.x; r < nrows; r += GB)
#pragma unroll
    for (int c = 0; c < ICP_COLS; c++) a[c] = a[c] + partial[(size_t)r * ICP_ROW + c];
#pragma unroll
  for (int c = 0; c < ICP_COLS; c++) sh[threadIdx.x][c] = a[c];
  __syncthreads();
  if (threadIdx.x < ICP_COLS) {
    const int c = threadIdx.x;
    double t = 0.0;
    for (int l = 0; l < GB; l++) t = t + sh[l][c];
    sh[0][c] = t;      // (column c of row 0: no other lane reads or writes it)
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double* s = sh[0];
  const double n = s[0], fin = s[ICP_SUMS];
  const double fitness = n > 0.0 ? n / fin : 0.0, rmse = n > 0.0 ? sqrt(s[16] / n) : 0.0;      // of the T this pass started with
  int status = -1;      // -1: go on
  if (k > 0 && fabs(fitness - hdr[1]) < rel_fitness && fabs(rmse - hdr[2]) < rel_rmse) status = 0;
  else if (n < 3.0) status = 2;
  else if (k == iters) status = 1;
  if (status < 0) {
    double T[12], quat[4];
    icp_horn(s, T, quat);
    for (int c = 0; c < 12; c++) state[c] = T[c];
    for (int c = 0; c < 4; c++) hdr[3 + c] = quat[c];
  }
  hdr[1] = fitness;
  hdr[2] = rmse;
  double* row = log + (size_t)k * ICP_LOG;
  row[0] = 1.0; row[1] = n; row[2] = fin; row[3] = fitness; row[4] = rmse;
  for (int c = 0; c < 4; c++) row[5 + c] = hdr[3 + c];
  for (int c = 0; c < 3; c++) row[9 + c] = state[4 * c + 3];
  row[12] = status > 0 ? (double)status : 0.0;
  row[13] = 0.0; row[14] = 0.0; row[15] = 0.0;
  if (status >= 0) {
    state[12] = (double)(k + 1);
    state[13] = (double)status;
    hdr[0] = 1.0;
  }
}

void launch_icp_point(const NnGrid& g, uint64_t n_q, const void* qrows, uint64_t n_ref, const void* cell_start, const void* sorted, double max_dist, int rmax,
                      int iters, double rel_fitness, double rel_rmse, double* state, double* log, float* dist_out, uint32_t* index_out, void* work, hipStream_t s) {
  const unsigned nb = (unsigned)ng_nb((size_t)n_q);
  double* hdr = (double*)work;
  double* partial = hdr + ICP_HDR;
  const size_t nlog = (size_t)(iters + 1) * ICP_LOG;
  hipLaunchKernelGGL(icp_zero_kernel, dim3((unsigned)ng_nb(nlog)), dim3(GB), 0, s, state, log, nlog, hdr);
  for (int k = 0; k <= iters; k++) {
    hipLaunchKernelGGL((dist_out || index_out) ? icp_pass_kernel<true> : icp_pass_kernel<false>, dim3(nb), dim3(GB), 0, s, g, (const uint4*)qrows, (uint32_t)n_q,
                       (const uint32_t*)cell_start, (const uint4*)sorted, (uint32_t)n_ref, max_dist, rmax, (const double*)state, (const double*)hdr, dist_out,
                       index_out, partial);
    hipLaunchKernelGGL(icp_step_kernel, dim3(1), dim3(GB), 0, s, (const double*)partial, (int)nb, k, iters, rel_fitness, rel_rmse, state, hdr, log);
  }
}

// (rows_in and rows_out may be the same array: a lane reads its row before it writes it)
__global__ void __launch_bounds__(GB) rows_move_kernel(uint32_t n, const uint4* rows_in, const double* __restrict__ Tdev, uint4* rows_out) {
  double T[12];
  for (int k = 0; k < 12; k++) T[k] = Tdev[k];      // uniform loads
  const uint32_t i = blockIdx.x * GB + threadIdx.x;
  if (i >= n) return;
  uint4 r = rows_in[i];
  const float x = __uint_as_float(r.x), y = __uint_as_float(r.y), z = __uint_as_float(r.z);
  if (view_finite(x, y, z)) {
    r.x = __float_as_uint(icp_move_axis(T, 0, (double)x, (double)y, (double)z));
    r.y = __float_as_uint(icp_move_axis(T, 1, (double)x, (double)y, (double)z));
    r.z = __float_as_uint(icp_move_axis(T, 2, (double)x, (double)y, (double)z));
  }
  rows_out[i] = r;      // one 16-byte store
}

void launch_rows_move(uint64_t n, const void* rows_in, const double* T, void* rows_out, hipStream_t s) {
  hipLaunchKernelGGL(rows_move_kernel, dim3((unsigned)ng_nb((size_t)n)), dim3(GB), 0, s, (uint32_t)n, (const uint4*)rows_in, T, (uint4*)rows_out);
}

// ---- surface sampler --------------------------------------------------------------------------------------------------------------
// work =[256 B header: uint64 samples (0 when they exceed 32 bits)][uint32 exclusive prefix per triangle][2 x uint32 per 256 triangles: samples, degenerate]
struct MsWork { unsigned long long* hdr; uint32_t* prefix; uint32_t* bcounts; uint32_t* dcounts; };
static MsWork ms_work(void* base, size_t m, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  MsWork w;
  w.hdr = c.take<unsigned long long>(1);
  w.prefix = c.take<uint32_t>(m);
  w.bcounts = c.take<uint32_t>(ng_nb(m));
  w.dcounts = c.take<uint32_t>(ng_nb(m));
  if (bytes) *bytes = c.at;
  return w;
}
size_t mesh_sample_work_bytes(uint64_t m) { size_t b; ms_work(nullptr, (size_t)m, &b); return b; }

// the 32-bit mixer (geometry.py: mix32 / sample_hash state the same one)
__device__ __forceinline__ uint32_t ms_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t ms_hash(uint32_t seed, uint32_t t, uint32_t k) { return ms_mix(ms_mix(ms_mix(seed ^ 0x9e3779b9u) + t) + k); }

struct MsTri { double a[3], e1[3], e2[3]; uint32_t rgba[3]; };

// the corners of triangle t widened to double; false: an index outside [0, n_vertices) or a corner that is not finite
__device__ __forceinline__ bool ms_load(const MeshSample& ms, uint32_t t, MsTri& T) {
#pragma clang fp contract(off)
  const int i0 = ms.tris[3 * (size_t)t], i1 = ms.tris[3 * (size_t)t + 1], i2 = ms.tris[3 * (size_t)t + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || (unsigned)i0 >= ms.n_vertices || (unsigned)i1 >= ms.n_vertices || (unsigned)i2 >= ms.n_vertices) return false;
  const uint4 a = ms.vrows[i0], b = ms.vrows[i1], c = ms.vrows[i2];
  const float af[3] = {__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)};
  const float bf[3] = {__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z)};
  const float cf[3] = {__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z)};
  if (!view_finite(af[0], af[1], af[2]) || !view_finite(bf[0], bf[1], bf[2]) || !view_finite(cf[0], cf[1], cf[2])) return false;
  for (int k = 0; k < 3; k++) {
    T.a[k] = (double)af[k];
    T.e1[k] = (double)bf[k] - (double)af[k];
    T.e2[k] = (double)cf[k] - (double)af[k];
  }
  T.rgba[0] = a.w; T.rgba[1] = b.w; T.rgba[2] = c.w;
  return true;
}

// the face cross product c = (b - a) x (c - a) of loaded corners: the one statement behind the sampler's area, the normal consistency and
// the vertex normals
__device__ __forceinline__ void ms_cross(const MsTri& T, double (&c)[3]) {
#pragma clang fp contract(off)
  c[0] = T.e1[1] * T.e2[2] - T.e1[2] * T.e2[1];
  c[1] = T.e1[2] * T.e2[0] - T.e1[0] * T.e2[2];
  c[2] = T.e1[0] * T.e2[1] - T.e1[1] * T.e2[0];
}
__device__ __forceinline__ double ms_dot(const double (&a)[3], const double (&b)[3]) {
#pragma clang fp contract(off)
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
// c and c . c of triangle t of the mesh; false: t >= m (nothing is read), ms_load rejects it, or c . c is 0 or not finite
__device__ __forceinline__ bool ms_face(const MeshSample& ms, uint32_t t, double (&c)[3], double& cc) {
  MsTri T;
  if (t >= ms.m || !ms_load(ms, t, T)) return false;
  ms_cross(T, c);
  cc = ms_dot(c, c);
  return cc > 0.0 && cc < (double)INFINITY;
}

// n_t = min(floor(A density + u_t), MS_TRI_MAX); 0 and `degenerate` for a triangle ms_load rejects or whose area is 0 or not finite
#define MS_TRI_MAX 8388608.0      // 2^23: a 256-block's total stays below 2^32
__device__ __forceinline__ uint32_t ms_count(const MeshSample& ms, uint32_t t, bool& degenerate) {
#pragma clang fp contract(off)
  MsTri T;
  degenerate = true;
  if (!ms_load(ms, t, T)) return 0u;
  double c[3];
  ms_cross(T, c);
  const double A = 0.5 * sqrt(ms_dot(c, c));
  if (!(A > 0.0) || !(A < (double)INFINITY)) return 0u;
  degenerate = false;
  const double u = (double)ms_hash(ms.seed, t, 0xffffffffu) * 0x1p-32;
  double nt = floor(A * ms.density + u);
  nt = nt < MS_TRI_MAX ? nt : MS_TRI_MAX;
  return (uint32_t)nt;
}

__global__ void __launch_bounds__(GB)
ms_plan_kernel(MeshSample ms, uint32_t* __restrict__ prefix, uint32_t* __restrict__ bcounts, uint32_t* __restrict__ dcounts) {
  __shared__ uint32_t wtot[GB / 64];
  __shared__ uint32_t wdeg[1][GB / 64];
  const uint32_t t = blockIdx.x * GB + threadIdx.x;
  bool deg = false;
  const uint32_t nt = t < ms.m ? ms_count(ms, t, deg) : 0u;
  const uint32_t incl = block_scan_incl(nt, wtot);
  if (t < ms.m) prefix[t] = incl - nt;
  if (threadIdx.x == GB - 1) bcounts[blockIdx.x] = incl;
  const bool is[1] = {deg};
  const uint32_t nd = block_flag_counts(is, wdeg);
  if (threadIdx.x == 0) dcounts[blockIdx.x] = nd;
}

__global__ void __launch_bounds__(1024)
ms_scan_kernel(int nb, uint32_t* __restrict__ bcounts, const uint32_t* __restrict__ dcounts, unsigned long long m, unsigned long long* __restrict__ hdr,
               unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long sh[16];
  __shared__ uint32_t total32;
  // the 64-bit sums first: the scan overwrites the block totals with their prefix
  const unsigned long long total = block_array_sum(nb, bcounts, sh), deg = block_array_sum(nb, dcounts, sh);
  scan_block_counts(nb, bcounts, &total32);
  if (threadIdx.x == 0) {
    const bool over = total > 0xffffffffull;      // the prefix is 32 bits wide: nothing can be emitted
    hdr[0] = over ? 0ull : total;
    counters[0] = total;
    counters[1] = deg;
    counters[2] = 0ull;
    counters[3] = 0ull;
    counters[4] = m;
    counters[5] = 0ull;
    counters[6] = over ? 1ull : 0ull;
    counters[7] = 0ull;
  }
}

__global__ void __launch_bounds__(GB) ms_base_kernel(uint32_t m, const uint32_t* __restrict__ bpre, uint32_t* __restrict__ prefix) {
  const uint32_t t = blockIdx.x * GB + threadIdx.x;
  if (t < m) prefix[t] += bpre[blockIdx.x];
}

void launch_mesh_sample_plan(const MeshSample& ms, void* work, uint64_t* counters, hipStream_t s) {
  const MsWork w = ms_work(work, (size_t)ms.m);
  const unsigned nb = (unsigned)ng_nb((size_t)ms.m);
  hipLaunchKernelGGL(ms_plan_kernel, dim3(nb), dim3(GB), 0, s, ms, w.prefix, w.bcounts, w.dcounts);
  hipLaunchKernelGGL(ms_scan_kernel, dim3(1), dim3(1024), 0, s, (int)nb, w.bcounts, w.dcounts, (unsigned long long)ms.m, w.hdr, (unsigned long long*)counters);
  hipLaunchKernelGGL(ms_base_kernel, dim3(nb), dim3(GB), 0, s, ms.m, w.bcounts, w.prefix);
}

template <bool TRI>
__global__ void __launch_bounds__(GB)
ms_emit_kernel(MeshSample ms, const uint32_t* __restrict__ prefix, const unsigned long long* __restrict__ hdr, unsigned long long cap, uint4* __restrict__ rows,
               uint32_t* __restrict__ tri_out, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  const unsigned long long total = hdr[0], written = total < cap ? total : cap;
  const unsigned long long i = (unsigned long long)blockIdx.x * GB + threadIdx.x;
  if (i == 0) {
    counters[2] = written;
    counters[3] = total - written;
  }
  if (i >= written) return;
  // the triangle of sample i: the last t with prefix[t] <= i (a triangle without samples shares its prefix with its successor)
  uint32_t lo = 0u, hi = ms.m;      // prefix[lo] <= i; hi: first index known to be beyond
  for (int step = 0; step < 32 && hi - lo > 1u; step++) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if ((unsigned long long)prefix[mid] <= i) lo = mid; else hi = mid;
  }
  const uint32_t t = lo, j = (uint32_t)(i - prefix[t]);
  MsTri T;
  if (!ms_load(ms, t, T)) return;      // (a triangle with samples passed this test in the plan)
  double r1 = (double)ms_hash(ms.seed, t, 2u * j) * 0x1p-32, r2 = (double)ms_hash(ms.seed, t, 2u * j + 1u) * 0x1p-32;
  if (r1 + r2 > 1.0) { r1 = 1.0 - r1; r2 = 1.0 - r2; }
  const double w0 = 1.0 - r1 - r2;      // exact: multiples of 2^-32
  const float px = (float)(T.a[0] + r1 * T.e1[0] + r2 * T.e2[0]);
  const float py = (float)(T.a[1] + r1 * T.e1[1] + r2 * T.e2[1]);
  const float pz = (float)(T.a[2] + r1 * T.e1[2] + r2 * T.e2[2]);
  const uint32_t rgba = (w0 >= r1 && w0 >= r2) ? T.rgba[0] : (r1 >= r2 ? T.rgba[1] : T.rgba[2]);      // the largest weight, lowest index on a tie
  rows[i] = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), rgba);      // one 16-byte store
  if (TRI) tri_out[i] = t;
}

// tri_out_or_null selects ms_emit_kernel<true>
void launch_mesh_sample_emit(const MeshSample& ms, const void* work, void* rows, uint32_t* tri_out_or_null, uint64_t cap, uint64_t* counters, hipStream_t s) {
  const MsWork w = ms_work((void*)work, (size_t)ms.m);
  size_t nb = ng_nb((size_t)cap);
  nb = nb < 1 ? 1 : nb;
  hipLaunchKernelGGL(tri_out_or_null ? ms_emit_kernel<true> : ms_emit_kernel<false>, dim3((unsigned)nb), dim3(GB), 0, s, ms, w.prefix, w.hdr, (unsigned long long)cap,
                     (uint4*)rows, tri_out_or_null, (unsigned long long*)counters);
}

// ---- normal consistency ---------------------------------------------------------------------------------------------------------------
// nc_dot_kernel, one lane per query: the faces of its own triangle and of its nearest row's triangle, their normalised dot product clamped
// to [-1, 1] and rounded once at the store; per workgroup one partial row {sum |dot|, sum dot, min |dot|, n, -, no neighbour, bad triangle, -}
// over the stored values, in ng_query_kernel's order; ng_finish_kernel<true> adds the partial rows.
size_t normal_consistency_work_bytes(uint64_t n_q) { return nn_query_work_bytes(n_q); }

__global__ void __launch_bounds__(GB)
nc_dot_kernel(uint32_t n_q, const uint32_t* __restrict__ tri_q, const uint32_t* __restrict__ index, uint32_t n_r, const uint32_t* __restrict__ tri_r,
              MeshSample mq, MeshSample mr, float* __restrict__ dot_out, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[GB / 64][2];
  __shared__ uint32_t wcnt[3][GB / 64];
  __shared__ uint32_t smin;
  const uint32_t i = blockIdx.x * GB + threadIdx.x;
  if (threadIdx.x == 0) smin = 0x7f800000u;      // +inf
  __syncthreads();
  bool counted = false, none = false, bad = false;
  double dd = 0.0;
  if (i < n_q) {
    const uint32_t j = index[i];
    float out = __uint_as_float(0x7fc00000u);
    if (j == NN_NO_CELL) {
      none = true;
    } else {
      double cq[3], cr[3], qq = 0.0, rr = 0.0;
      bad = true;
      if (j < n_r && ms_face(mq, tri_q[i], cq, qq) && ms_face(mr, tri_r[j], cr, rr)) {      // (ms_face reads nothing for an id >= m)
        double d = ms_dot(cq, cr) / (sqrt(qq) * sqrt(rr));
        d = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);
        out = (float)d;      // the one rounding
        if (out == out) {
          bad = false;
          counted = true;
          dd = (double)out;
          atomicMin(&smin, __float_as_uint(fabsf(out)));      // LDS, integer: a non-negative float orders as its bits
        }
      }
    }
    dot_out[i] = out;
  }
  double sums[2] = {fabs(dd), dd};
  block_sums_f64<2, false>(sums, wsum);
  const bool is[3] = {counted, none, bad};
  const uint32_t cnt = block_flag_counts(is, wcnt);
  double* row = partial + (size_t)blockIdx.x * NN_ROW;
  if (threadIdx.x == 0) row[3] = (double)cnt;
  if (threadIdx.x == 1 || threadIdx.x == 2) row[4 + threadIdx.x] = (double)cnt;
  if (threadIdx.x == 0) {
    row[0] = sums[0];
    row[1] = sums[1];
    row[2] = (double)__uint_as_float(smin);
    row[4] = 0.0;
    row[7] = 0.0;
  }
}

void launch_normal_consistency(uint64_t n_q, const uint32_t* tri_q, const uint32_t* index, uint64_t n_r, const uint32_t* tri_r, const MeshSample& mq,
                               const MeshSample& mr, float* dot_out, double* row, void* work, hipStream_t s) {
  const unsigned nb = (unsigned)ng_nb((size_t)n_q);
  hipLaunchKernelGGL(nc_dot_kernel, dim3(nb), dim3(GB), 0, s, (uint32_t)n_q, tri_q, index, (uint32_t)n_r, tri_r, mq, mr, dot_out, (double*)work);
  hipLaunchKernelGGL(ng_finish_kernel<true>, dim3(1), dim3(GB), 0, s, (const double*)work, (int)nb, row);
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------------------
// Area-weighted (the face cross product is twice the area times the unit normal), accumulated in fixed point: integer adds commute, so no
// order of arrival changes a bit.  E_v = the largest frexp exponent among the faces at v, every face adds llrint(c 2^(40 - E_v)) to three
// int64 sums: a term is below 2^40 in magnitude, so a valence up to 2^22 cannot overflow; beyond it the sums wrap (two's complement).
//   vn_zero_kernel    E_v = VN_NO_EXP, S_v = 0, the counters to zero.
//   vn_exp_kernel     one lane per triangle: integer atomicMax on the three E_v; the rejected triangles are counted.
//   vn_add_kernel     one lane per triangle: three 64-bit integer atomicAdd per corner.
//   vn_finish_kernel  one lane per vertex: n_v = S_v / sqrt(S_v . S_v) in double, one rounding; the vertices without a normal are counted.
// work = [int32 E per vertex][int64 S x 3 per vertex]
#define VN_NO_EXP (-0x7fffffff - 1)
#define VN_FRAC_BITS 40
struct VnWork { int* E; unsigned long long* S; };
static VnWork vn_work(void* base, size_t nv, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  VnWork w;
  w.E = c.take<int>(nv);
  w.S = c.take<unsigned long long>(3 * nv);
  if (bytes) *bytes = c.at;
  return w;
}
size_t mesh_vertex_normals_work_bytes(uint64_t n_vertices) { size_t b; vn_work(nullptr, (size_t)n_vertices, &b); return b; }

__global__ void __launch_bounds__(GB) vn_zero_kernel(uint32_t nv, int* __restrict__ E, unsigned long long* __restrict__ S, unsigned long long* __restrict__ counters) {
  const uint32_t v = blockIdx.x * GB + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 8) counters[threadIdx.x] = threadIdx.x == 0 ? (unsigned long long)nv : 0ull;
  if (v >= nv) return;
  E[v] = VN_NO_EXP;
  S[3 * (size_t)v] = 0ull; S[3 * (size_t)v + 1] = 0ull; S[3 * (size_t)v + 2] = 0ull;
}

// the corners of triangle t (valid once ms_face has accepted it)
__device__ __forceinline__ void vn_corners(const MeshSample& ms, uint32_t t, uint32_t (&v)[3]) {
  for (int k = 0; k < 3; k++) v[k] = (uint32_t)ms.tris[3 * (size_t)t + k];
}

__global__ void __launch_bounds__(GB) vn_exp_kernel(MeshSample ms, int* __restrict__ E, unsigned long long* __restrict__ counters) {
  const uint32_t t = blockIdx.x * GB + threadIdx.x;
  bool rejected = false;
  if (t < ms.m) {
    double c[3], cc;
    if (ms_face(ms, t, c, cc)) {
      const double ax = fabs(c[0]), ay = fabs(c[1]), az = fabs(c[2]);
      const double mx = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
      int e;
      frexp(mx, &e);
      uint32_t v[3];
      vn_corners(ms, t, v);
      for (int k = 0; k < 3; k++) atomicMax(&E[v[k]], e);      // integer: a maximum does not depend on the order
    } else {
      rejected = true;
    }
  }
  const unsigned long long mr = __ballot(rejected);
  if ((threadIdx.x & 63) == 0 && mr) atomicAdd(counters + 2, (unsigned long long)__popcll(mr));      // integer adds: any order
}

__global__ void __launch_bounds__(GB) vn_add_kernel(MeshSample ms, const int* __restrict__ E, unsigned long long* __restrict__ S) {
  const uint32_t t = blockIdx.x * GB + threadIdx.x;
  if (t >= ms.m) return;
  double c[3], cc;
  if (!ms_face(ms, t, c, cc)) return;
  uint32_t v[3];
  vn_corners(ms, t, v);
  for (int k = 0; k < 3; k++) {
    const int sh = VN_FRAC_BITS - E[v[k]];      // E_v >= this face's exponent: |c 2^sh| < 2^40
    for (int a = 0; a < 3; a++) atomicAdd(&S[3 * (size_t)v[k] + a], (unsigned long long)llrint(ldexp(c[a], sh)));      // wraps as int64 does
  }
}

__global__ void __launch_bounds__(GB)
vn_finish_kernel(uint32_t nv, const int* __restrict__ E, const unsigned long long* __restrict__ S, float* __restrict__ normals, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  const uint32_t v = blockIdx.x * GB + threadIdx.x;
  bool without = false;
  if (v < nv) {
    const double s[3] = {(double)(long long)S[3 * (size_t)v], (double)(long long)S[3 * (size_t)v + 1], (double)(long long)S[3 * (size_t)v + 2]};
    const double ss = ms_dot(s, s);
    float n[3] = {0.f, 0.f, 0.f};
    if (E[v] != VN_NO_EXP && ss > 0.0) {
      const double len = sqrt(ss);
      for (int a = 0; a < 3; a++) n[a] = (float)(s[a] / len);      // the one rounding
    } else {
      without = true;
    }
    for (int a = 0; a < 3; a++) normals[3 * (size_t)v + a] = n[a];
  }
  const unsigned long long mw = __ballot(without);
  if ((threadIdx.x & 63) == 0 && mw) atomicAdd(counters + 1, (unsigned long long)__popcll(mw));
}

void launch_mesh_vertex_normals(const MeshSample& ms, float* normals, void* work, uint64_t* counters, hipStream_t s) {
  const VnWork w = vn_work(work, (size_t)ms.n_vertices);
  const unsigned nbv = (unsigned)ng_nb((size_t)ms.n_vertices), nbt = (unsigned)ng_nb((size_t)ms.m);
  unsigned long long* cn = (unsigned long long*)counters;
  hipLaunchKernelGGL(vn_zero_kernel, dim3(nbv), dim3(GB), 0, s, ms.n_vertices, w.E, w.S, cn);
  hipLaunchKernelGGL(vn_exp_kernel, dim3(nbt), dim3(GB), 0, s, ms, w.E, cn);
  hipLaunchKernelGGL(vn_add_kernel, dim3(nbt), dim3(GB), 0, s, ms, (const int*)w.E, w.S);
  hipLaunchKernelGGL(vn_finish_kernel, dim3(nbv), dim3(GB), 0, s, ms.n_vertices, (const int*)w.E, (const unsigned long long*)w.S, normals, cn);
}

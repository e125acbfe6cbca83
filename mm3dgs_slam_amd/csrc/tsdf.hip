// The reconstruction as a coloured triangle mesh (mm3dgs_tsdf_integrate / mm3dgs_tsdf_mesh_plan / mm3dgs_tsdf_mesh_emit; host statement:
// mesh.integrate_host / mesh.mesh_host).  The volume is the caller's: tsdf_w float2 [nz][ny][nx] {truncated distance in [-1, 1], weight} and
// rgb_w float4 [nz][ny][nx] {mean colour, colour weight} over a lattice of sample points origin + voxel (i, j, k), x fastest; zeros = empty.
//
//   tsdf_integrate_kernel   one launch per view, one lane per sample and slice, 64 consecutive x per wave (workgroup = 64 x by 4 y, walking
//                           up to 8 z slices).  The sample is projected into the view in double (no contraction, so the host statement
//                           rounds alike); z <= 0, a pixel outside the image or one that fails the point cloud's validity test
//                           (view_pixel.h), or sdf < -trunc end the sample before anything is loaded from the volume: free space outside
//                           the frustum costs arithmetic only.  Running means, rounded to float32 once at the 8- and 16-byte stores.
//                           Counters: one integer add per workgroup and counter (with one per wave and slice, all of them on one word,
//                           the adds were what a view cost: 832 us against 86 us over 256^3 samples, profiles/r15_mesh.jsonl).
//   marching tetrahedra     every cube is cut into the six Kuhn tetrahedra (the monotone corner paths 0 -> 7, one per axis permutation),
//                           the same cut in every cube.  Plan: tm_state (known / inside bits per sample), tm_cube (valid cubes and their
//                           triangle counts), tm_edge (per sample the 7-bit mask of the directions d whose edge (q, d) carries a vertex:
//                           endpoints differ in `inside` and one of the up to four cubes around the edge is valid -- gathered, no atomic),
//                           tm_scan (one workgroup: scan_block_counts over both per-256 counts, the totals), tm_base (per-sample vertex base
//                           and per-cube triangle base).  Emit: tm_vertex (one 16-byte row per vertex at base[q] + popcount(mask[q] below d)),
//                           tm_triangle (int32[3] per triangle, by tetrahedron then case order).  No atomic decides a position or an index.
//                           The cube, edge, vertex and triangle kernels are tsdf_march.h's, instantiated here over the dense lattice
//                           (TmGrid: a stride to a neighbour, none beyond the lattice, 32-bit index arithmetic); state, scan and base
//                           see only the flat run of samples and are defined here for both volumes.
#include <math.h>
#include "tsdf_sample.h"      // the per-sample update (shared with tsdf_sparse.hip)
#include "tsdf_march.h"       // the extraction over a lattice (shared with tsdf_sparse.hip)

#define TB TM_TB

// ---- integration ----------------------------------------------------------------------------------------------------------------
#define TZ 8      // z slices per workgroup: one add per workgroup and counter instead of one per wave and slice (every add lands on the same word)

__global__ void __launch_bounds__(TB)
tsdf_integrate_kernel(TsdfView v, float2* __restrict__ tsdf_w, float4* __restrict__ rgb_w, unsigned long long* __restrict__ counters, unsigned xb,
                      unsigned yb) {
#pragma clang fp contract(off)
  __shared__ Rigid g;
  __shared__ uint32_t wsum[2][TB / 64];
  const unsigned b = blockIdx.x;
  const int i = (int)(b % xb) * 64 + (int)(threadIdx.x & 63);
  const int j = (int)((b / xb) % yb) * 4 + (int)(threadIdx.x >> 6);
  const int k0 = (int)(b / (xb * yb)) * TZ;
  view_rigid_shared(v.pose, g);
  uint32_t nupd = 0, ncup = 0;
  if (i < v.nx && j < v.ny) {
    const size_t hw = (size_t)v.H * (size_t)v.W;
    const double pw0 = v.o[0] + v.voxel * (double)i, pw1 = v.o[1] + v.voxel * (double)j;
    for (int k = k0; k < k0 + TZ && k < v.nz; k++) {
      const double pw2 = v.o[2] + v.voxel * (double)k;
      const size_t q = ((size_t)k * (size_t)v.ny + (size_t)j) * (size_t)v.nx + (size_t)i;
      tsdf_sample_update(v, g, hw, pw0, pw1, pw2, tsdf_w + q, rgb_w + q, nupd, ncup);
    }
  }
  const uint32_t nn[2] = {nupd, ncup};
  const uint32_t t = block_sums_u32(nn, wsum);      // (every lane is here)
  if (threadIdx.x < 2 && t) atomicAdd(counters + 1 + threadIdx.x, (unsigned long long)t);
  if (threadIdx.x == 0 && b == 0) atomicAdd(counters, 1ull);
}

void launch_tsdf_integrate(const TsdfView& v, void* tsdf_w, void* rgb_w, uint64_t* counters, hipStream_t s) {
  const unsigned xb = (unsigned)((v.nx + 63) / 64), yb = (unsigned)((v.ny + 3) / 4), zb = (unsigned)((v.nz + TZ - 1) / TZ);
  const size_t nb = (size_t)xb * yb * zb;      // <= 2^30 / 2 / 2: within the grid's 2^31 - 1
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)nb), dim3(TB), 0, s, v, (float2*)tsdf_w, (float4*)rgb_w, (unsigned long long*)counters, xb, yb);
}

// ---- marching tetrahedra --------------------------------------------------------------------------------------------------------
size_t tsdf_mesh_work_bytes(int nx, int ny, int nz) { size_t b; tm_work(nullptr, (size_t)nx * (size_t)ny * (size_t)nz, &b); return b; }

// the dense lattice: sample (x, y, z) at flat index (z ny + y) nx + x; beyond 0 .. nx - 1 (ny, nz) there is no sample.  n <= 2^30 (the entry
// points have checked): a flat index and a step of one row and one slice fit 32 bits, which spares every lane 64-bit divisions
struct TmGrid {
  struct Cell { int i, x, y, z; };
  int nx, ny, nz;
  size_t n;
  __device__ __forceinline__ Cell cell(size_t i) const {
    const unsigned u = (unsigned)i, row = u / (unsigned)nx;
    return {(int)u, (int)(u % (unsigned)nx), (int)(row % (unsigned)ny), (int)(row / (unsigned)ny)};
  }
  __device__ __forceinline__ long long at(const Cell& c, int dx, int dy, int dz) const {
    if ((unsigned)(c.x + dx) >= (unsigned)nx || (unsigned)(c.y + dy) >= (unsigned)ny || (unsigned)(c.z + dz) >= (unsigned)nz) return -1;
    return c.i + dx + (dy + dz * ny) * nx;
  }
  __device__ __forceinline__ void lattice_index(const Cell& c, int q[3]) const { q[0] = c.x; q[1] = c.y; q[2] = c.z; }
  __device__ __forceinline__ bool cube(const Cell& c, long long q[8]) const {
    if (c.x >= nx - 1 || c.y >= ny - 1 || c.z >= nz - 1) return false;
    for (unsigned e = 0; e < 8; e++) q[e] = c.i + (int)(e & 1u) + ((int)((e >> 1) & 1u) + (int)((e >> 2) & 1u) * ny) * nx;
    return true;
  }
};
static TmGrid tm_grid(int nx, int ny, int nz) { return {nx, ny, nz, (size_t)nx * (size_t)ny * (size_t)nz}; }

__global__ void __launch_bounds__(TB) tm_state_kernel(size_t n, const float2* __restrict__ tsdf_w, float min_weight, uint8_t* __restrict__ state) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const float2 tw = tsdf_w[i];
  state[i] = (uint8_t)((tw.y >= min_weight ? 1 : 0) | (tw.x < 0.f ? 2 : 0));      // (a NaN weight is not known)
}

__global__ void __launch_bounds__(1024)
tm_scan_kernel(int nb, uint32_t* __restrict__ vcounts, uint32_t* __restrict__ tcounts, unsigned long long* __restrict__ hdr, unsigned long long* __restrict__ counters) {
  __shared__ uint32_t totals[2];
  scan_block_counts(nb, vcounts, &totals[0]);
  __syncthreads();
  scan_block_counts(nb, tcounts, &totals[1]);
  if (threadIdx.x == 0) {      // (lane 0 wrote both totals itself)
    hdr[0] = totals[0];
    hdr[1] = totals[1];
    counters[0] = totals[0];
    counters[1] = totals[1];
  }
  if (threadIdx.x >= 2 && threadIdx.x < 8) counters[threadIdx.x] = 0ull;
}

__global__ void __launch_bounds__(TB)
tm_base_kernel(size_t n, const uint8_t* __restrict__ cube, const uint8_t* __restrict__ vmask, const uint32_t* __restrict__ vpre, const uint32_t* __restrict__ tpre,
               uint32_t* __restrict__ vbase, uint32_t* __restrict__ tbase) {
  __shared__ uint32_t wv[TB / 64], wt[TB / 64];
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  const uint32_t nv = i < n ? (uint32_t)__popc((unsigned)vmask[i]) : 0u, nt = i < n ? (uint32_t)(cube[i] & 0x7fu) : 0u;
  const uint32_t iv = block_scan_incl(nv, wv), it = block_scan_incl(nt, wt);
  if (i < n) {
    vbase[i] = vpre[blockIdx.x] + iv - nv;
    tbase[i] = tpre[blockIdx.x] + it - nt;
  }
}

void launch_tm_state(size_t n, const void* tsdf_w, float min_weight, const TmWork& w, hipStream_t s) {
  hipLaunchKernelGGL(tm_state_kernel, dim3((unsigned)tm_nb(n)), dim3(TB), 0, s, n, (const float2*)tsdf_w, min_weight, w.state);
}

void launch_tm_scan_base(size_t n, const TmWork& w, uint64_t* counters, hipStream_t s) {
  const unsigned nb = (unsigned)tm_nb(n);
  hipLaunchKernelGGL(tm_scan_kernel, dim3(1), dim3(1024), 0, s, (int)nb, w.vcounts, w.tcounts, w.hdr, (unsigned long long*)counters);
  hipLaunchKernelGGL(tm_base_kernel, dim3(nb), dim3(TB), 0, s, n, w.cube, w.vmask, w.vcounts, w.tcounts, w.vbase, w.tbase);
}

void launch_tsdf_mesh_plan(int nx, int ny, int nz, const void* tsdf_w, float min_weight, void* work, uint64_t* counters, hipStream_t s) {
  tm_launch_plan(tm_grid(nx, ny, nz), tsdf_w, min_weight, work, counters, s);
}

void launch_tsdf_mesh_emit(int nx, int ny, int nz, const void* tsdf_w, const void* rgb_w, const double* origin, double voxel, const void* work, void* rows,
                           uint64_t vcap, void* tris, uint64_t tcap, uint64_t* counters, hipStream_t s) {
  tm_launch_emit(tm_grid(nx, ny, nz), tsdf_w, rgb_w, origin, voxel, work, rows, vcap, tris, tcap, counters, s);
}

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
#include <math.h>
#include "tsdf_sample.h"      // the per-sample update, the case tables and the work layout (shared with tsdf_sparse.hip)

#define TB TM_TB

// ---- integration ----------------------------------------------------------------------------------------------------------------
#define TZ 8      // z slices per workgroup: one add per workgroup and counter instead of one per wave and slice (every add lands on the same word)

__global__ void __launch_bounds__(TB)
tsdf_integrate_kernel(TsdfView v, float2* __restrict__ tsdf_w, float4* __restrict__ rgb_w, unsigned long long* __restrict__ counters, unsigned xb,
                      unsigned yb) {
#pragma clang fp contract(off)
  __shared__ Rigid g;      // the pose is the same for every sample: one lane normalises the quaternion for its workgroup
  __shared__ uint32_t wsum[2][TB / 64];
  const unsigned b = blockIdx.x;
  const int i = (int)(b % xb) * 64 + (int)(threadIdx.x & 63);
  const int j = (int)((b / xb) % yb) * 4 + (int)(threadIdx.x >> 6);
  const int k0 = (int)(b / (xb * yb)) * TZ;
  if (threadIdx.x == 0) g = rigid_from_pose(v.pose);
  __syncthreads();
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

struct TmGrid { int nx, ny, nz; size_t n; };

__device__ __forceinline__ size_t tm_corner(const TmGrid& g, unsigned c) {
  return (size_t)(c & 1u) + (size_t)((c >> 1) & 1u) * (size_t)g.nx + (size_t)((c >> 2) & 1u) * (size_t)g.nx * (size_t)g.ny;
}

__device__ __forceinline__ void tm_coords(const TmGrid& g, size_t i, int& x, int& y, int& z) {
  x = (int)(i % (size_t)g.nx);
  y = (int)((i / (size_t)g.nx) % (size_t)g.ny);
  z = (int)(i / ((size_t)g.nx * (size_t)g.ny));
}

__global__ void __launch_bounds__(TB) tm_state_kernel(size_t n, const float2* __restrict__ tsdf_w, float min_weight, uint8_t* __restrict__ state) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const float2 tw = tsdf_w[i];
  state[i] = (uint8_t)((tw.y >= min_weight ? 1 : 0) | (tw.x < 0.f ? 2 : 0));      // (a NaN weight is not known)
}

// the 8 corner states of the cube with origin i: all known -> valid; the inside bits by corner number
__device__ __forceinline__ bool tm_cube_corners(const TmGrid& g, const uint8_t* __restrict__ state, size_t i, unsigned& inside) {
  unsigned known = 1;
  inside = 0;
  for (unsigned c = 0; c < 8; c++) {
    const unsigned s = state[i + tm_corner(g, c)];
    known &= s;
    inside |= ((s >> 1) & 1u) << c;
  }
  return (known & 1u) != 0;
}

__global__ void __launch_bounds__(TB) tm_cube_kernel(TmGrid g, const uint8_t* __restrict__ state, uint8_t* __restrict__ cube, uint32_t* __restrict__ tcounts) {
  __shared__ uint32_t wtot[TB / 64];
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  uint32_t ntri = 0;
  uint8_t out = 0;
  if (i < g.n) {
    int x, y, z;
    tm_coords(g, i, x, y, z);
    unsigned inside;
    if (x < g.nx - 1 && y < g.ny - 1 && z < g.nz - 1 && tm_cube_corners(g, state, i, inside)) {
      for (int k = 0; k < 6; k++) ntri += TM_CASES[tm_tet_mask(inside, k)] & 3u;
      out = (uint8_t)(0x80u | ntri);
    }
    cube[i] = out;
  }
  const uint32_t incl = block_scan_incl(ntri, wtot);
  if (threadIdx.x == TB - 1) tcounts[blockIdx.x] = incl;
}

__global__ void __launch_bounds__(TB)
tm_edge_kernel(TmGrid g, const uint8_t* __restrict__ state, const uint8_t* __restrict__ cube, uint8_t* __restrict__ vmask, uint32_t* __restrict__ vcounts) {
  __shared__ uint32_t wtot[TB / 64];
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  unsigned mask = 0;
  if (i < g.n) {
    int x, y, z;
    tm_coords(g, i, x, y, z);
    const unsigned in0 = (state[i] >> 1) & 1u;
    // valid cubes with origin q - e, e in {0,1}^3 (bit e of `around`); a cube beyond the lattice is not valid
    unsigned around = 0;
    for (unsigned e = 0; e < 8; e++) {
      if (((e & 1u) && x == 0) || ((e & 2u) && y == 0) || ((e & 4u) && z == 0)) continue;
      around |= (unsigned)(cube[i - tm_corner(g, e)] >> 7) << e;
    }
    for (unsigned d = 1; d < 8; d++) {
      if (((d & 1u) && x == g.nx - 1) || ((d & 2u) && y == g.ny - 1) || ((d & 4u) && z == g.nz - 1)) continue;
      // the cubes that contain the edge (q, d): origins q - e with e inside the zero bits of d
      unsigned near = 0;
      for (unsigned e = 0; e < 8; e++)
        if (!(e & d)) near |= (around >> e) & 1u;
      const unsigned in1 = (state[i + tm_corner(g, d)] >> 1) & 1u;
      if (near && in0 != in1) mask |= 1u << d;
    }
    vmask[i] = (uint8_t)mask;
  }
  const uint32_t incl = block_scan_incl((uint32_t)__popc(mask), wtot);
  if (threadIdx.x == TB - 1) vcounts[blockIdx.x] = incl;
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
  TmGrid g;
  g.nx = nx; g.ny = ny; g.nz = nz; g.n = (size_t)nx * (size_t)ny * (size_t)nz;
  const TmWork w = tm_work(work, g.n);
  const unsigned nb = (unsigned)tm_nb(g.n);
  launch_tm_state(g.n, tsdf_w, min_weight, w, s);
  hipLaunchKernelGGL(tm_cube_kernel, dim3(nb), dim3(TB), 0, s, g, w.state, w.cube, w.tcounts);
  hipLaunchKernelGGL(tm_edge_kernel, dim3(nb), dim3(TB), 0, s, g, w.state, w.cube, w.vmask, w.vcounts);
  launch_tm_scan_base(g.n, w, counters, s);
}

__global__ void __launch_bounds__(TB)
tm_vertex_kernel(TmGrid g, TmEmit e, const float2* __restrict__ tsdf_w, const float4* __restrict__ rgb_w, const uint8_t* __restrict__ vmask,
                 const uint32_t* __restrict__ vbase, const unsigned long long* __restrict__ hdr, uint4* __restrict__ rows, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i == 0) {      // the counts of this emit: what the caps let through (the triangle kernel adds its two behind the kernel boundary)
    const unsigned long long V = hdr[0], written = V < e.vcap ? V : e.vcap;
    counters[2] = written;
    counters[3] = 0ull;
    counters[4] = V - written;
    counters[5] = 0ull;
  }
  if (i >= g.n) return;
  const unsigned mask = vmask[i];
  if (!mask) return;
  int q[3];
  tm_coords(g, i, q[0], q[1], q[2]);
  const double T0 = (double)tsdf_w[i].x;
  const float4 c0 = rgb_w[i];
  unsigned long long r = vbase[i];
  for (unsigned d = 1; d < 8; d++) {
    if (!((mask >> d) & 1u)) continue;
    if (r < e.vcap) {
      const size_t j = i + tm_corner(g, d);
      const double T1 = (double)tsdf_w[j].x;
      const float4 c1 = rgb_w[j];
      const double t = T0 / (T0 - T1);
      const float px = (float)(e.o[0] + e.voxel * ((double)q[0] + t * (double)(d & 1u)));
      const float py = (float)(e.o[1] + e.voxel * ((double)q[1] + t * (double)((d >> 1) & 1u)));
      const float pz = (float)(e.o[2] + e.voxel * ((double)q[2] + t * (double)((d >> 2) & 1u)));
      const float cr = (float)((double)c0.x + t * ((double)c1.x - (double)c0.x));
      const float cg = (float)((double)c0.y + t * ((double)c1.y - (double)c0.y));
      const float cb = (float)((double)c0.z + t * ((double)c1.z - (double)c0.z));
      rows[r] = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), pc_quant(cr) | (pc_quant(cg) << 8) | (pc_quant(cb) << 16) | 0xff000000u);
    }
    r++;
  }
}

__global__ void __launch_bounds__(TB)
tm_triangle_kernel(TmGrid g, TmEmit e, const uint8_t* __restrict__ state, const uint8_t* __restrict__ cube, const uint8_t* __restrict__ vmask,
                   const uint32_t* __restrict__ vbase, const uint32_t* __restrict__ tbase, int* __restrict__ tris, unsigned long long* __restrict__ counters) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  uint32_t written = 0, dropped = 0;
  if (i < g.n && (cube[i] & 0x7fu)) {      // (a cube with triangles is valid and inside the lattice)
    unsigned inside;
    tm_cube_corners(g, state, i, inside);
    unsigned long long r = tbase[i];
    for (int k = 0; k < 6; k++) {
      const uint32_t cs = TM_CASES[tm_tet_mask(inside, k)];
      const unsigned corner[4] = {0u, TM_MID1[k], TM_MID2[k], 7u};
      for (uint32_t s = 0; s < (cs & 3u); s++) {
        uint32_t idx[3];
        for (int a = 0; a < 3; a++) {
          const unsigned edge = (cs >> (2 + 9 * s + 3 * a)) & 7u;
          const unsigned lo = corner[TM_EDGE_LO[edge]], hi = corner[TM_EDGE_HI[edge]];
          const size_t smp = i + tm_corner(g, lo);
          idx[a] = vbase[smp] + (uint32_t)__popc((unsigned)vmask[smp] & ((1u << (hi ^ lo)) - 1u));
        }
        if ((TM_ODD >> k) & 1u) { const uint32_t t = idx[1]; idx[1] = idx[2]; idx[2] = t; }
        if (r < e.tcap && idx[0] < e.vcap && idx[1] < e.vcap && idx[2] < e.vcap) {
          tris[3 * r] = (int)idx[0];
          tris[3 * r + 1] = (int)idx[1];
          tris[3 * r + 2] = (int)idx[2];
          written++;
        } else {
          dropped++;
        }
        r++;
      }
    }
  }
  const uint32_t sw = wave_scan_incl(written), sd = wave_scan_incl(dropped);
  if ((threadIdx.x & 63) == 63) {
    if (sw) atomicAdd(counters + 3, (unsigned long long)sw);
    if (sd) atomicAdd(counters + 5, (unsigned long long)sd);
  }
}

void launch_tsdf_mesh_emit(int nx, int ny, int nz, const void* tsdf_w, const void* rgb_w, const double* origin, double voxel, const void* work, void* rows,
                           uint64_t vcap, void* tris, uint64_t tcap, uint64_t* counters, hipStream_t s) {
  TmGrid g;
  g.nx = nx; g.ny = ny; g.nz = nz; g.n = (size_t)nx * (size_t)ny * (size_t)nz;
  const TmWork w = tm_work((void*)work, g.n);
  TmEmit e;
  e.o[0] = origin[0]; e.o[1] = origin[1]; e.o[2] = origin[2]; e.voxel = voxel; e.vcap = vcap; e.tcap = tcap;
  const unsigned nb = (unsigned)tm_nb(g.n);
  hipLaunchKernelGGL(tm_vertex_kernel, dim3(nb), dim3(TB), 0, s, g, e, (const float2*)tsdf_w, (const float4*)rgb_w, w.vmask, w.vbase, w.hdr, (uint4*)rows,
                     (unsigned long long*)counters);
  hipLaunchKernelGGL(tm_triangle_kernel, dim3(nb), dim3(TB), 0, s, g, e, w.state, w.cube, w.vmask, w.vbase, w.tbase, (int*)tris, (unsigned long long*)counters);
}

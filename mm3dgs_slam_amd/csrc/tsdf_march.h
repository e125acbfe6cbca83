// Marching tetrahedra over a flat run of n samples, stated once for the dense volume (tsdf.hip) and the voxel-block volume
// (tsdf_sparse.hip): the work buffer, the case tables, the four kernels that know where a sample's neighbours are (cube, edge, vertex,
// triangle) as templates over a lattice, and the two launch sequences.  A lattice is a small struct passed by value that answers
//   n                     the length of the flat run the work buffer covers
//   cell(i)               the cell (type L::Cell) of flat index i < n
//   at(c, dx, dy, dz)     the flat index of the sample at offset (dx, dy, dz), each in {-1, 0, 1}, from cell c; -1 where there is none
//   lattice_index(c, q)   the signed index q[3] of cell c: the sample sits at o + voxel q
//   cube(c, q)            whether all 8 corners of the cube with origin c are there, and then their flat indices q[8] by corner number, as
//                         at() gives them: one test in front of the cube's eight loads instead of one in front of each
// and nothing else differs between the two volumes: the valid-cube rule, the edge rule, the vertex placement and the triangle indexing are
// the text below.  The kernels that see only the flat run (state, scan, base) are not templates; they stay in tsdf.hip.
#pragma once
#include "block_ops.h"
#include "fused_api.h"
#include "view_pixel.h"

// ---- the work buffer over n samples ------------------------------------------------------------------------------------------------
#define TM_TB 256
// work = [256 B header: uint64 vertices, triangles][state byte per sample: bit 0 known, bit 1 inside][cube byte per sample: 0x80 valid | triangles]
//        [edge mask byte per sample: bit d][uint32 vertex base per sample][uint32 triangle base per cube][per-256 vertex counts][per-256 triangle counts]
struct TmWork { unsigned long long* hdr; uint8_t* state; uint8_t* cube; uint8_t* vmask; uint32_t* vbase; uint32_t* tbase; uint32_t* vcounts; uint32_t* tcounts; };
static inline size_t tm_nb(size_t n) { return (n + TM_TB - 1) / TM_TB; }
static inline TmWork tm_work(void* base, size_t n, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  TmWork w;
  w.hdr = c.take<unsigned long long>(2);
  w.state = c.take<uint8_t>(n);
  w.cube = c.take<uint8_t>(n);
  w.vmask = c.take<uint8_t>(n);
  w.vbase = c.take<uint32_t>(n);
  w.tbase = c.take<uint32_t>(n);
  w.vcounts = c.take<uint32_t>(tm_nb(n));
  w.tcounts = c.take<uint32_t>(tm_nb(n));
  if (bytes) *bytes = c.at;
  return w;
}
struct TmEmit { double o[3], voxel; unsigned long long vcap, tcap; };

// the two ends of a plan that see only the flat run of n samples (tsdf.hip): the state bytes before the cubes and edges are counted, and
// the scan of both per-256 counts with the per-sample bases behind them
void launch_tm_state(size_t n, const void* tsdf_w, float min_weight, const TmWork& w, hipStream_t s);
void launch_tm_scan_base(size_t n, const TmWork& w, uint64_t* counters, hipStream_t s);

// ---- the case tables ---------------------------------------------------------------------------------------------------------------
// The triangles of a positively oriented tetrahedron by its 4-bit inside mask (bit v: vertex v of the path is inside), as
// count | six 3-bit edge ids << 2; edges 0..5 = the vertex pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  One vertex apart: the triangle of its
// three edges; two and two: the quadrilateral (a,c) (a,d) (b,d) (b,c) as two triangles; wound so that the normal points from the inside
// vertices to the outside ones (mesh.py derives the same table by rule and checks the winding numerically).
#define TM1(a, b, c) (1u | (a##u << 2) | (b##u << 5) | (c##u << 8))
#define TM2(a, b, c, d, e, f) (2u | (a##u << 2) | (b##u << 5) | (c##u << 8) | (d##u << 11) | (e##u << 14) | (f##u << 17))
static __device__ const uint32_t TM_CASES[16] = {0u, TM1(0, 1, 2), TM1(0, 4, 3), TM2(1, 2, 4, 1, 4, 3), TM1(1, 3, 5), TM2(0, 5, 2, 0, 3, 5), TM2(0, 4, 5, 0, 5, 1),
                                                 TM1(2, 4, 5), TM1(2, 5, 4), TM2(0, 1, 5, 0, 5, 4), TM2(0, 5, 3, 0, 2, 5), TM1(1, 5, 3), TM2(1, 3, 4, 1, 4, 2),
                                                 TM1(0, 3, 4), TM1(0, 2, 1), 0u};
// cube corners (bit 0 x, bit 1 y, bit 2 z) of the path's two middle vertices, by tetrahedron = axis permutation in lexicographic order:
// (x,y,z) (x,z,y) (y,x,z) (y,z,x) (z,x,y) (z,y,x); the odd permutations (1, 2, 5) mirror the tetrahedron: their triangles swap two corners
static __device__ const uint8_t TM_MID1[6] = {1, 1, 2, 2, 4, 4};
static __device__ const uint8_t TM_MID2[6] = {3, 5, 3, 6, 5, 6};
#define TM_ODD 0x26u
static __device__ const uint8_t TM_EDGE_LO[6] = {0, 0, 0, 1, 1, 2};
static __device__ const uint8_t TM_EDGE_HI[6] = {1, 2, 3, 2, 3, 3};

__device__ __forceinline__ unsigned tm_tet_mask(unsigned inside, int k) {
  return (inside & 1u) | (((inside >> TM_MID1[k]) & 1u) << 1) | (((inside >> TM_MID2[k]) & 1u) << 2) | (((inside >> 7) & 1u) << 3);
}

// ---- the plan's two lattice kernels ------------------------------------------------------------------------------------------------
// the sample one cube corner e (bit 0 x, bit 1 y, bit 2 z) ahead of cell c (sign = 1) or behind it (sign = -1), or -1
template <class L>
__device__ __forceinline__ long long tm_at(const L& g, const typename L::Cell& c, unsigned e, int sign) {
  return g.at(c, sign * (int)(e & 1u), sign * (int)((e >> 1) & 1u), sign * (int)((e >> 2) & 1u));
}

// the 8 corner states of the cube with origin c: all there and known -> valid, and then the inside bits by corner number
template <class L>
__device__ __forceinline__ bool tm_cube_corners(const L& g, const uint8_t* __restrict__ state, const typename L::Cell& c, unsigned& inside) {
  long long q[8];
  inside = 0;
  if (!g.cube(c, q)) return false;
  unsigned known = 1;
  for (unsigned e = 0; e < 8; e++) {
    const unsigned s = state[q[e]];
    known &= s;
    inside |= ((s >> 1) & 1u) << e;
  }
  return (known & 1u) != 0;
}

template <class L>
__global__ void __launch_bounds__(TM_TB) tm_cube_kernel(L g, const uint8_t* __restrict__ state, uint8_t* __restrict__ cube, uint32_t* __restrict__ tcounts) {
  __shared__ uint32_t wtot[TM_TB / 64];
  const size_t i = (size_t)blockIdx.x * TM_TB + threadIdx.x;
  uint32_t ntri = 0;
  if (i < g.n) {
    uint8_t out = 0;
    unsigned inside;
    if (tm_cube_corners(g, state, g.cell(i), inside)) {
      for (int k = 0; k < 6; k++) ntri += TM_CASES[tm_tet_mask(inside, k)] & 3u;
      out = (uint8_t)(0x80u | ntri);
    }
    cube[i] = out;
  }
  const uint32_t incl = block_scan_incl(ntri, wtot);      // (every lane is here)
  if (threadIdx.x == TM_TB - 1) tcounts[blockIdx.x] = incl;
}

template <class L>
__global__ void __launch_bounds__(TM_TB)
tm_edge_kernel(L g, const uint8_t* __restrict__ state, const uint8_t* __restrict__ cube, uint8_t* __restrict__ vmask, uint32_t* __restrict__ vcounts) {
  __shared__ uint32_t wtot[TM_TB / 64];
  const size_t i = (size_t)blockIdx.x * TM_TB + threadIdx.x;
  unsigned mask = 0;
  if (i < g.n) {
    const typename L::Cell c = g.cell(i);
    const unsigned in0 = (state[i] >> 1) & 1u;
    // a neighbour that is not there is read as sample i itself and then left out: fifteen loads in flight instead of a branch in front of each
    // valid cubes with origin q - e, e in {0,1}^3 (bit e of `around`); a cube whose origin is not there is not valid
    unsigned around = 0;
    for (unsigned e = 0; e < 8; e++) {
      const long long q = tm_at(g, c, e, -1);
      const unsigned valid = cube[q < 0 ? i : (size_t)q] >> 7;
      around |= (q < 0 ? 0u : valid) << e;
    }
    for (unsigned d = 1; d < 8; d++) {
      const long long q = tm_at(g, c, d, 1);
      // the cubes that contain the edge (q, d): origins q - e with e inside the zero bits of d
      unsigned near = 0;
      for (unsigned e = 0; e < 8; e++)
        if (!(e & d)) near |= (around >> e) & 1u;
      const unsigned in1 = (state[q < 0 ? i : (size_t)q] >> 1) & 1u;
      if (q >= 0 && near && in0 != in1) mask |= 1u << d;
    }
    vmask[i] = (uint8_t)mask;
  }
  const uint32_t incl = block_scan_incl((uint32_t)__popc(mask), wtot);      // (every lane is here)
  if (threadIdx.x == TM_TB - 1) vcounts[blockIdx.x] = incl;
}

template <class L>
void tm_launch_plan(const L& g, const void* tsdf_w, float min_weight, void* work, uint64_t* counters, hipStream_t s) {
  const TmWork w = tm_work(work, g.n);
  const unsigned nb = (unsigned)tm_nb(g.n);      // <= 2^30 / 256
  launch_tm_state(g.n, tsdf_w, min_weight, w, s);
  hipLaunchKernelGGL(tm_cube_kernel<L>, dim3(nb), dim3(TM_TB), 0, s, g, w.state, w.cube, w.tcounts);
  hipLaunchKernelGGL(tm_edge_kernel<L>, dim3(nb), dim3(TM_TB), 0, s, g, w.state, w.cube, w.vmask, w.vcounts);
  launch_tm_scan_base(g.n, w, counters, s);
}

// ---- the emit's two kernels --------------------------------------------------------------------------------------------------------
template <class L>
__global__ void __launch_bounds__(TM_TB)
tm_vertex_kernel(L g, TmEmit e, const float2* __restrict__ tsdf_w, const float4* __restrict__ rgb_w, const uint8_t* __restrict__ vmask,
                 const uint32_t* __restrict__ vbase, const unsigned long long* __restrict__ hdr, uint4* __restrict__ rows, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * TM_TB + threadIdx.x;
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
  const typename L::Cell c = g.cell(i);
  int q[3];
  g.lattice_index(c, q);
  const double T0 = (double)tsdf_w[i].x;
  const float4 c0 = rgb_w[i];
  unsigned long long r = vbase[i];
  for (unsigned d = 1; d < 8; d++) {
    if (!((mask >> d) & 1u)) continue;
    const long long j = tm_at(g, c, d, 1);      // (there: the plan found the edge through the same lattice)
    if (r < e.vcap && j >= 0) {
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

template <class L>
__global__ void __launch_bounds__(TM_TB)
tm_triangle_kernel(L g, TmEmit e, const uint8_t* __restrict__ state, const uint8_t* __restrict__ cube, const uint8_t* __restrict__ vmask,
                   const uint32_t* __restrict__ vbase, const uint32_t* __restrict__ tbase, int* __restrict__ tris, unsigned long long* __restrict__ counters) {
  const size_t i = (size_t)blockIdx.x * TM_TB + threadIdx.x;
  uint32_t written = 0, dropped = 0;
  if (i < g.n && (cube[i] & 0x7fu)) {      // (a cube with triangles is valid: its 8 corners are there)
    const typename L::Cell c = g.cell(i);
    unsigned inside;
    if (!tm_cube_corners(g, state, c, inside)) {      // (valid in the plan: only where the lattice is not the plan's, and then the cube's triangles are dropped, not read out of bounds)
      dropped = cube[i] & 0x7fu;
      inside = 0;
    }
    unsigned long long r = tbase[i];
    for (int k = 0; k < 6; k++) {
      const uint32_t cs = TM_CASES[tm_tet_mask(inside, k)];
      const unsigned corner[4] = {0u, TM_MID1[k], TM_MID2[k], 7u};
      for (uint32_t s = 0; s < (cs & 3u); s++) {
        uint32_t idx[3];
        for (int a = 0; a < 3; a++) {
          const unsigned edge = (cs >> (2 + 9 * s + 3 * a)) & 7u;
          const unsigned lo = corner[TM_EDGE_LO[edge]], hi = corner[TM_EDGE_HI[edge]];
          const long long smp = tm_at(g, c, lo, 1);
          // (there, as the cube's corners were; a lattice that says otherwise has the triangle dropped)
          idx[a] = smp < 0 ? 0xffffffffu : vbase[smp] + (uint32_t)__popc((unsigned)vmask[smp] & ((1u << (hi ^ lo)) - 1u));
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

template <class L>
void tm_launch_emit(const L& g, const void* tsdf_w, const void* rgb_w, const double* o, double voxel, const void* work, void* rows, uint64_t vcap, void* tris,
                    uint64_t tcap, uint64_t* counters, hipStream_t s) {
  const TmWork w = tm_work((void*)work, g.n);
  TmEmit e;
  e.o[0] = o[0]; e.o[1] = o[1]; e.o[2] = o[2]; e.voxel = voxel; e.vcap = vcap; e.tcap = tcap;
  const unsigned nb = (unsigned)tm_nb(g.n);
  hipLaunchKernelGGL(tm_vertex_kernel<L>, dim3(nb), dim3(TM_TB), 0, s, g, e, (const float2*)tsdf_w, (const float4*)rgb_w, w.vmask, w.vbase, w.hdr, (uint4*)rows,
                     (unsigned long long*)counters);
  hipLaunchKernelGGL(tm_triangle_kernel<L>, dim3(nb), dim3(TM_TB), 0, s, g, e, w.state, w.cube, w.vmask, w.vbase, w.tbase, (int*)tris, (unsigned long long*)counters);
}

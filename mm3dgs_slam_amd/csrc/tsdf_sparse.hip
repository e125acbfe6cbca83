// The mesh export's volume as voxel blocks (mm3dgs_tsdf_blocks_*; host statement: mesh.reserve_host / mesh.HostSparseTsdfVolume): storage
// in blocks of 8 x 8 x 8 samples, only where a depth pixel puts the truncation band.  Sample (i, j, k) in Z^3 sits at anchor + voxel (i, j,
// k); block b = floor(index / 8) per axis, |b| < 2^20; key = (bz + 2^20) << 42 | (by + 2^20) << 21 | (bx + 2^20), so ascending keys are
// blocks in z-major raster order; all ones = empty.  The export reserves all its views, freezes the block set (list, sort, index), then
// integrates all views; a sample outside the frozen set is never touched.
//
//   blk_reserve_kernel     one launch per view, one lane per pixel.  A valid pixel is lifted to its world point P (view_lift);
//                          with ax = (|u - cx| trunc + (d + trunc) / 2) / |fx|, ay likewise and R = sqrt(ax^2 + ay^2 + trunc^2) every sample
//                          the integration can update through this pixel with |sdf| <= trunc lies within R of P (|z - d| <= trunc, the
//                          nearest-pixel projection at most half a pixel off, the ray's slope).  Per axis the blocks from
//                          floor(floor((P - R - anchor) / voxel) / 8) to floor(ceil((P + R - anchor) / voxel) / 8) are claimed: an
//                          agent-scope load of the slot, a 64-bit atomicCAS only where it read empty, linear probing, at most
//                          BLK_MAX_PROBE slots (pc_claim_kernel's scheme).  A key goes from empty to its value once.  A box beyond
//                          |b| < 2^20 or wider than BLK_MAX_BOX blocks on an axis skips the pixel and is counted.  Counters: one integer
//                          add per workgroup and counter, one per newly claimed block.
//   blk_list_*             the table's keys by count, scan_block_counts and block_rank scatter: slot order, the caller sorts.
//   blk_index_*            sorted keys -> each key's rank in its slot, and neighbours int32 [n][27] (-1: none) by lookup; keys that are
//                          not strictly ascending or not in the table set counters[6] and nothing is indexed.
//   blk_integrate_kernel   one launch per view, one workgroup of 256 per block, a wave of 64 lanes = one 8 x 8 z slice, two slices per wave;
//                          the per-sample body is the dense kernel's (tsdf_sample.h).  A block whose bounding sphere is behind the camera
//                          or projects outside the image (conservatively: a pixel of slack, the sphere 1e-6 larger) leaves early.
//   marching tetrahedra    tsdf_march.h's cube, edge, vertex and triangle kernels, instantiated over the block lattice (BlkGrid: n 512
//                          samples with block-local indexing and the neighbour table at the faces; a missing neighbour is unknown);
//                          state, scan and base are tsdf.hip's own kernels.
// Every loop is bounded: probes, a pixel's block box (8^3), the 27 neighbours.  No atomic decides a position or an index.
#include <math.h>
#include "tsdf_sample.h"
#include "tsdf_march.h"

#define SB 256
#define BLK_MAX_PROBE 128
#define BLK_MAX_BOX 8                       // blocks a pixel's box may span per axis (trunc <= 16 voxel: a box of at most 2 R + 2 samples)
#define BLK_EMPTY 0xffffffffffffffffull
#define BLK_BIAS 1048576ll                  // 2^20
#define BLK_NO_RANK 0xffffffffu

// table = [uint64 key per slot][uint32 rank per slot][uint32 count per 256 slots]; slots = the power of two >= 2 max_blocks
struct BlkTable { unsigned long long* keys; uint32_t* rank; uint32_t* counts; uint64_t slots; int shift; };
static BlkTable blk_table(void* base, uint64_t max_blocks, size_t* bytes = nullptr) {
  BlkTable t;
  t.slots = 2;
  t.shift = 63;
  while (t.slots < 2 * max_blocks) { t.slots <<= 1; t.shift--; }
  Carve c = {(uintptr_t)base};
  t.keys = c.take<unsigned long long>(t.slots);
  t.rank = c.take<uint32_t>(t.slots);
  t.counts = c.take<uint32_t>((t.slots + SB - 1) / SB);
  if (bytes) *bytes = c.at;
  return t;
}
size_t tsdf_blocks_table_bytes(uint64_t max_blocks, uint64_t* slots) {
  size_t b;
  const BlkTable t = blk_table(nullptr, max_blocks, &b);
  if (slots) *slots = t.slots;
  return b;
}

__device__ __forceinline__ uint64_t blk_hash(uint64_t key, int shift) { return (key * 0x9E3779B97F4A7C15ull) >> shift; }
__device__ __forceinline__ uint64_t blk_key(long long bx, long long by, long long bz) {
  return ((uint64_t)(bz + BLK_BIAS) << 42) | ((uint64_t)(by + BLK_BIAS) << 21) | (uint64_t)(bx + BLK_BIAS);
}
__device__ __forceinline__ void blk_coords(uint64_t key, int& bx, int& by, int& bz) {
  bx = (int)((long long)(key & 0x1fffffull) - BLK_BIAS);
  by = (int)((long long)((key >> 21) & 0x1fffffull) - BLK_BIAS);
  bz = (int)((long long)((key >> 42) & 0x1fffffull) - BLK_BIAS);
}
__device__ __forceinline__ int blk_probes(const BlkTable& t) { return t.slots < (uint64_t)BLK_MAX_PROBE ? (int)t.slots : BLK_MAX_PROBE; }

// the slot that holds `key`, or -1 (plain loads: behind the kernel boundary of the last reservation)
__device__ __forceinline__ long long blk_find(const BlkTable& t, uint64_t key) {
  const uint64_t mask = t.slots - 1, h = blk_hash(key, t.shift);
  const int probes = blk_probes(t);
  for (int p = 0; p < probes; p++) {
    const uint64_t s = (h + (uint64_t)p) & mask;
    const unsigned long long k = t.keys[s];
    if (k == key) return (long long)s;
    if (k == BLK_EMPTY) return -1;
  }
  return -1;
}

// ---- reset ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB) blk_reset_kernel(BlkTable t, unsigned long long* __restrict__ counters) {
  const size_t step = (size_t)gridDim.x * SB;
  for (size_t i = (size_t)blockIdx.x * SB + threadIdx.x; i < t.slots; i += step) {
    t.keys[i] = BLK_EMPTY;
    t.rank[i] = BLK_NO_RANK;
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) counters[threadIdx.x] = 0ull;
}

void launch_tsdf_blocks_reset(void* table, uint64_t max_blocks, uint64_t* counters, hipStream_t s) {
  const BlkTable t = blk_table(table, max_blocks);
  size_t nb = (t.slots + SB - 1) / SB;
  nb = nb > 4096 ? 4096 : nb;
  hipLaunchKernelGGL(blk_reset_kernel, dim3((unsigned)nb), dim3(SB), 0, s, t, (unsigned long long*)counters);
}

// ---- reservation -------------------------------------------------------------------------------------------------------------------
// counters: [0] views, [1] valid pixels, [2] (pixel, block) pairs, [3] distinct blocks, [4] dropped (a pair whose probe window held no
// room, or a block claimed beyond max_blocks), [5] pixels out of range, [6] the index call's errors, [7] 0
__global__ void __launch_bounds__(SB)
blk_reserve_kernel(TsdfView v, TsdfBlockClip clip, BlkTable t, unsigned long long max_blocks, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  __shared__ Rigid g;
  __shared__ uint32_t wsum[4][SB / 64];
  const int n = v.H * v.W;
  const int i = blockIdx.x * SB + threadIdx.x;
  view_rigid_shared(v.pose, g);
  uint32_t valid = 0, pairs = 0, dropped = 0, oor = 0;
  float df;
  if (i < n && view_pixel_valid(v.depth, v.sil, v.sil_min, v.depth_max, (size_t)i, df)) {
    valid = 1;
    const double z = (double)df, u = (double)(i % v.W), w = (double)(i / v.W);
    double P[3];
    view_lift(v, g, u, w, z, P);
    const double ax = (fabs(u - v.cx) * v.trunc + 0.5 * (z + v.trunc)) / fabs(v.fx);
    const double ay = (fabs(w - v.cy) * v.trunc + 0.5 * (z + v.trunc)) / fabs(v.fy);
    const double R = sqrt(ax * ax + ay * ay + v.trunc * v.trunc);
    int lo[3], hi[3];
    bool in = true;
    for (int a = 0; a < 3; a++) {
      const double bl = floor(floor((P[a] - R - v.o[a]) / v.voxel) / 8.0), bh = floor(ceil((P[a] + R - v.o[a]) / v.voxel) / 8.0);
      if (!(fabs(bl) < (double)BLK_BIAS && fabs(bh) < (double)BLK_BIAS && bh - bl < (double)BLK_MAX_BOX)) { in = false; break; }      // (a NaN fails)
      lo[a] = (int)bl;
      hi[a] = (int)bh;
      lo[a] = lo[a] > clip.lo[a] ? lo[a] : clip.lo[a];
      hi[a] = hi[a] < clip.hi[a] ? hi[a] : clip.hi[a];
    }
    if (!in) {
      oor = 1;
    } else {
      const uint64_t mask = t.slots - 1;
      const int probes = blk_probes(t);
      for (int dz = 0; dz < BLK_MAX_BOX && lo[2] + dz <= hi[2]; dz++)
        for (int dy = 0; dy < BLK_MAX_BOX && lo[1] + dy <= hi[1]; dy++)
          for (int dx = 0; dx < BLK_MAX_BOX && lo[0] + dx <= hi[0]; dx++) {
            const uint64_t key = blk_key(lo[0] + dx, lo[1] + dy, lo[2] + dz), h = blk_hash(key, t.shift);
            pairs++;
            bool done = false;
            for (int p = 0; p < probes; p++) {
              unsigned long long* slot = t.keys + ((h + (uint64_t)p) & mask);
              // a key goes from empty to its value once: what an agent-scope load shows as another block's key stays that key
              unsigned long long k = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if (k == BLK_EMPTY) {
                k = atomicCAS(slot, BLK_EMPTY, (unsigned long long)key);
                if (k == BLK_EMPTY) {      // this lane made the block: it counts it, and beyond max_blocks it counts it as dropped
                  if (atomicAdd(counters + 3, 1ull) >= max_blocks) atomicAdd(counters + 4, 1ull);
                  done = true;
                  break;
                }
              }
              if (k == key) { done = true; break; }
            }
            if (!done) dropped++;
          }
    }
  }
  const uint32_t nn[4] = {valid, pairs, dropped, oor};
  const uint32_t s = block_sums_u32(nn, wsum);      // (every lane is here)
  if (s) {
    if (threadIdx.x == 0) atomicAdd(counters + 1, (unsigned long long)s);
    if (threadIdx.x == 1) atomicAdd(counters + 2, (unsigned long long)s);
    if (threadIdx.x == 2) atomicAdd(counters + 4, (unsigned long long)s);
    if (threadIdx.x == 3) atomicAdd(counters + 5, (unsigned long long)s);
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(counters, 1ull);
}

void launch_tsdf_blocks_reserve(const TsdfView& v, const TsdfBlockClip& clip, void* table, uint64_t max_blocks, uint64_t* counters, hipStream_t s) {
  const size_t n = (size_t)v.H * (size_t)v.W;
  hipLaunchKernelGGL(blk_reserve_kernel, dim3((unsigned)((n + SB - 1) / SB)), dim3(SB), 0, s, v, clip, blk_table(table, max_blocks), (unsigned long long)max_blocks,
                     (unsigned long long*)counters);
}

// ---- list ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB) blk_list_count_kernel(BlkTable t) {
  __shared__ uint32_t wsum[1][SB / 64];
  const size_t i = (size_t)blockIdx.x * SB + threadIdx.x;
  const bool is[1] = {i < t.slots && t.keys[i] != BLK_EMPTY};
  const uint32_t c = block_flag_counts(is, wsum);
  if (threadIdx.x == 0) t.counts[blockIdx.x] = c;
}

__global__ void __launch_bounds__(1024) blk_list_scan_kernel(int nb, uint32_t* __restrict__ counts) {
  __shared__ uint32_t total;
  scan_block_counts(nb, counts, &total);
}

__global__ void __launch_bounds__(SB) blk_list_scatter_kernel(BlkTable t, unsigned long long* __restrict__ keys, unsigned long long cap) {
  __shared__ uint32_t wsum[SB / 64];
  const size_t i = (size_t)blockIdx.x * SB + threadIdx.x;
  const unsigned long long k = i < t.slots ? t.keys[i] : BLK_EMPTY;
  const uint32_t r = block_rank(k != BLK_EMPTY, t.counts[blockIdx.x], wsum);
  if (k != BLK_EMPTY && (unsigned long long)r < cap) keys[r] = k;
}

void launch_tsdf_blocks_list(void* table, uint64_t max_blocks, uint64_t* keys, uint64_t cap, hipStream_t s) {
  const BlkTable t = blk_table(table, max_blocks);
  const unsigned nb = (unsigned)((t.slots + SB - 1) / SB);      // <= 2^22 / 256
  hipLaunchKernelGGL(blk_list_count_kernel, dim3(nb), dim3(SB), 0, s, t);
  hipLaunchKernelGGL(blk_list_scan_kernel, dim3(1), dim3(1024), 0, s, (int)nb, t.counts);
  hipLaunchKernelGGL(blk_list_scatter_kernel, dim3(nb), dim3(SB), 0, s, t, (unsigned long long*)keys, (unsigned long long)cap);
}

// ---- index ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB) blk_index_clear_kernel(BlkTable t, unsigned long long* __restrict__ counters) {
  const size_t i = (size_t)blockIdx.x * SB + threadIdx.x;
  if (i < t.slots) t.rank[i] = BLK_NO_RANK;
  if (i == 0) counters[6] = 0ull;
}

__global__ void __launch_bounds__(SB)
blk_index_check_kernel(BlkTable t, const unsigned long long* __restrict__ keys, unsigned long long n, unsigned long long* __restrict__ counters) {
  __shared__ uint32_t wsum[1][SB / 64];
  const size_t r = (size_t)blockIdx.x * SB + threadIdx.x;
  bool bad = false;
  if (r < n) {
    const unsigned long long k = keys[r];
    bad = k == BLK_EMPTY || (r > 0 && keys[r - 1] >= k) || blk_find(t, k) < 0;
  }
  const bool is[1] = {bad};
  const uint32_t c = block_flag_counts(is, wsum);
  if (threadIdx.x == 0 && c) atomicAdd(counters + 6, (unsigned long long)c);
}

__global__ void __launch_bounds__(SB)
blk_index_rank_kernel(BlkTable t, const unsigned long long* __restrict__ keys, unsigned long long n, const unsigned long long* __restrict__ counters) {
  const size_t r = (size_t)blockIdx.x * SB + threadIdx.x;
  if (r >= n || counters[6]) return;      // (the check kernel ended before this one began)
  const long long s = blk_find(t, keys[r]);
  if (s >= 0) t.rank[s] = (uint32_t)r;
}

__global__ void __launch_bounds__(SB)
blk_index_neighbours_kernel(BlkTable t, const unsigned long long* __restrict__ keys, unsigned long long n, int* __restrict__ neighbours,
                            const unsigned long long* __restrict__ counters) {
  const size_t i = (size_t)blockIdx.x * SB + threadIdx.x;
  if (i >= n * 27ull || counters[6]) return;
  const size_t r = i / 27;
  const int j = (int)(i % 27);
  int bx, by, bz;
  blk_coords(keys[r], bx, by, bz);
  bx += j % 3 - 1; by += (j / 3) % 3 - 1; bz += j / 9 - 1;
  int out = -1;
  if (abs(bx) < (int)BLK_BIAS && abs(by) < (int)BLK_BIAS && abs(bz) < (int)BLK_BIAS) {
    const long long s = blk_find(t, blk_key(bx, by, bz));
    if (s >= 0) {
      const uint32_t rk = t.rank[s];
      if ((unsigned long long)rk < n) out = (int)rk;
    }
  }
  neighbours[i] = out;
}

void launch_tsdf_blocks_index(void* table, uint64_t max_blocks, const uint64_t* keys, uint64_t n, int* neighbours, uint64_t* counters, hipStream_t s) {
  const BlkTable t = blk_table(table, max_blocks);
  const unsigned nbn = (unsigned)((n + SB - 1) / SB);
  hipLaunchKernelGGL(blk_index_clear_kernel, dim3((unsigned)((t.slots + SB - 1) / SB)), dim3(SB), 0, s, t, (unsigned long long*)counters);
  hipLaunchKernelGGL(blk_index_check_kernel, dim3(nbn), dim3(SB), 0, s, t, (const unsigned long long*)keys, (unsigned long long)n, (unsigned long long*)counters);
  hipLaunchKernelGGL(blk_index_rank_kernel, dim3(nbn), dim3(SB), 0, s, t, (const unsigned long long*)keys, (unsigned long long)n, (const unsigned long long*)counters);
  hipLaunchKernelGGL(blk_index_neighbours_kernel, dim3((unsigned)((n * 27 + SB - 1) / SB)), dim3(SB), 0, s, t, (const unsigned long long*)keys, (unsigned long long)n,
                     neighbours, (const unsigned long long*)counters);
}

// ---- integration -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB)
blk_integrate_kernel(TsdfView v, const unsigned long long* __restrict__ keys, float2* __restrict__ tsdf_w, float4* __restrict__ rgb_w,
                     unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  __shared__ Rigid g;
  __shared__ uint32_t wsum[2][SB / 64];
  const unsigned r = blockIdx.x;
  view_rigid_shared(v.pose, g);
  if (threadIdx.x == 0 && r == 0) atomicAdd(counters, 1ull);
  int b[3];
  blk_coords(keys[r], b[0], b[1], b[2]);
  // the block's bounding sphere in the camera frame: the same for every lane, so the whole workgroup leaves or stays
  const double rad = v.voxel * 3.5 * 1.7320508075688773 * (1.0 + 1e-6);
  const double m0 = v.o[0] + v.voxel * ((double)(8 * b[0]) + 3.5), m1 = v.o[1] + v.voxel * ((double)(8 * b[1]) + 3.5), m2 = v.o[2] + v.voxel * ((double)(8 * b[2]) + 3.5);
  double xc, yc, zc;
  view_to_camera(g, m0, m1, m2, xc, yc, zc);
  if (zc + rad <= 0.0) return;      // every sample has z <= 0
  if (zc - rad > 0.0 && v.fx > 0.0 && v.fy > 0.0) {      // (a bound on the sphere's pixels with slack, not view_pixel_index's nearest pixel)
    const double zn = zc - rad, zf = zc + rad;
    // x / z over the sphere lies in [(xc - rad) / (its sign < 0 ? zn : zf), (xc + rad) / (its sign > 0 ? zn : zf)]
    const double uhi = v.fx * ((xc + rad) / (xc + rad >= 0.0 ? zn : zf)) + v.cx + 0.5, ulo = v.fx * ((xc - rad) / (xc - rad <= 0.0 ? zn : zf)) + v.cx + 0.5;
    const double vhi = v.fy * ((yc + rad) / (yc + rad >= 0.0 ? zn : zf)) + v.cy + 0.5, vlo = v.fy * ((yc - rad) / (yc - rad <= 0.0 ? zn : zf)) + v.cy + 0.5;
    if (uhi < -1.0 || ulo > (double)v.W + 1.0 || vhi < -1.0 || vlo > (double)v.H + 1.0) return;      // every sample's pixel is outside the image
  }
  const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
  const int i = 8 * b[0] + (lane & 7), j = 8 * b[1] + (lane >> 3);
  const size_t hw = (size_t)v.H * (size_t)v.W;
  const double pw0 = v.o[0] + v.voxel * (double)i, pw1 = v.o[1] + v.voxel * (double)j;
  uint32_t nupd = 0, ncup = 0;
  for (int kk = wv; kk < 8; kk += SB / 64) {
    const double pw2 = v.o[2] + v.voxel * (double)(8 * b[2] + kk);
    const size_t q = (size_t)r * 512 + (size_t)kk * 64 + (size_t)lane;
    tsdf_sample_update(v, g, hw, pw0, pw1, pw2, tsdf_w + q, rgb_w + q, nupd, ncup);
  }
  const uint32_t nn[2] = {nupd, ncup};
  const uint32_t t = block_sums_u32(nn, wsum);      // (every lane of a workgroup that stayed is here)
  if (threadIdx.x < 2 && t) atomicAdd(counters + 1 + threadIdx.x, (unsigned long long)t);
}

void launch_tsdf_blocks_integrate(const TsdfView& v, const uint64_t* keys, uint64_t n, void* tsdf_w, void* rgb_w, uint64_t* counters, hipStream_t s) {
  hipLaunchKernelGGL(blk_integrate_kernel, dim3((unsigned)n), dim3(SB), 0, s, v, (const unsigned long long*)keys, (float2*)tsdf_w, (float4*)rgb_w,
                     (unsigned long long*)counters);
}

// ---- marching tetrahedra -----------------------------------------------------------------------------------------------------------
// the block lattice: sample (x, y, z) of block r at pool index 512 r + 64 z + 8 y + x; a step across a face goes through the 27-neighbour
// table, and there is no sample where the block that would hold it is not in the set
struct BlkGrid {
  struct Cell { unsigned r; int x, y, z; };
  unsigned blocks;
  size_t n;      // 512 blocks: every workgroup of 256 is full
  const int* nbr;
  const unsigned long long* keys;      // (the emit's: only lattice_index reads them)
  __device__ __forceinline__ Cell cell(size_t i) const { return {(unsigned)(i >> 9), (int)(i & 7), (int)((i >> 3) & 7), (int)((i >> 6) & 7)}; }
  __device__ __forceinline__ long long at(const Cell& c, int dx, int dy, int dz) const {
    const int x = c.x + dx, y = c.y + dy, z = c.z + dz;      // each in -1 .. 8
    const int j = ((z + 8) >> 3) * 9 + ((y + 8) >> 3) * 3 + ((x + 8) >> 3);
    unsigned rr = c.r;
    if (j != 13) {
      rr = (unsigned)nbr[(size_t)c.r * 27 + j];
      if (rr >= blocks) return -1;      // (-1, or an index the caller's table should not hold)
    }
    return (long long)rr * 512 + (z & 7) * 64 + (y & 7) * 8 + (x & 7);
  }
  __device__ __forceinline__ void lattice_index(const Cell& c, int q[3]) const {
    int b[3];
    blk_coords(keys[c.r], b[0], b[1], b[2]);
    q[0] = 8 * b[0] + c.x; q[1] = 8 * b[1] + c.y; q[2] = 8 * b[2] + c.z;
  }
  __device__ __forceinline__ bool cube(const Cell& c, long long q[8]) const {
    bool all = true;
    for (unsigned e = 0; e < 8; e++) {
      q[e] = at(c, (int)(e & 1u), (int)((e >> 1) & 1u), (int)((e >> 2) & 1u));
      all = all && q[e] >= 0;
    }
    return all;
  }
};
static BlkGrid blk_grid(uint64_t n, const int* neighbours, const uint64_t* keys) {
  return {(unsigned)n, (size_t)n * 512, neighbours, (const unsigned long long*)keys};
}

size_t tsdf_blocks_mesh_work_bytes(uint64_t n) { size_t b; tm_work(nullptr, (size_t)n * 512, &b); return b; }

void launch_tsdf_blocks_mesh_plan(uint64_t n, const int* neighbours, const void* tsdf_w, float min_weight, void* work, uint64_t* counters, hipStream_t s) {
  tm_launch_plan(blk_grid(n, neighbours, nullptr), tsdf_w, min_weight, work, counters, s);
}

void launch_tsdf_blocks_mesh_emit(uint64_t n, const uint64_t* keys, const int* neighbours, const void* tsdf_w, const void* rgb_w, const double* anchor, double voxel,
                                  const void* work, void* rows, uint64_t vcap, void* tris, uint64_t tcap, uint64_t* counters, hipStream_t s) {
  tm_launch_emit(blk_grid(n, neighbours, keys), tsdf_w, rgb_w, anchor, voxel, work, rows, vcap, tris, tcap, counters, s);
}

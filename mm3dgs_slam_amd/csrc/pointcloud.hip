// Fused coloured point cloud of a finished run (mm3dgs_pointcloud_add_view; reference scripts/visualizer.py:69-112 rgbd2pcd, the lift of
// every pixel of an RGB-D image to a world point; host statement: pointcloud.backproject_host / voxel_select_host).  One call adds one
// view to a growing buffer of 16-byte rows {float x, y, z; uint32 rgba}; with a voxel size only the first point that ever reached a voxel
// (in stream order: view, then raster) is kept, so the rows of a view are final when its call ends and the file is the same on every run.
//
// Kernels of one view, in stream order (256-lane workgroups over the H W pixels unless noted):
//   pc_claim_kernel    (voxel > 0) every valid in-range pixel probes the caller's open-addressing table {uint64 key, uint64 ticket} from a
//                      multiplicative hash of its voxel key, linearly, at most PC_MAX_PROBE slots: the first slot whose key is its own or
//                      empty is taken (64-bit atomicCAS on the key), then atomicMin of its ticket (view << 32 | pixel).  Keys only ever go
//                      from empty to a value, so a key read as non-empty is final; every loop is bounded: a full table ends as a count.
//   pc_select_kernel   after the kernel boundary (the only hand-off: no flag, no fence) every pixel finds its slot again with plain loads;
//                      it represents its voxel iff the ticket there is its own.  Writes one flag byte per pixel and four counts per
//                      workgroup (representatives, valid, out of range, probe failures), plain stores.  voxel == 0: representative = valid.
//   pc_scan_kernel     one workgroup of 1024: scan_block_counts over the representatives, the three other sums, the view's base = the
//                      running row count, and the counters -- no atomic touches a counter or decides a position.
//   pc_scatter_kernel  representatives in raster order from the base by ballot rank; rows at or beyond cap are not written.
// A position is evaluated in double from the float32 inputs and rounded once to float32; the three kernels that need it call one function
// compiled without contraction, so they agree on the float32 value and hence on the key.
#include <math.h>
#include "block_ops.h"
#include "fused_api.h"
#include "view_pixel.h"      // Rigid / rigid_from_pose, view_lift, view_pixel_valid, pc_quant

#define PB 256
#define PC_MAX_PROBE 128                 // slots a point may inspect; the table is sized for a load of at most 1/2
#define PC_EMPTY 0xffffffffffffffffull
#define PC_CELL_LIMIT 1048576.0          // 2^20 cells on either side of the origin per axis

// work = [256 B header: uint64 base of this view][flag byte per pixel][4 x per-workgroup counts: representatives, valid, out of range, probe failures]
struct PcWork { unsigned long long* hdr; uint8_t* flag; uint32_t* counts[4]; };
static size_t pc_nb(size_t n) { return (n + PB - 1) / PB; }
static PcWork pc_work(void* base, size_t n, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  PcWork w;
  w.hdr = c.take<unsigned long long>(1);
  w.flag = c.take<uint8_t>(n);
  for (int k = 0; k < 4; k++) w.counts[k] = c.take<uint32_t>(pc_nb(n));
  if (bytes) *bytes = c.at;
  return w;
}
size_t pointcloud_work_bytes(int H, int W) { size_t b; pc_work(nullptr, (size_t)H * (size_t)W, &b); return b; }

struct PcPoint { float x, y, z; };

// the world point of pixel i at depth z (view_lift), rounded once to float32
__device__ __forceinline__ PcPoint pc_backproject(const PointCloudView& v, const Rigid& g, int i, float zf) {
  double P[3];
  view_lift(v, g, (double)(i % v.W), (double)(i / v.W), (double)zf, P);
  return {(float)P[0], (float)P[1], (float)P[2]};
}

// the pixel test of view_pixel.h on this view's images
__device__ __forceinline__ bool pc_valid(const PointCloudView& v, int i, float& z) {
  return view_pixel_valid(v.depth, v.sil, v.sil_min, v.depth_max, (size_t)i, z);
}

// voxel key of a stored position; false: some |cell| >= 2^20 (or not a number)
__device__ __forceinline__ bool pc_key(const PcPoint& p, double voxel, uint64_t& key) {
  const double c[3] = {floor((double)p.x / voxel), floor((double)p.y / voxel), floor((double)p.z / voxel)};
  if (!(fabs(c[0]) < PC_CELL_LIMIT && fabs(c[1]) < PC_CELL_LIMIT && fabs(c[2]) < PC_CELL_LIMIT)) return false;
  key = ((uint64_t)((long long)c[0] + 1048576ll) << 42) | ((uint64_t)((long long)c[1] + 1048576ll) << 21) | (uint64_t)((long long)c[2] + 1048576ll);
  return true;
}

__device__ __forceinline__ uint64_t pc_hash(uint64_t key, int shift) { return (key * 0x9E3779B97F4A7C15ull) >> shift; }

__global__ void __launch_bounds__(PB) pc_claim_kernel(PointCloudView v) {
  const int n = v.H * v.W;
  const int i = blockIdx.x * PB + threadIdx.x;
  if (i >= n) return;
  float z;
  if (!pc_valid(v, i, z)) return;
  const Rigid g = rigid_from_pose(v.pose);
  uint64_t key;
  if (!pc_key(pc_backproject(v, g, i, z), v.voxel, key)) return;
  const uint64_t mask = v.slots - 1, ticket = ((uint64_t)v.view << 32) | (uint64_t)(uint32_t)i;
  const uint64_t h = pc_hash(key, v.hash_shift);
  const int probes = v.slots < (uint64_t)PC_MAX_PROBE ? (int)v.slots : PC_MAX_PROBE;
  for (int p = 0; p < probes; p++) {
    unsigned long long* slot = v.table + 2 * ((h + (uint64_t)p) & mask);
    // a key goes from empty to its value once: what an agent-scope load shows as another voxel's key stays that key
    unsigned long long k = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == PC_EMPTY) k = atomicCAS(slot, PC_EMPTY, (unsigned long long)key);
    if (k == PC_EMPTY || k == key) {
      atomicMin(slot + 1, (unsigned long long)ticket);
      return;
    }
  }
}

__global__ void __launch_bounds__(PB)
pc_select_kernel(PointCloudView v, uint8_t* __restrict__ flag, uint32_t* __restrict__ counts, size_t stride) {
  __shared__ uint32_t wsum[4][PB / 64];
  const int n = v.H * v.W;
  const int i = blockIdx.x * PB + threadIdx.x;
  float z;
  const bool valid = i < n && pc_valid(v, i, z);
  bool rep = valid, oor = false, fail = false;
  if (valid && v.table) {
    const Rigid g = rigid_from_pose(v.pose);
    uint64_t key;
    rep = false;
    if (!pc_key(pc_backproject(v, g, i, z), v.voxel, key)) {
      oor = true;
    } else {
      const uint64_t mask = v.slots - 1, ticket = ((uint64_t)v.view << 32) | (uint64_t)(uint32_t)i;
      const uint64_t h = pc_hash(key, v.hash_shift);
      const int probes = v.slots < (uint64_t)PC_MAX_PROBE ? (int)v.slots : PC_MAX_PROBE;
      fail = true;
      for (int p = 0; p < probes; p++) {
        const unsigned long long* slot = v.table + 2 * ((h + (uint64_t)p) & mask);
        const unsigned long long k = slot[0];
        if (k == key) { rep = slot[1] == ticket; fail = false; break; }
        if (k == PC_EMPTY) break;      // (cannot happen after a claim that found a slot; a failed claim saw no empty slot in its window)
      }
    }
  }
  if (i < n) flag[i] = rep ? 1 : 0;
  const bool is[4] = {rep, valid, oor, fail};
  const uint32_t t = block_flag_counts(is, wsum);
  if (threadIdx.x < 4) counts[threadIdx.x * stride + blockIdx.x] = t;
}

__global__ void __launch_bounds__(1024)
pc_scan_kernel(int nb, size_t stride, uint32_t* __restrict__ counts, unsigned long long cap, unsigned long long* __restrict__ counters,
               unsigned long long* __restrict__ hdr) {
  __shared__ uint32_t sh[16];
  __shared__ uint32_t total;
  scan_block_counts(nb, counts, &total);
  const uint32_t valid = block_array_sum(nb, counts + stride, sh);
  const uint32_t oor = block_array_sum(nb, counts + 2 * stride, sh);
  const uint32_t fail = block_array_sum(nb, counts + 3 * stride, sh);
  if (threadIdx.x == 0) {      // (lane 0 wrote `total` itself)
    const unsigned long long reps = total, base = counters[0];
    const unsigned long long room = base < cap ? cap - base : 0ull;
    const unsigned long long written = reps < room ? reps : room;
    hdr[0] = base;
    counters[0] = base + written;
    counters[1] += valid;
    counters[2] += (unsigned long long)valid - oor - fail - reps;
    counters[3] += oor;
    counters[4] += fail;
    counters[5] += reps - written;
    counters[6] += 1ull;
  }
}

__global__ void __launch_bounds__(PB)
pc_scatter_kernel(PointCloudView v, const uint8_t* __restrict__ flag, const uint32_t* __restrict__ block_pre, const unsigned long long* __restrict__ hdr,
                  unsigned long long cap, uint4* __restrict__ rows) {
  __shared__ uint32_t wsum[PB / 64];
  const int n = v.H * v.W;
  const int i = blockIdx.x * PB + threadIdx.x;
  const bool rep = i < n && flag[i] != 0;
  const unsigned long long r = hdr[0] + (unsigned long long)block_rank(rep, block_pre[blockIdx.x], wsum);
  if (!rep || r >= cap) return;
  const Rigid g = rigid_from_pose(v.pose);
  const PcPoint p = pc_backproject(v, g, i, v.depth[i]);
  const uint32_t rgba = pc_quant(v.color[i]) | (pc_quant(v.color[(size_t)n + i]) << 8) | (pc_quant(v.color[2 * (size_t)n + i]) << 16) | 0xff000000u;
  rows[r] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), rgba);      // one 16-byte store
}

// table words (2 per slot) to all ones, the eight counters to zero
__global__ void __launch_bounds__(PB) pc_reset_kernel(unsigned long long* __restrict__ table, size_t words, unsigned long long* __restrict__ counters) {
  const size_t step = (size_t)gridDim.x * PB;
  for (size_t i = (size_t)blockIdx.x * PB + threadIdx.x; i < words; i += step) table[i] = PC_EMPTY;
  if (blockIdx.x == 0 && threadIdx.x < 8) counters[threadIdx.x] = 0ull;
}

void launch_pointcloud_reset(void* table, uint64_t slots, uint64_t* counters, hipStream_t s) {
  const size_t words = table ? (size_t)slots * 2 : 0;
  size_t nb = (words + PB - 1) / PB;
  nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
  hipLaunchKernelGGL(pc_reset_kernel, dim3((unsigned)nb), dim3(PB), 0, s, (unsigned long long*)table, words, (unsigned long long*)counters);
}

void launch_pointcloud_add_view(const PointCloudView& v, void* rows, uint64_t cap, uint64_t* counters, void* work, hipStream_t s) {
  const size_t n = (size_t)v.H * (size_t)v.W;
  const int nb = (int)pc_nb(n);
  const PcWork w = pc_work(work, n);
  const size_t stride = (size_t)(w.counts[1] - w.counts[0]);      // the four count arrays are equally spaced
  if (v.table) hipLaunchKernelGGL(pc_claim_kernel, dim3(nb), dim3(PB), 0, s, v);
  hipLaunchKernelGGL(pc_select_kernel, dim3(nb), dim3(PB), 0, s, v, w.flag, w.counts[0], stride);
  hipLaunchKernelGGL(pc_scan_kernel, dim3(1), dim3(1024), 0, s, nb, stride, w.counts[0], (unsigned long long)cap, (unsigned long long*)counters, w.hdr);
  hipLaunchKernelGGL(pc_scatter_kernel, dim3(nb), dim3(PB), 0, s, v, w.flag, w.counts[0], w.hdr, (unsigned long long)cap, (uint4*)rows);
}

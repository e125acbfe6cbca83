// Connected components of an indexed triangle mesh and the removal of its small pieces (mm3dgs_mesh_components / mm3dgs_mesh_clean_work_bytes /
// mm3dgs_mesh_clean_plan / mm3dgs_mesh_clean_emit; host statement: mesh_clean.components_host / clean_host).  rows are the mesh's 16-byte rows,
// triangles int32 [T][3].  A triangle is valid when its three indices lie in [0, V); two vertices are connected when a valid triangle uses
// both; label[v] is the smallest vertex index of v's component, tri_count[r] the valid triangles of the component whose label is r.
//
//   mc_init_kernel     parent[v] = v, tri_count[v] = 0 (parent IS the label array).
//   mc_union_kernel    one lane per triangle: union(a, b), union(b, c).  union finds both roots and hooks the LARGER root under the smaller
//                      with one atomicCAS(&parent[hi], hi, lo); when the CAS fails it goes on from the value the CAS returned.
//   mc_flatten_kernel  label[v] = find(v), in place.
//   mc_count_kernel    tri_count[label[a]] += 1 per valid triangle by integer atomicAdd, the lanes of a wave that share a label adding once (a
//                      sum of integers does not depend on its order or its grouping).
//   mc_finish_kernel   one workgroup of 1024 over tri_count / label: the components with a triangle, the largest by the integer maximum of
//                      the key (count << 32) | ~label (the greatest count, on a tie the smallest label), the unreferenced vertices, and
//                      skipped = T - sum(tri_count); counters [0..3], [4..7] = 0.
//
// Why mc_union_kernel ends, and why its result does not depend on the order of arrival:
//   * parent[x] <= x at all times.  parent[x] starts as x and is written by two things only: the CAS, which replaces x by lo < x, and
//     the path-halving store, which replaces a value p < x by parent[p] < p (MC_PATH_HALVING, on: DESIGN.md has the measurement).  Every
//     value ever stored in parent[x] is x itself or a vertex of x's component below x.  A read that is stale (another XCD's L2) returns
//     one of these earlier values, so it is as good as a fresh one for what follows.
//   * find(x) replaces x by parent[x] until parent[x] == x: x decreases strictly with every step, at most V steps.
//   * union holds two candidates and leaves when they are equal.  Otherwise it tries the CAS on the larger one, hi.  The CAS is the
//     one authority on whether hi is a root: it succeeds -- done, hi now hangs under a vertex of the other side -- or it returns the
//     parent another lane gave hi, which is below hi, and the lane goes on from there.  Every failed CAS lowers a candidate, so a lane
//     makes at most 2 V attempts, and a CAS fails only because another lane's CAS has succeeded: no lane waits for another lane.  There
//     is no flag, no spin on a value another wave has yet to produce, no barrier between workgroups and no cooperative launch.
//   * once parent[x] != x, x is never a root again (both writers need parent[x] == x to make it one: none does), so the halving store,
//     which goes to non-roots only, never touches a word a CAS can win.
//   * the smallest vertex m of a component is never hooked: hooking m needs a lo < m in m's component.  When the kernel is over every
//     valid triangle's three vertices reach one root, so each component has exactly one root, m: label = find is the component's minimum
//     whatever the order of arrival.  That, the order-free integer sums, and scatters by rank make every output of this file the same
//     bytes on every call.
//   mc_flatten_kernel's in-place stores obey the same two rules (a root stores itself, a non-root a lower vertex of its component).
//
// Cleaning.  A component is kept in mode 1 (small) when tri_count >= min_triangles (>= 1), in mode 2 (largest) when it is the winner
// mc_finish_kernel left in counters[1]; a vertex is kept with its component (so never when the component has no triangle), a triangle
// when it is valid and its component is kept.
//   mcl_vcount_kernel  per 256 vertices: kept vertices, kept roots (= kept components).
//   mcl_tcount_kernel  per 256 triangles: kept triangles.
//   mcl_scan_kernel    one workgroup of 1024: scan_block_counts over both, the kept components, counters [4..7].
//   mcl_remap_kernel   remap[v] = the new index of a kept vertex (block prefix + block_rank), MC_NONE otherwise.
//   mcl_vertex_kernel  kept rows to out_rows / index at remap[v], below vcap.
//   mcl_triangle_kernel  kept triangles through remap to block prefix + block_rank, below tcap.
//   mcl_dropped_kernel counters [7] from the two totals and the two caps.
// No atomic decides a position.
#include "block_ops.h"
#include "fused_api.h"

#define MB 256
#define MC_NONE 0xffffffffu
#ifndef MC_PATH_HALVING
#define MC_PATH_HALVING 1      // 0: find() without path halving (the A/B of tools/mesh_clean_ab.py; DESIGN.md has the figures)
#endif

static size_t mc_nb(size_t n) { return (n + MB - 1) / MB; }

// work = [uint32 kept vertices per 256][uint32 kept roots per 256][uint32 kept triangles per 256][uint32 remap per vertex] (at least one
// word each: V = 0 and T = 0 are valid sizes)
struct CleanWork { uint32_t* vcounts; uint32_t* ccounts; uint32_t* tcounts; uint32_t* remap; };
static CleanWork clean_work(void* base, size_t V, size_t T, size_t* bytes = nullptr) {
  Carve c = {(uintptr_t)base};
  CleanWork w;
  const size_t nbv = mc_nb(V) ? mc_nb(V) : 1, nbt = mc_nb(T) ? mc_nb(T) : 1;
  w.vcounts = c.take<uint32_t>(nbv);
  w.ccounts = c.take<uint32_t>(nbv);
  w.tcounts = c.take<uint32_t>(nbt);
  w.remap = c.take<uint32_t>(V ? V : 1);
  if (bytes) *bytes = c.at;
  return w;
}
size_t mesh_clean_work_bytes(uint64_t V, uint64_t T) { size_t b; clean_work(nullptr, (size_t)V, (size_t)T, &b); return b; }

// ---- components ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mc_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mc_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x (x < V): every step lowers x
__device__ __forceinline__ uint32_t mc_find(uint32_t* parent, uint32_t x) {
  uint32_t p = mc_load(parent + x);
  while (p != x) {
#if MC_PATH_HALVING
    const uint32_t g = mc_load(parent + p);      // (p < x <= V - 1)
    if (g != p) mc_store(parent + x, g);         // x is not a root and never will be
    x = p;
    p = g;
#else
    x = p;
    p = mc_load(parent + x);
#endif
  }
  return x;
}

__device__ __forceinline__ void mc_union(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = mc_find(parent, a);
    b = mc_find(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;      // (below hi: another lane hooked it)
    b = lo;
  }
}

// the three indices of triangle t (t < T) and whether all lie in [0, V)
__device__ __forceinline__ bool mc_triangle(const int* __restrict__ tris, uint32_t t, uint32_t V, uint32_t& a, uint32_t& b, uint32_t& c) {
  const int* p = tris + (size_t)t * 3;
  a = (uint32_t)p[0]; b = (uint32_t)p[1]; c = (uint32_t)p[2];      // (a negative index is above 2^31 as uint32, V is at most 2^30)
  return a < V && b < V && c < V;
}

__global__ void __launch_bounds__(MB)
mc_init_kernel(uint32_t V, uint32_t* __restrict__ parent, uint32_t* __restrict__ tri_count) {
  const uint32_t v = blockIdx.x * MB + threadIdx.x;
  if (v < V) { parent[v] = v; tri_count[v] = 0u; }
}

__global__ void __launch_bounds__(MB)
mc_union_kernel(uint32_t V, uint32_t T, const int* __restrict__ tris, uint32_t* parent) {
  const uint32_t t = blockIdx.x * MB + threadIdx.x;
  uint32_t a, b, c;
  if (t >= T || !mc_triangle(tris, t, V, a, b, c)) return;
  mc_union(parent, a, b);
  mc_union(parent, b, c);
}

__global__ void __launch_bounds__(MB)
mc_flatten_kernel(uint32_t V, uint32_t* label) {
  const uint32_t v = blockIdx.x * MB + threadIdx.x;
  if (v >= V) return;
  uint32_t x = v, p = mc_load(label + x);
  while (p != x) { x = p; p = mc_load(label + x); }
  if (x != v) mc_store(label + v, x);
}

__global__ void __launch_bounds__(MB)
mc_count_kernel(uint32_t V, uint32_t T, const int* __restrict__ tris, const uint32_t* __restrict__ label, uint32_t* __restrict__ tri_count) {
  const uint32_t t = blockIdx.x * MB + threadIdx.x;
  uint32_t a, b, c;
  const bool valid = t < T && mc_triangle(tris, t, V, a, b, c);
  const uint32_t r = valid ? label[a] : MC_NONE;      // (label[a] <= a < V)
  // the lanes of a wave that share a label add once: neighbouring triangles of a mesh mostly share their component, and every add of a
  // component lands on one word (14 ns each: with one add per triangle the largest component's word bounded the whole call)
  unsigned long long todo = __ballot(valid);
  while (todo) {      // (wave-uniform; at most 64 rounds)
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t lr = (uint32_t)__shfl((int)r, leader, 64);
    const unsigned long long same = __ballot(r == lr);      // (an invalid lane holds MC_NONE, no label)
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(tri_count + lr, (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

__device__ __forceinline__ unsigned long long mc_wave_max(unsigned long long k) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(k, off, 64);
    k = o > k ? o : k;
  }
  return k;
}

__global__ void __launch_bounds__(1024)
mc_finish_kernel(uint32_t V, unsigned long long T, const uint32_t* __restrict__ label, const uint32_t* __restrict__ tri_count,
                 unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long sh[3][16];
  __shared__ unsigned long long shk[16];
  unsigned long long comps = 0, unref = 0, sum = 0, key = 0;
  for (uint32_t v = threadIdx.x; v < V; v += 1024) {
    const uint32_t c = tri_count[v];
    comps += c != 0u;
    unref += c == 0u && label[v] == v;      // a vertex of a component without a triangle: it is alone in it
    sum += c;
    const unsigned long long k = c ? ((unsigned long long)c << 32) | (unsigned long long)(~v) : 0ull;
    key = k > key ? k : key;
  }
  comps = wave_sum_to_lane63_int(comps);
  unref = wave_sum_to_lane63_int(unref);
  sum = wave_sum_to_lane63_int(sum);
  key = mc_wave_max(key);
  if ((threadIdx.x & 63) == 63) {
    const int w = threadIdx.x >> 6;
    sh[0][w] = comps; sh[1][w] = unref; sh[2][w] = sum; shk[w] = key;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t[3] = {0, 0, 0}, k = 0;
    for (int w = 0; w < 16; w++) {
      t[0] += sh[0][w]; t[1] += sh[1][w]; t[2] += sh[2][w];
      k = shk[w] > k ? shk[w] : k;
    }
    counters[0] = t[0];
    counters[1] = k;
    counters[2] = T - t[2];
    counters[3] = t[1];
    counters[4] = 0ull; counters[5] = 0ull; counters[6] = 0ull; counters[7] = 0ull;
  }
}

void launch_mesh_components(uint64_t V, uint64_t T, const int* tris, uint32_t* label, uint32_t* tri_count, uint64_t* counters, hipStream_t s) {
  const unsigned nbv = (unsigned)mc_nb((size_t)V), nbt = (unsigned)mc_nb((size_t)T);
  if (nbv) hipLaunchKernelGGL(mc_init_kernel, dim3(nbv), dim3(MB), 0, s, (uint32_t)V, label, tri_count);
  if (nbv && nbt) {
    hipLaunchKernelGGL(mc_union_kernel, dim3(nbt), dim3(MB), 0, s, (uint32_t)V, (uint32_t)T, tris, label);
    hipLaunchKernelGGL(mc_flatten_kernel, dim3(nbv), dim3(MB), 0, s, (uint32_t)V, label);
    hipLaunchKernelGGL(mc_count_kernel, dim3(nbt), dim3(MB), 0, s, (uint32_t)V, (uint32_t)T, tris, (const uint32_t*)label, tri_count);
  }
  hipLaunchKernelGGL(mc_finish_kernel, dim3(1), dim3(1024), 0, s, (uint32_t)V, (unsigned long long)T, (const uint32_t*)label, (const uint32_t*)tri_count,
                     (unsigned long long*)counters);
}

// ---- cleaning --------------------------------------------------------------------------------------------------------------------------
// what decides whether a component is kept: the mode's threshold, or the winner's label (MC_NONE: no component has a triangle)
struct CleanRule { int mode; uint32_t min_triangles; uint32_t winner; };
__device__ __forceinline__ CleanRule mcl_rule(int mode, uint32_t min_triangles, const unsigned long long* __restrict__ counters) {
  const unsigned long long k = counters[1];
  return {mode, min_triangles, k ? ~(uint32_t)k : MC_NONE};
}
// is the component with label r (r < V) kept
__device__ __forceinline__ bool mcl_kept(const CleanRule& q, uint32_t r, const uint32_t* __restrict__ tri_count) {
  return q.mode == MM3DGS_MESH_CLEAN_LARGEST ? r == q.winner : tri_count[r] >= q.min_triangles;
}

__global__ void __launch_bounds__(MB)
mcl_vcount_kernel(uint32_t V, const uint32_t* __restrict__ label, const uint32_t* __restrict__ tri_count, int mode, uint32_t min_triangles,
                  const unsigned long long* __restrict__ counters, uint32_t* __restrict__ vcounts, uint32_t* __restrict__ ccounts) {
  __shared__ uint32_t wcnt[2][MB / 64];
  const CleanRule q = mcl_rule(mode, min_triangles, counters);
  const uint32_t v = blockIdx.x * MB + threadIdx.x;
  bool kept = false, root = false;
  if (v < V) {
    const uint32_t r = label[v];
    kept = r < V && mcl_kept(q, r, tri_count);      // (r <= v by the rule; the test keeps a foreign label array inside tri_count)
    root = kept && r == v;
  }
  const bool is[2] = {kept, root};
  const uint32_t t = block_flag_counts(is, wcnt);
  if (threadIdx.x == 0) vcounts[blockIdx.x] = t;
  if (threadIdx.x == 1) ccounts[blockIdx.x] = t;
}

__device__ __forceinline__ bool mcl_triangle_kept(const CleanRule& q, const int* __restrict__ tris, uint32_t t, uint32_t V, const uint32_t* __restrict__ label,
                                                  const uint32_t* __restrict__ tri_count) {
  uint32_t a, b, c;
  if (!mc_triangle(tris, t, V, a, b, c)) return false;
  const uint32_t r = label[a];
  return r < V && mcl_kept(q, r, tri_count);
}

__global__ void __launch_bounds__(MB)
mcl_tcount_kernel(uint32_t V, uint32_t T, const int* __restrict__ tris, const uint32_t* __restrict__ label, const uint32_t* __restrict__ tri_count, int mode,
                  uint32_t min_triangles, const unsigned long long* __restrict__ counters, uint32_t* __restrict__ tcounts) {
  __shared__ uint32_t wcnt[1][MB / 64];
  const CleanRule q = mcl_rule(mode, min_triangles, counters);
  const uint32_t t = blockIdx.x * MB + threadIdx.x;
  const bool is[1] = {t < T && mcl_triangle_kept(q, tris, t, V, label, tri_count)};
  const uint32_t n = block_flag_counts(is, wcnt);
  if (threadIdx.x == 0) tcounts[blockIdx.x] = n;
}

__global__ void __launch_bounds__(1024)
mcl_scan_kernel(int nbv, int nbt, uint32_t* __restrict__ vcounts, const uint32_t* __restrict__ ccounts, uint32_t* __restrict__ tcounts,
                unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long sh[16];
  __shared__ uint32_t totals[2];
  const unsigned long long comps = block_array_sum(nbv, ccounts, sh);
  scan_block_counts(nbv, vcounts, &totals[0]);
  __syncthreads();
  scan_block_counts(nbt, tcounts, &totals[1]);
  if (threadIdx.x == 0) {      // (lane 0 wrote both totals itself)
    counters[4] = comps;
    counters[5] = totals[0];
    counters[6] = totals[1];
    counters[7] = 0ull;
  }
}

__global__ void __launch_bounds__(MB)
mcl_remap_kernel(uint32_t V, const uint32_t* __restrict__ label, const uint32_t* __restrict__ tri_count, int mode, uint32_t min_triangles,
                 const unsigned long long* __restrict__ counters, const uint32_t* __restrict__ vpre, uint32_t* __restrict__ remap) {
  __shared__ uint32_t wsum[MB / 64];
  const CleanRule q = mcl_rule(mode, min_triangles, counters);
  const uint32_t v = blockIdx.x * MB + threadIdx.x;
  bool kept = false;
  if (v < V) {
    const uint32_t r = label[v];
    kept = r < V && mcl_kept(q, r, tri_count);
  }
  const uint32_t pos = block_rank(kept, vpre[blockIdx.x], wsum);      // (every lane is here)
  if (v < V) remap[v] = kept ? pos : MC_NONE;
}

void launch_mesh_clean_plan(uint64_t V, uint64_t T, const int* tris, const uint32_t* label, const uint32_t* tri_count, int mode, uint32_t min_triangles,
                            void* work, uint64_t* counters, hipStream_t s) {
  const CleanWork w = clean_work(work, (size_t)V, (size_t)T);
  const unsigned nbv = (unsigned)mc_nb((size_t)V), nbt = (unsigned)mc_nb((size_t)T);
  const unsigned long long* c = (const unsigned long long*)counters;
  const bool any = nbv && nbt;      // without a vertex or without a triangle nothing is kept: the scan over no blocks writes the zeros
  if (any) hipLaunchKernelGGL(mcl_vcount_kernel, dim3(nbv), dim3(MB), 0, s, (uint32_t)V, label, tri_count, mode, min_triangles, c, w.vcounts, w.ccounts);
  if (any) hipLaunchKernelGGL(mcl_tcount_kernel, dim3(nbt), dim3(MB), 0, s, (uint32_t)V, (uint32_t)T, tris, label, tri_count, mode, min_triangles, c, w.tcounts);
  hipLaunchKernelGGL(mcl_scan_kernel, dim3(1), dim3(1024), 0, s, any ? (int)nbv : 0, any ? (int)nbt : 0, w.vcounts, (const uint32_t*)w.ccounts, w.tcounts,
                     (unsigned long long*)counters);
  if (any) hipLaunchKernelGGL(mcl_remap_kernel, dim3(nbv), dim3(MB), 0, s, (uint32_t)V, label, tri_count, mode, min_triangles, c, (const uint32_t*)w.vcounts, w.remap);
}

__global__ void __launch_bounds__(MB)
mcl_vertex_kernel(uint32_t V, const uint4* __restrict__ rows, const uint32_t* __restrict__ remap, unsigned long long vcap, uint4* __restrict__ out_rows,
                  uint32_t* __restrict__ index) {
  const uint32_t v = blockIdx.x * MB + threadIdx.x;
  if (v >= V) return;
  const uint32_t pos = remap[v];
  if (pos == MC_NONE || (unsigned long long)pos >= vcap) return;
  out_rows[pos] = rows[v];      // one 16-byte load, one 16-byte store: the row's bytes as they are
  if (index) index[pos] = v;
}

__global__ void __launch_bounds__(MB)
mcl_triangle_kernel(uint32_t V, uint32_t T, const int* __restrict__ tris, const uint32_t* __restrict__ remap, const uint32_t* __restrict__ tpre,
                    unsigned long long tcap, int* __restrict__ out_tris) {
  __shared__ uint32_t wsum[MB / 64];
  const uint32_t t = blockIdx.x * MB + threadIdx.x;
  uint32_t a = 0, b = 0, c = 0;
  bool kept = false;
  if (t < T && mc_triangle(tris, t, V, a, b, c)) {
    a = remap[a];
    kept = a != MC_NONE;      // (a triangle's three vertices share a component: kept or dropped together)
    if (kept) { b = remap[b]; c = remap[c]; }
  }
  const uint32_t pos = block_rank(kept, tpre[blockIdx.x], wsum);      // (every lane is here)
  if (kept && (unsigned long long)pos < tcap) {
    int* o = out_tris + (size_t)pos * 3;
    o[0] = (int)a; o[1] = (int)b; o[2] = (int)c;
  }
}

__global__ void mcl_dropped_kernel(unsigned long long vcap, unsigned long long tcap, unsigned long long* __restrict__ counters) {
  const unsigned long long kv = counters[5], kt = counters[6];
  counters[7] = (kv > vcap ? kv - vcap : 0ull) | ((kt > tcap ? kt - tcap : 0ull) << 32);
}

void launch_mesh_clean_emit(uint64_t V, uint64_t T, const void* rows, const int* tris, const void* work, void* out_rows, uint64_t vcap, int* out_tris,
                            uint64_t tcap, uint32_t* index, uint64_t* counters, hipStream_t s) {
  const CleanWork w = clean_work((void*)work, (size_t)V, (size_t)T);
  const unsigned nbv = (unsigned)mc_nb((size_t)V), nbt = (unsigned)mc_nb((size_t)T);
  if (nbv && nbt && vcap) hipLaunchKernelGGL(mcl_vertex_kernel, dim3(nbv), dim3(MB), 0, s, (uint32_t)V, (const uint4*)rows, (const uint32_t*)w.remap, (unsigned long long)vcap,
                                      (uint4*)out_rows, index);
  if (nbv && nbt && tcap) hipLaunchKernelGGL(mcl_triangle_kernel, dim3(nbt), dim3(MB), 0, s, (uint32_t)V, (uint32_t)T, tris, (const uint32_t*)w.remap,
                                             (const uint32_t*)w.tcounts, (unsigned long long)tcap, out_tris);
  hipLaunchKernelGGL(mcl_dropped_kernel, dim3(1), dim3(1), 0, s, (unsigned long long)vcap, (unsigned long long)tcap, (unsigned long long*)counters);
}

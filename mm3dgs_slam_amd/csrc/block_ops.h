// What the kernels outside the tracking and mapping loops (compact, align, eval, pointcloud, tsdf, geometry) share: the workgroup scan,
// count and sum idioms, each stated once, and the cursor that carves a work buffer.  The LDS scratch is the caller's.  No atomic decides a
// position and every floating-point sum has one fixed order: the same inputs give the same bytes on every call.
// (loss_pixel.h's block_sums is not one of these: float and double columns, another order, and it sits in the mapping loop.)
#pragma once
#include "mm3dgs_common.h"

// ---- work buffers: one statement of a layout serves its size (walked from 0) and its pointers (walked from the buffer) ----------------
struct Carve {
  uintptr_t at;
  template <typename T> T* take(size_t count) { T* p = (T*)at; at += align_up(count * sizeof(T), 256); return p; }
};

// ---- one workgroup of 1024 lanes over an array of per-256 counts ---------------------------------------------------------------------
// block_counts[0..nb) -> exclusive prefix in place, total to *total
__device__ __forceinline__ void scan_block_counts(int nb, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ total) {
  __shared__ uint32_t wtot[16];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + tid;
    const uint32_t v = i < nb ? block_counts[i] : 0u;
    const uint32_t x = wave_scan_incl(v);
    if (lane == 63) wtot[wv] = x;
    __syncthreads();
    uint32_t pre = carry;
    for (int w = 0; w < wv; w++) pre += wtot[w];
    if (i < nb) block_counts[i] = pre + x - v;
    __syncthreads();
    if (tid == 1023) carry = pre + x;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

__device__ __forceinline__ uint32_t wave_sum_to_lane63_int(uint32_t s) { return wave_scan_incl(s); }
__device__ __forceinline__ unsigned long long wave_sum_to_lane63_int(unsigned long long s) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_up(s, off, 64);      // (no 64-bit DPP add; integer sums: any order)
  return s;
}
// sum of a[0..n) as T (uint32_t or unsigned long long), valid in lane 0; every lane calls; sh: 16 words of T
template <typename T>
__device__ __forceinline__ T block_array_sum(int n, const uint32_t* __restrict__ a, T* sh) {
  T s = 0;
  for (int i = threadIdx.x; i < n; i += 1024) s += a[i];
  s = wave_sum_to_lane63_int(s);
  __syncthreads();                                                         // (sh may hold the previous call's sums)
  if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  T t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < 16; w++) t += sh[w];
  return t;
}

// ---- one workgroup of 256 lanes, every lane calls ----------------------------------------------------------------------------------
// position of this lane's element among the flagged ones of the workgroup, offset by the workgroup's exclusive prefix `base`
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t base, uint32_t* wsum) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) wsum[wv] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t pre = base;
  for (int w = 0; w < wv; w++) pre += wsum[w];
  return pre + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// inclusive scan of v; wtot: 4 words
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* wtot) {
  const uint32_t x = wave_scan_incl(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 63) wtot[wv] = x;
  __syncthreads();
  uint32_t pre = 0;
  for (int w = 0; w < wv; w++) pre += wtot[w];
  return pre + x;
}

// K flags, or K uint32 values, per lane -> the K workgroup totals, total k in lane k (k < K); sh: K rows of 4 words
template <int K>
__device__ __forceinline__ uint32_t block_totals(uint32_t (*sh)[4]) {
  __syncthreads();
  const uint32_t* r = sh[threadIdx.x < K ? threadIdx.x : 0];
  return r[0] + r[1] + r[2] + r[3];
}
template <int K>
__device__ __forceinline__ uint32_t block_flag_counts(const bool (&flag)[K], uint32_t (*sh)[4]) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    const unsigned long long m = __ballot(flag[k]);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = (uint32_t)__popcll(m);
  }
  return block_totals<K>(sh);
}
template <int K>
__device__ __forceinline__ uint32_t block_sums_u32(const uint32_t (&v)[K], uint32_t (*sh)[4]) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    const uint32_t x = wave_scan_incl(v[k]);
    if ((threadIdx.x & 63) == 63) sh[k][threadIdx.x >> 6] = x;
  }
  return block_totals<K>(sh);
}

// NR doubles per lane -> their workgroup sums in place, each wave's DPP sum and then (w0 + w1) + (w2 + w3); valid in lane 0, or with
// ALL_LANES in every lane.  Additions only: the including file's contraction setting does not reach it.  sh: 4 rows of NR doubles
template <int NR, bool ALL_LANES>
__device__ __forceinline__ void block_sums_f64(double (&v)[NR], double (*sh)[NR]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NR; k++) {
    const double t = wave_sum_to_lane63_f64(v[k]);
    if (lane == 63) sh[wv][k] = t;
  }
  __syncthreads();
  if (ALL_LANES || threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < NR; k++) v[k] = (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
}

// The two device helpers of the order-preserving compaction (per-256 counts, one-workgroup scan, scatter by ballot rank) that compact.hip
// and pointcloud.hip share.  No atomic decides a position: the same flags give the same rows in the same order on every call.
#pragma once
#include "mm3dgs_common.h"

// one workgroup of 1024 lanes: block_counts[0..nb) -> exclusive prefix in place, total to *total
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

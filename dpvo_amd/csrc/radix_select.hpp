// radix_select.hpp -- the value of one sorted rank among `count` fp32 values by
// a four-pass radix select (no sort), one workgroup.  Shared by frontend.hip
// (the median depth of dpvo_frame_init) and dataset.hip (the two order
// statistics of normalize_depth's quantile).
#pragma once

#include "common.hpp"

namespace dpvo {

// order-preserving key of a float: a < b  <=>  key(a) < key(b) (-0 below +0)
__device__ __forceinline__ uint32_t float_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct RadixSelectLds {
  int hist[256];
  int wtot[4];
  uint32_t prefix;
  int rank;
};

// The key of sorted rank `rank` (0-based, < count) among key_at(0..count).
// Called by every thread of a workgroup of a multiple of 64 threads, at least
// 256; key_at(i) is evaluated once per pass, by thread i % blockDim.x.  Eight
// bits per pass from the top: the bins of the keys that share the prefix found
// so far are counted with LDS atomics (integer counts: the result does not
// depend on their order), an exclusive scan of the 256 bins finds the bin that
// holds the rank.  Starts and ends with a barrier.
template <typename KeyAt>
__device__ __forceinline__ uint32_t block_radix_select(int count, int rank, KeyAt key_at,
                                                       RadixSelectLds& s) {
  const int tid = threadIdx.x, T = blockDim.x;
  __syncthreads();
  if (tid == 0) {
    s.prefix = 0;
    s.rank = rank;
  }
  uint32_t prefix = 0;
#pragma unroll 1
  for (int pass = 0; pass < 4; pass++) {
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    if (tid < 256) s.hist[tid] = 0;
    __syncthreads();
    // four keys per trip, every load issued before the first count: a trip costs
    // one memory latency, not four
    for (int i0 = tid; i0 < count; i0 += 4 * T) {
      uint32_t k[4];
#pragma unroll
      for (int u = 0; u < 4; u++) k[u] = i0 + u * T < count ? key_at(i0 + u * T) : 0u;
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (i0 + u * T < count && (k[u] & himask) == prefix)
          atomicAdd(&s.hist[(k[u] >> shift) & 255u], 1);
    }
    __syncthreads();
    // exclusive scan of the 256 bins, one per thread of the first four waves;
    // the bin holding the rank is selected
    const int c = tid < 256 ? s.hist[tid] : 0;
    const int incl = wave_incl_sum(c);
    if (tid < 256 && (tid & 63) == 63) s.wtot[tid >> 6] = incl;
    __syncthreads();
    int excl = incl - c;
    for (int w = 0; w < (tid >> 6) && w < 4; w++) excl += s.wtot[w];
    const int r = s.rank;
    __syncthreads();  // every thread has read the rank
    if (tid < 256 && c > 0 && r >= excl && r < excl + c) {
      s.prefix = prefix | ((uint32_t)tid << shift);
      s.rank = r - excl;
    }
    __syncthreads();
    prefix = s.prefix;
  }
  return prefix;
}

}  // namespace dpvo

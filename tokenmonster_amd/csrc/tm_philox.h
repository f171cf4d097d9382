// tm_philox.h - the selection rule that tm_batch_collate_masked (tm_masked.hip) and tm_batch_collate_denoise (tm_denoise.hip) share: Philox4x32-10
// keyed by the place g of an id in the batch's id buffer, the reach of the span an id opens, and the end of no span for the running maximum
// of span ends both kernels select by (the rule: include/tokenmonster_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tmh {

__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11), counter (g, 0, 0), key (k0, k1)
__host__ __device__ __forceinline__ void philox4x32_10(uint64_t g, uint32_t k0, uint32_t k1, uint32_t w[4]) {
  uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
  for (uint32_t i = 0; i < 10; i++) {
    if (i) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// the ids a span that opens at this id covers (0: none opens).  Args: start_thr, span_min, span_n = span_max - span_min + 1
template <typename Args>
__device__ __forceinline__ uint32_t reach_of(const Args& m, const uint32_t w[4]) {
  return (uint64_t)w[0] < m.start_thr ? m.span_min + mulhi32(w[1], m.span_n) : 0u;
}

constexpr int32_t NO_END = -(1 << 20);       // the end of no span: in front of every position of a tile and of the 31 ids before it

}  // namespace tmh

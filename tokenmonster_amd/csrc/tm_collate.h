// tm_collate.h - what the fixed-shape outputs share (tm_collate.hip: ids, masks, streams; tm_spans.hip: the byte spans of the ids): an output as
// one flat run of elements with 16-byte stores between an unaligned head and tail, and the plan of a row of tm_batch_collate.
#pragma once
#include <algorithm>

#include "tm_pipeline.h"

namespace tmh {

// ---- a flat output of n elements of T ------------------------------------------------------------------------------------------------------
// work-items [0, nvec): the 16-byte vector at element head + t * (16 / sizeof(T)); then `head` single elements in front and the single
// elements behind the last vector.  A base that is not even a multiple of sizeof(T) has no vectors at all (head == n).
struct Flat { uint64_t n, head, nvec; };
inline Flat flat_of(const void* out, uint64_t n, uint32_t elem) {
  const uint64_t a = (uint64_t)reinterpret_cast<uintptr_t>(out);
  Flat f{n, n, 0};
  if (a % elem) return f;
  const uint64_t mis = a & 15u;
  f.head = std::min<uint64_t>(mis ? (16 - mis) / elem : 0, n);
  f.nvec = (n - f.head) / (16 / elem);
  return f;
}
inline uint64_t flat_items(const Flat& f, uint32_t elem) { return f.n - f.nvec * (16 / elem) + f.nvec; }

template <typename T>
__device__ __forceinline__ bool flat_span(const Flat& f, uint64_t t, uint64_t& e0, uint32_t& cnt) {
  constexpr uint32_t PER = 16 / sizeof(T);
  if (t < f.nvec) { e0 = f.head + t * PER; cnt = PER; return true; }
  uint64_t u = t - f.nvec;
  cnt = 1;
  if (u < f.head) { e0 = u; return true; }
  u -= f.head;
  const uint64_t tail0 = f.head + f.nvec * PER;
  if (u < f.n - tail0) { e0 = tail0 + u; return true; }
  return false;
}
template <typename T>
__device__ __forceinline__ void flat_store(T* __restrict__ out, uint64_t e0, uint32_t cnt, const T* vals) {
  constexpr uint32_t PER = 16 / sizeof(T);
  if (cnt == PER) {
    uint4 v;
    __builtin_memcpy(&v, vals, 16);
    *reinterpret_cast<uint4*>(out + e0) = v;          // (e0 is on a 16-byte boundary: flat_of)
  } else {
    out[e0] = vals[0];
  }
}

// ---- one document per row (tm_batch_collate, tm_batch_collate_spans) -----------------------------------------------------------------------------
struct CollateArgs {
  const uint32_t* ids;        // the batch's ids
  const uint64_t* toff;       // tok_offsets + first_doc
  uint32_t rows, L, pad, bos, eos, flags;      // bos / eos: TM_NONE = none
};
// what row r holds: `len` entries [bos?] content [eos?] from column `lo` on, the content from ids[src]
struct RowPlan { uint64_t src; uint32_t lo, len; };
__device__ __forceinline__ RowPlan row_plan(const CollateArgs& a, uint64_t r) {
  const uint64_t b0 = a.toff[r], b1 = a.toff[r + 1];
  const uint32_t ns = (a.bos != TM_NONE ? 1u : 0u) + (a.eos != TM_NONE ? 1u : 0u);
  const uint32_t m = (uint32_t)std::min<uint64_t>(b1 - b0, a.L - ns);            // (L >= ns: checked by the host)
  RowPlan p;
  p.src = (a.flags & TM_COLLATE_KEEP_TAIL) ? b1 - m : b0;
  p.len = m + ns;
  p.lo = (a.flags & TM_COLLATE_PAD_LEFT) ? a.L - p.len : 0u;
  return p;
}

constexpr uint64_t COLLATE_MAX_ELEMS = 1ull << 36;       // elements of one output: keeps every grid below 2^31 workgroups

inline uint32_t grid_of(uint64_t items) { return (uint32_t)((items + 255) / 256); }
inline int launch_check() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? TM_OK : hip_fail(e, "kernel launch");
}

// the arguments every layout shares (ids_out: only that it is there)
int check_how(const tm_batch* b, const tm_collate* how, const void* ids_out, const char* who);

}  // namespace tmh

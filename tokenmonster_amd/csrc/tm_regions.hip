// tm_regions.hip — region labels: character ranges of the documents (entities, answers, the parts of a loss mask) aligned to the ids where they lie
// (the rule: tokenmonster_hip.h, "region labels").  The pairs come from the span pass (tm_spans.hip, tm_units.hip) into the batch's own buffer, in the
// `text` and `unit` the regions are given in; the documents' lengths in that unit cut the regions (batch_doc_units_on, tm_units.hip).
//
// k_region_labels: a wavefront (a workgroup of 64) takes RG_TILE = 256 consecutive ids of the ragged stream, four per lane - a lane's four pairs one
// 32-byte read, its four labels one 16-byte store (two for 8-byte labels).  The documents of the tile's first and last id are found uniformly
// (doc_of_id).  One document - the common case: two uniform binary searches over its regions give the window [r0, r1) that can meet the tile's extent,
// from the lowest begin of the tile to its largest end; a window of at most RG_WIN = 128 regions is staged in LDS, cut, as three planes of 128 words
// (12 bytes a region, 1.5 KB per wavefront), and every lane searches LDS for each of its ids.  A tile that crosses a document boundary, or a larger
// window: every lane finds the document of its ids itself and searches that document's regions in global memory.  Both paths run the one search
// (find_regions) over the regions as the rule cuts them, so they give the same labels.
// Per id the search leaves the first and last region it meets, [jf, jl] - sorted regions that do not overlap make the regions an id meets a run, less
// the empty ones.  The token range of a region is an atomicMin / atomicMax of the ids' indices: a lane issues the min only where the id in front (the
// lane's own, or the neighbour lane's last by __shfl) does not meet the same region, the max only where the id behind does not - a region over a whole
// tile costs two atomics per wavefront.  The atomics work on pairs in the batch's own buffer (the caller's array may be page-locked host memory):
// k_region_init sets them to (0xFFFFFFFF, 0) and counts the regions that break the order rule, a ballot and one atomic add per wavefront;
// k_region_finish writes (first, last + 1), or (0, 0), to the caller.
// k_collate_labels: the ragged labels laid out like tm_batch_collate's rows - the walk of tm_collate.h's fill_walk with the specials as FLAGS (any ignore_label is
// a label, TM_NONE's bit pattern too) and a store that sign-extends.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tm_pipeline.h"
#include "tm_collate.h"

namespace tmh {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t RG_TILE = 256;      // ids per wavefront
constexpr uint32_t RG_WIN = 128;       // regions a wavefront stages in LDS

struct RegionArgs {
  const uint32_t* spans;        // the ragged pairs, 32-byte aligned (the batch's own buffer)
  const uint64_t* toff;         // tok_offsets[ndocs + 1]
  const uint64_t* roff;         // reg_offsets[ndocs + 1]
  const uint32_t* regs;         // regions[nreg][3]
  const uint32_t* doc_len;      // the documents' lengths in the regions' unit
  uint32_t* rtok;               // the token ranges the atomics work on, in the batch's own buffer (null: not asked for)
  uint64_t total;
  uint32_t ndocs, vec;          // vec: labels_out lies on a 16-byte boundary
  int32_t ignore;
};

// what the search leaves for an id: the first and last region of its document it meets (jf > jl: none) and the first one's label
struct RegionHit { uint32_t jf, jl; int32_t label; };

// The regions [lo, hi) of a document as rb(j), re(j) give them (cut to the document), an id with the pair (b, e).  It meets region j if the region is
// not empty and - e > b: b < re && rb < e; e == b: rb <= b && b < re.  Ends never decrease, so the first region with re > b is found by bisection; the
// ids' run of regions goes on while a region begins in front of the id's end (`bound`: e, or b + 1 for an id without units).
template <typename RB, typename RE>
__device__ __forceinline__ void find_regions(uint32_t b, uint32_t e, uint32_t lo, uint32_t hi, RB rb, RE re, uint32_t& jf, uint32_t& jl) {
  const uint32_t n = hi;
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (re(mid) > b) hi = mid; else lo = mid + 1u; }
  const uint64_t bound = e > b ? (uint64_t)e : (uint64_t)b + 1u;
  jf = 1u; jl = 0u;
  for (uint32_t j = lo; j < n; j++) {
    const uint32_t x = rb(j), y = re(j);
    if (x >= bound) break;
    if (x < y && b < y) { if (jf > jl) jf = j; jl = j; }
  }
}

__device__ __forceinline__ uint32_t region_count(const uint64_t* __restrict__ roff, uint32_t d) {
  const uint64_t a = roff[d], z = roff[d + 1];
  return z > a ? (uint32_t)std::min<uint64_t>(z - a, 0xFFFFFFFFull) : 0u;
}

template <typename T>
__global__ __launch_bounds__(64) void k_region_labels(RegionArgs a, T* __restrict__ out) {
  __shared__ uint32_t s_rb[RG_WIN], s_re[RG_WIN], s_lab[RG_WIN];
  const uint32_t lane = threadIdx.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * RG_TILE;                    // (< total: the grid covers the ids and no more)
  const uint64_t tl = t0 + 4u * lane;
  const uint32_t live = tl >= a.total ? 0u : (uint32_t)std::min<uint64_t>(a.total - tl, 4u);
  uint32_t pb[4] = {0u, 0u, 0u, 0u}, pe[4] = {0u, 0u, 0u, 0u};
  if (live == 4u) {
    const u32x4 q0 = *reinterpret_cast<const u32x4*>(a.spans + 2u * tl), q1 = *reinterpret_cast<const u32x4*>(a.spans + 2u * tl + 4u);
    pb[0] = q0.x; pe[0] = q0.y; pb[1] = q0.z; pe[1] = q0.w; pb[2] = q1.x; pe[2] = q1.y; pb[3] = q1.z; pe[3] = q1.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) if (k < live) { pb[k] = a.spans[2u * (tl + k)]; pe[k] = a.spans[2u * (tl + k) + 1u]; }
  }
  // the tile's extent, over the lanes that hold ids
  uint32_t lo = 0xFFFFFFFFu;
  uint64_t hi = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {                  // (k as a constant everywhere: the lane's pairs and hits stay in registers)
    if (k >= live) continue;
    lo = std::min(lo, pb[k]);
    hi = std::max<uint64_t>(hi, pe[k] > pb[k] ? (uint64_t)pe[k] : (uint64_t)pb[k] + 1u);
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    lo = std::min(lo, (uint32_t)__shfl_xor((int)lo, m));
    hi = std::max<uint64_t>(hi, (uint64_t)__shfl_xor((unsigned long long)hi, m));
  }
  const uint32_t d_first = doc_of_id(a.toff, a.ndocs, t0);
  const uint32_t d_last = doc_of_id(a.toff, a.ndocs, std::min<uint64_t>(t0 + RG_TILE, a.total) - 1u);
  // the window of the one document's regions that can meet the extent: [first with end > lo, first with begin >= hi)
  bool staged = false;
  uint32_t r0 = 0, r1 = 0;
  if (d_first == d_last) {
    const uint32_t n = region_count(a.roff, d_first), len = a.doc_len[d_first];
    const uint32_t* __restrict__ R = a.regs + 3u * a.roff[d_first];
    uint32_t x = 0, y = n;
    while (x < y) { const uint32_t mid = x + (y - x) / 2u; if (std::min(R[3ull * mid + 1u], len) > lo) y = mid; else x = mid + 1u; }
    r0 = x; y = n;
    while (x < y) { const uint32_t mid = x + (y - x) / 2u; if ((uint64_t)std::min(R[3ull * mid], len) >= hi) y = mid; else x = mid + 1u; }
    r1 = x;
    staged = r1 - r0 <= RG_WIN;
    if (staged) {
      for (uint32_t j = lane; j < r1 - r0; j += 64u) {
        const uint32_t* __restrict__ r = R + 3ull * (r0 + j);
        s_rb[j] = std::min(r[0], len); s_re[j] = std::min(r[1], len); s_lab[j] = r[2];
      }
    }
  }
  __syncthreads();                                     // (one wavefront: the staged window is there for all its lanes)
  RegionHit h[4];
  uint32_t doc[4], idx[4];                             // an id's document and its index inside it
  uint32_t d = d_first;
  uint64_t d_end = 0;                                  // the first id behind document d, once it has been looked up
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    h[k] = RegionHit{1u, 0u, a.ignore};
    doc[k] = 0xFFFFFFFFu; idx[k] = 0u;
    if (k >= live) continue;
    const uint64_t t = tl + k;
    if (staged) {
      find_regions(pb[k], pe[k], 0u, r1 - r0, [&](uint32_t j) { return s_rb[j]; }, [&](uint32_t j) { return s_re[j]; }, h[k].jf, h[k].jl);
      if (h[k].jf <= h[k].jl) { h[k].label = (int32_t)s_lab[h[k].jf]; h[k].jf += r0; h[k].jl += r0; }
    } else {
      if (d_first != d_last && (d_end == 0 || t >= d_end)) { d = doc_of_id(a.toff, a.ndocs, t); d_end = a.toff[d + 1]; }
      const uint32_t len = a.doc_len[d];
      const uint32_t* __restrict__ R = a.regs + 3u * a.roff[d];
      find_regions(pb[k], pe[k], 0u, region_count(a.roff, d), [&](uint32_t j) { return std::min(R[3ull * j], len); },
                   [&](uint32_t j) { return std::min(R[3ull * j + 1u], len); }, h[k].jf, h[k].jl);
      if (h[k].jf <= h[k].jl) h[k].label = (int32_t)R[3ull * h[k].jf + 2u];
    }
    doc[k] = d;
    idx[k] = (uint32_t)(t - a.toff[d]);
  }
  // the labels: one 16-byte store per four 4-byte labels, two per four 8-byte ones
  if (live == 4u && a.vec) {
    if (sizeof(T) == 4) {
      u32x4 v;
      v.x = (uint32_t)h[0].label; v.y = (uint32_t)h[1].label; v.z = (uint32_t)h[2].label; v.w = (uint32_t)h[3].label;
      *reinterpret_cast<u32x4*>(out + tl) = v;
    } else {
      const int64_t w[4] = {h[0].label, h[1].label, h[2].label, h[3].label};
      u32x4 v0, v1;
      __builtin_memcpy(&v0, &w[0], 16);
      __builtin_memcpy(&v1, &w[2], 16);
      *reinterpret_cast<u32x4*>(out + tl) = v0;
      *reinterpret_cast<u32x4*>(out + tl + 2u) = v1;
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) if (k < live) out[tl + k] = (T)h[k].label;
  }
  if (!a.rtok) return;                                 // (uniform)
  // the regions' token ranges.  The id in front of a lane's first and behind its last is the neighbour lane's: none at the ends of the wavefront.
  const int before = lane > 0u ? (int)lane - 1 : 0, behind = lane < 63u ? (int)lane + 1 : 63;
  uint32_t pd = (uint32_t)__shfl((int)doc[3], before), pf = (uint32_t)__shfl((int)h[3].jf, before), pl = (uint32_t)__shfl((int)h[3].jl, before);
  const uint32_t nd = (uint32_t)__shfl((int)doc[0], behind), nf = (uint32_t)__shfl((int)h[0].jf, behind), nl = (uint32_t)__shfl((int)h[0].jl, behind);
  if (lane == 0u) pd = 0xFFFFFFFFu;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    const bool last = k == 3u;
    const uint32_t qd = last ? (lane == 63u ? 0xFFFFFFFFu : nd) : doc[k < 3u ? k + 1u : 3u];
    const uint32_t qf = last ? nf : h[k < 3u ? k + 1u : 3u].jf, ql = last ? nl : h[k < 3u ? k + 1u : 3u].jl;
    if (k < live && h[k].jf <= h[k].jl) {
      const uint64_t base = a.roff[doc[k]];
      const uint32_t len = a.doc_len[doc[k]];
      for (uint32_t j = h[k].jf; j <= h[k].jl; j++) {
        if (j != h[k].jf && j != h[k].jl) {            // a region inside the run: met unless it is empty
          const uint32_t* __restrict__ r = a.regs + 3ull * (base + j);
          if (std::min(r[0], len) >= std::min(r[1], len)) continue;
        }
        uint32_t* __restrict__ o = a.rtok + 2ull * (base + j);
        if (!(pd == doc[k] && pf <= j && j <= pl)) atomicMin(o, idx[k]);
        if (!(qd == doc[k] && qf <= j && j <= ql)) atomicMax(o + 1, idx[k]);
      }
    }
    pd = doc[k]; pf = h[k].jf; pl = h[k].jl;
  }
}

// one work-item per region: the pair of its token range set to (0xFFFFFFFF, 0), and whether it breaks the order rule - its begin behind its end, or in
// front of the end of the region before it in its document - counted by ballot, one atomic add per wavefront.  No lane leaves before the ballot.
__global__ __launch_bounds__(256) void k_region_init(const uint64_t* __restrict__ roff, uint32_t ndocs, const uint32_t* __restrict__ regs, uint64_t nreg,
                                                     uint32_t* __restrict__ rtok, uint32_t* bad) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool breaks = false;
  if (r < nreg) {
    if (rtok) { rtok[2u * r] = 0xFFFFFFFFu; rtok[2u * r + 1u] = 0u; }
    if (bad && r >= roff[0]) {
      breaks = regs[3u * r] > regs[3u * r + 1u];
      if (!breaks && r > roff[0]) {
        uint32_t lo = 0, hi = ndocs;                   // the document of region r: the last one whose first region is not behind it
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (roff[mid] <= r) lo = mid; else hi = mid; }
        breaks = roff[lo] < r && regs[3u * (r - 1u) + 1u] > regs[3u * r];
      }
    }
  }
  if (bad) {
    const unsigned long long m = __ballot(breaks);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(bad, (uint32_t)__popcll(m));
  }
}

__global__ void k_region_clear(uint32_t* bad) { *bad = 0u; }

// the pairs as the atomics left them -> (first, last + 1), or (0, 0) for a region no id met, into the caller's array; the count of regions out of order
// into the caller's word
__global__ __launch_bounds__(256) void k_region_finish(const uint32_t* __restrict__ rtok, uint64_t nreg, uint32_t* __restrict__ rtok_out, const uint32_t* bad,
                                                       uint32_t* bad_out) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (bad_out && r == 0) *bad_out = *bad;
  if (!rtok_out || r >= nreg) return;
  const uint32_t first = rtok[2u * r], last = rtok[2u * r + 1u];
  const bool none = first == 0xFFFFFFFFu;              // (no id: the max is still 0)
  rtok_out[2u * r] = none ? 0u : first;
  rtok_out[2u * r + 1u] = none ? 0u : last + 1u;
}

// ---- k_collate_labels: the walk of rows of fill_walk (tm_collate.h), spelled out, over the ragged labels ------------------------------------------------
// The plan of a row is row_plan's, asked with a CollateArgs whose bos / eos only say whether the special is there.
struct LabelRows {
  CollateArgs c;              // toff, rows, L, flags; bos / eos: 0 = given, TM_NONE = none; ids and pad unused
  const int32_t* labels;      // the ragged labels
  int32_t ignore;
};
template <typename T>
__global__ __launch_bounds__(256) void k_collate_labels(LabelRows a, Flat f, T* __restrict__ out) {
  constexpr uint32_t PER = 16 / sizeof(T);
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t e0;
  uint32_t cnt;
  if (!flat_span<T>(f, t, e0, cnt)) return;
  const uint32_t L = a.c.L;
  uint64_t r;
  uint32_t c;
  if (f.n <= 0xFFFFFFFFull) { r = (uint32_t)e0 / L; c = (uint32_t)e0 - (uint32_t)r * L; }
  else { r = e0 / L; c = (uint32_t)(e0 - r * L); }
  RowPlan p = row_plan(a.c, r);
  const uint32_t hb = a.c.bos != TM_NONE ? 1u : 0u, he = a.c.eos != TM_NONE ? 1u : 0u;
  T vals[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    if (k < cnt) {
      const uint32_t j = c - p.lo;                     // (wraps to a large number left of the entries)
      int32_t v = a.ignore;
      if (j >= hb && j < p.len - he && j < p.len) v = a.labels[p.src + (j - hb)];
      vals[k] = (T)v;                                  // (T is signed: an 8-byte label keeps its sign)
      if (++c == L && k + 1 < cnt) { c = 0; r++; p = row_plan(a.c, r); }
    } else {
      vals[k] = 0;
    }
  }
  flat_store<T>(out, e0, cnt, vals);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
// the batch's region buffer, in 4-byte words, every part on a 16-byte boundary: the count of regions out of order | the documents' lengths [ndocs] |
// the token ranges the atomics work on [2 * nreg] | the ragged labels of the collated form
struct RegionBuf { uint32_t* bad; uint32_t* doc_len; uint32_t* rtok; int32_t* labels; };
static uint64_t up4(uint64_t words) { return (words + 3u) & ~3ull; }
static int region_reserve(tm_batch* b, uint64_t nreg, uint64_t labels, RegionBuf& rb) {
  const uint64_t need = 4u + up4(b->ndocs) + up4(2u * nreg) + labels;
  const int rc = grow_batch(b, (void**)&b->d_region, &b->region_cap, need, need + need / 4 + 1024, 4, "region labels");
  rb.bad = b->d_region;
  rb.doc_len = rb.bad + 4;
  rb.rtok = rb.doc_len + up4(b->ndocs);
  rb.labels = reinterpret_cast<int32_t*>(rb.rtok + up4(2u * nreg));
  return rc;
}

static int region_args(const tm_batch* b, const tm_regions* rg, uint32_t label_bytes, const char* who) {
  if (!b || !rg) return set_error(TM_E_INVALID, "%s: null argument", who);
  int rc = units_args(rg->text, rg->unit, who);
  if (rc != TM_OK || (rc = spans_ready(b, who)) != TM_OK || (rg->text == TM_TEXT_RAW && (rc = origin_ready(b, who)) != TM_OK)) return rc;
  if (label_bytes != 4 && label_bytes != 8) return set_error(TM_E_INVALID, "%s: label_bytes %u (4 or 8)", who, label_bytes);
  if (b->ndocs && (!rg->reg_offsets || reinterpret_cast<uintptr_t>(rg->reg_offsets) % 8 || reinterpret_cast<uintptr_t>(rg->regions) % 4))
    return set_error(TM_E_INVALID, "%s: reg_offsets (8-byte aligned) and regions (4-byte aligned) must be given", who);
  return TM_OK;
}

// The whole of a call behind its checks, on `st`: the number of regions read back where the token ranges or the count of regions out of order are asked
// for (the one wait of the call), the batch's buffer grown for them, the pairs of the regions' text and unit into the batch's span buffer, the documents'
// lengths, the labels of all `total` ids into `out`, the token ranges and the count.  out null (T = int32_t, the collated form): the labels go to the
// batch's own buffer, *own says where.
template <typename T>
static int region_labels_on(tm_batch* b, hipStream_t st, const tm_regions* rg, T* out, uint64_t total, uint32_t* rtok_out, uint32_t* bad_out,
                            uint32_t* host_docs, int32_t** own = nullptr) {
  int rc = TM_OK;
  uint64_t nreg = 0;
  const bool sweep = rtok_out || bad_out;
  if (sweep && ((rc = small_d2h(b, &nreg, rg->reg_offsets + b->ndocs, 8, st)) != TM_OK || (rc = small_sync(b, st)) != TM_OK)) return rc;
  RegionBuf rb;
  if ((rc = region_reserve(b, rtok_out ? nreg : 0, out ? 0 : total, rb)) != TM_OK) return rc;
  if (!out) out = reinterpret_cast<T*>(rb.labels);
  if (own) *own = rb.labels;
  if (total && ((rc = batch_own_spans_on(b, st, rg->text, rg->unit, total, host_docs)) != TM_OK || (rc = batch_doc_units_on(b, st, rg->text, rg->unit, rb.doc_len)) != TM_OK)) return rc;
  (void)hipGetLastError();
  if (bad_out) TM_LAUNCH(k_region_clear, 1, 1, 0, st, rb.bad);
  if (sweep && nreg) TM_LAUNCH(k_region_init, grid_of(nreg), 256, 0, st, rg->reg_offsets, b->ndocs, rg->regions, nreg, rtok_out ? rb.rtok : nullptr, bad_out ? rb.bad : nullptr);
  if (total) {
    const RegionArgs a{reinterpret_cast<const uint32_t*>(b->d_spans), b->d_tok_offsets, rg->reg_offsets, rg->regions, rb.doc_len, rtok_out ? rb.rtok : nullptr, total, b->ndocs,
                       reinterpret_cast<uintptr_t>(out) % 16 ? 0u : 1u, rg->ignore_label};
    const auto kern = k_region_labels<T>;
    TM_LAUNCH(kern, (uint32_t)((total + RG_TILE - 1) / RG_TILE), 64, 0, st, a, out);
  }
  if (sweep) TM_LAUNCH(k_region_finish, grid_of(std::max<uint64_t>(nreg, 1)), 256, 0, st, rb.rtok, nreg, rtok_out, rb.bad, bad_out);
  return launch_check();
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_region_labels(tm_batch* b, void* stream, const tm_regions* rg, void* labels_out, uint32_t label_bytes, uint64_t labels_cap, uint32_t* region_tokens_out,
                           uint32_t* bad_out, uint32_t* host_docs) {
  const char* who = "tm_batch_region_labels";
  if (host_docs) *host_docs = 0;
  int rc = region_args(b, rg, label_bytes, who);
  if (rc != TM_OK) return rc;
  if (reinterpret_cast<uintptr_t>(labels_out) % label_bytes || reinterpret_cast<uintptr_t>(region_tokens_out) % 4)
    return set_error(TM_E_INVALID, "%s: labels_out or region_tokens_out not aligned to its elements", who);
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the rows are all there)
  if (b->ndocs == 0) return TM_OK;
  const uint64_t total = b->last_totals[1];
  if (total > labels_cap) return set_error(TM_E_NOSPACE, "%s: labels_cap %llu < %llu ids", who, (unsigned long long)labels_cap, (unsigned long long)total);
  if (!labels_out) return set_error(TM_E_INVALID, "%s: null argument", who);
  if ((rc = spans_check_lengths(b, who)) != TM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  return label_bytes == 4 ? region_labels_on(b, st, rg, static_cast<int32_t*>(labels_out), total, region_tokens_out, bad_out, host_docs)
                          : region_labels_on(b, st, rg, static_cast<int64_t*>(labels_out), total, region_tokens_out, bad_out, host_docs);
}

int tm_batch_collate_region_labels(tm_batch* b, const tm_collate* how, void* stream, const tm_regions* rg, void* labels_out, uint32_t label_bytes, uint32_t* bad_out) {
  const char* who = "tm_batch_collate_region_labels";
  int rc = check_how(b, how, labels_out, who);
  if (rc != TM_OK || (rc = region_args(b, rg, label_bytes, who)) != TM_OK) return rc;
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + (how->eos_id != TM_NONE ? 1u : 0u);
  if ((rc = check_row_room(who, how->row_len, ns, how->ndocs, "documents")) != TM_OK) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the rows are all there)
  if (how->ndocs == 0) return TM_OK;
  const uint64_t total = b->last_totals[1];
  if ((rc = spans_check_lengths(b, who)) != TM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  int32_t* ragged = nullptr;
  if ((rc = region_labels_on<int32_t>(b, st, rg, nullptr, total, nullptr, bad_out, nullptr, &ragged)) != TM_OK) return rc;
  (void)hipGetLastError();
  const LabelRows a{CollateArgs{nullptr, b->d_tok_offsets + how->first_doc, how->ndocs, how->row_len, 0u, how->bos_id != TM_NONE ? 0u : TM_NONE,
                                how->eos_id != TM_NONE ? 0u : TM_NONE, how->flags},
                    ragged, rg->ignore_label};
  with_wide_type<int32_t, int64_t>(label_bytes, [&](auto z) {
    using T = decltype(z);
    launch_flat(k_collate_labels<T>, st, static_cast<T*>(labels_out), (uint64_t)a.c.rows * a.c.L, 0, a, static_cast<T*>(labels_out));
  });
  return launch_check();
}

}  // extern "C"

// tm_collate.h - what the fixed-shape outputs share (tm_collate.hip: ids, masks, streams; tm_windows.hip: overlapping windows; tm_spans.hip: the
// spans of the ids in either layout): an output as one flat run of elements with 16-byte stores between an unaligned head and tail, the plan of a
// row of tm_batch_collate and of tm_batch_windows, the ONE fill body each for ids / mask and for pairs that both layouts' kernels call with their
// plan, the searches from an id or a stream position to its document, and two documents per row (tm_pairs.hip): its plan and its fill bodies.
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

// ---- the fill of rows: what k_collate_rows / k_window_rows and k_collate_spans / k_window_spans do with work-item t ------------------------------
// Args: CollateArgs or WindowArgs (L, pad, bos, eos, ids); plan(r): the RowPlan of row r - row_plan, or win_plan's.  The row of the work-item's
// first element is a division; when its vector crosses a row end the next row's plan is asked for.
// MASK: the element is 1 inside the row's entries and 0 on padding (T = uint8_t); else the id.
template <typename T, bool MASK, typename Args, typename Plan>
__device__ __forceinline__ void fill_rows(const Args& a, const Flat& f, T* __restrict__ out, uint64_t t, Plan plan) {
  constexpr uint32_t PER = 16 / sizeof(T);
  uint64_t e0;
  uint32_t cnt;
  if (!flat_span<T>(f, t, e0, cnt)) return;
  uint64_t r;
  uint32_t c;
  if (f.n <= 0xFFFFFFFFull) { r = (uint32_t)e0 / a.L; c = (uint32_t)e0 - (uint32_t)r * a.L; }      // (a 64-bit division costs more than the store it is for)
  else { r = e0 / a.L; c = (uint32_t)(e0 - r * a.L); }
  RowPlan p = plan(r);                                 // (r is a row: e0 is an element of the output)
  const uint32_t hb = a.bos != TM_NONE ? 1u : 0u;
  T vals[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    if (k < cnt) {
      const uint32_t j = c - p.lo;                     // (wraps to a large number left of the entries)
      uint32_t v;
      if (MASK) v = j < p.len ? 1u : 0u;
      else if (j >= p.len) v = a.pad;
      else if (hb && j == 0) v = a.bos;
      else if (a.eos != TM_NONE && j == p.len - 1) v = a.eos;
      else v = a.ids[p.src + (j - hb)];
      vals[k] = (T)v;
      if (++c == a.L && k + 1 < cnt) { c = 0; r++; p = plan(r); }      // (another element follows: r is a row)
    } else {
      vals[k] = 0;
    }
  }
  flat_store<T>(out, e0, cnt, vals);
}
// The pairs of the ids laid out like the rows: the output [rows, L, 2] is one flat run of 2 * rows * L elements of T, element e is component
// e & 1 of column (e >> 1) % L of row (e >> 1) / L.  A column that holds a content id gets that id's pair; BOS, EOS and padding get (0, 0).
template <typename T, typename Args, typename Plan>
__device__ __forceinline__ void fill_spans(const Args& a, const Flat& f, const uint32_t* __restrict__ spans, T* __restrict__ out, uint64_t t, Plan plan) {
  constexpr uint32_t PER = 16 / sizeof(T);
  uint64_t e0;
  uint32_t cnt;
  if (!flat_span<T>(f, t, e0, cnt)) return;
  const uint64_t L2 = 2ull * a.L;
  uint64_t r;
  uint64_t c;                                         // element of the row: 2 * column + component
  if (f.n <= 0xFFFFFFFFull && L2 <= 0xFFFFFFFFull) { r = (uint32_t)e0 / (uint32_t)L2; c = (uint32_t)e0 - (uint32_t)r * (uint32_t)L2; }
  else { r = e0 / L2; c = e0 - r * L2; }
  RowPlan p = plan(r);
  const uint32_t hb = a.bos != TM_NONE ? 1u : 0u;
  T vals[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    if (k < cnt) {
      const uint32_t j = (uint32_t)(c >> 1) - p.lo;      // (wraps to a large number left of the entries)
      uint32_t v = 0;
      if (j < p.len && !(hb && j == 0) && !(a.eos != TM_NONE && j == p.len - 1)) v = spans[2 * (p.src + (j - hb)) + (c & 1u)];
      vals[k] = (T)v;
      if (++c == L2 && k + 1 < cnt) { c = 0; r++; p = plan(r); }
    } else {
      vals[k] = 0;
    }
  }
  flat_store<T>(out, e0, cnt, vals);
}

// ---- an id of a run -> its document ----------------------------------------------------------------------------------------------------------------
// the last document whose first id is not behind id t, over tok_offsets[0 .. ndocs) (documents without ids share their offset with the next)
__device__ __forceinline__ uint32_t doc_of_id(const uint64_t* __restrict__ tok_offsets, uint32_t ndocs, uint64_t t) {
  uint32_t lo = 0, hi = ndocs;
  while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (tok_offsets[mid] <= t) lo = mid; else hi = mid; }
  return lo;
}

// ---- a position of a stream of documents -> its document ---------------------------------------------------------------------------------------------
// key(d) = toff[d] - toff[0] + d * sep: where document d begins in the stream (sep = 1: every document is followed by a separator).  The
// cursor holds the document d with key(d) <= p < key(d + 1) - for an empty document without separator there is no such p, it vanishes.
struct DocCursor {
  const uint64_t* toff;
  uint32_t nd, sep, d;
  uint64_t base, next;        // key(d), key(d + 1)
  __device__ __forceinline__ uint64_t key(uint32_t k) const { return toff[k] - toff[0] + (uint64_t)k * sep; }
  // p < key(nd) and key(from) <= p
  __device__ __forceinline__ void seek(uint64_t p, uint32_t from) {
    uint32_t lo = from, hi = nd;      // invariant: key(lo) <= p < key(hi)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (key(mid) <= p) lo = mid; else hi = mid;
    }
    d = lo; base = key(lo); next = key(lo + 1);
  }
  // the next position asked for is >= the last one: stay, or search the documents behind (never a walk: a run of empty documents is legal)
  __device__ __forceinline__ void advance(uint64_t p) { if (p >= next) seek(p, d + 1); }
};

// ---- overlapping windows of a document as rows (tm_batch_windows, tm_batch_windows_spans: tm_windows.hip) -------------------------------------
// room = L - specials content ids per row, consecutive rows of a document step = room - overlap ids apart.  win_off[d]: the first row of
// document d (a scan of the windows per document); row_doc[r]: the document of row r (a search over win_off, once per row).
struct WindowArgs {
  const uint32_t* ids;        // the batch's ids
  const uint64_t* toff;       // tok_offsets + first_doc
  const uint64_t* win_off;    // [nd + 1]
  const uint32_t* row_doc;    // [rows]
  uint64_t rows;              // win_off[nd]
  uint32_t nd, L, room, step, pad, bos, eos, flags;      // bos / eos: TM_NONE = none
};
// windows of a document of n ids: one if it fits (an empty document too), else one more for every `step` ids, or part of them, beyond `room`
__host__ __device__ __forceinline__ uint64_t window_count(uint64_t n, uint32_t room, uint32_t step) {
  return n <= room ? 1u : 1u + (n - room + step - 1) / step;
}
// what row r holds: RowPlan as above, its document and the index of its first content id inside the document
struct WinPlan { RowPlan p; uint64_t start; uint32_t d; };
__device__ __forceinline__ WinPlan win_plan(const WindowArgs& a, uint64_t r) {
  WinPlan w;
  w.d = a.row_doc[r];
  const uint64_t b0 = a.toff[w.d], n = a.toff[w.d + 1] - b0;
  const uint32_t ns = (a.bos != TM_NONE ? 1u : 0u) + (a.eos != TM_NONE ? 1u : 0u);
  w.start = (r - a.win_off[w.d]) * a.step;           // (<= n - 1 for every window but an empty document's only one)
  const uint32_t m = (uint32_t)std::min<uint64_t>(n - w.start, a.room);
  w.p.src = b0 + w.start;
  w.p.len = m + ns;
  w.p.lo = (a.flags & TM_COLLATE_PAD_LEFT) ? a.L - w.p.len : 0u;
  return w;
}

// ---- two documents per row (tm_batch_pair, tm_batch_pair_windows and their spans: tm_pairs.hip) --------------------------------------------------
// [bos] A [sep]*nsep B [eos]: pair p is the documents toff_a[p], toff_b[p] of one run.  R = L - specials: the content ids a row holds.  The
// window form (win_off, row_doc as in WindowArgs, per PAIR): A cut to max_first in every row of the pair, B slides.
struct PairArgs {
  const uint32_t* ids;        // the batch's ids
  const uint64_t* toff_a;     // tok_offsets + first_a
  const uint64_t* toff_b;     // tok_offsets + first_b
  const uint64_t* win_off;    // [np + 1]        (windows only)
  const uint32_t* row_doc;    // [rows]          (windows only)
  uint64_t rows;              // np, or win_off[np]
  uint32_t np, L, R, pad, bos, sep, eos, nsep, trunc, max_first, overlap, flags;      // bos / sep / eos: TM_NONE = none
};
// what of a ids of A and b ids of B a row with room for R keeps (the rule: tokenmonster_hip.h; LONGEST_FIRST in closed form)
struct PairKept { uint32_t a, b; };
__host__ __device__ __forceinline__ PairKept pair_kept(uint64_t a, uint64_t b, uint32_t R, uint32_t trunc) {
  if (a + b <= R) return PairKept{(uint32_t)a, (uint32_t)b};
  PairKept k;
  if (trunc == TM_PAIR_ONLY_SECOND) { k.a = (uint32_t)std::min<uint64_t>(a, R); k.b = (uint32_t)std::min<uint64_t>(b, R - k.a); return k; }
  if (trunc == TM_PAIR_ONLY_FIRST) { k.b = (uint32_t)std::min<uint64_t>(b, R); k.a = (uint32_t)std::min<uint64_t>(a, R - k.b); return k; }
  const uint32_t h = R / 2;
  if (a <= h) { k.a = (uint32_t)a; k.b = R - k.a; }
  else if (b <= R - h) { k.b = (uint32_t)b; k.a = R - k.b; }
  else { k.a = h; k.b = R - h; }
  return k;
}
// what a row holds: `len` entries [bos?] A[0..na) [sep]*nsep B[0..nb) [eos?] from column `lo` on, A from ids[src_a], B from ids[src_b]
struct PairPlan { uint64_t src_a, src_b; uint32_t lo, na, nb, len; };
__device__ __forceinline__ uint32_t pair_specials(const PairArgs& a) { return (a.bos != TM_NONE ? 1u : 0u) + a.nsep + (a.eos != TM_NONE ? 1u : 0u); }
__device__ __forceinline__ PairPlan pair_plan(const PairArgs& a, uint64_t r) {
  const uint64_t a0 = a.toff_a[r], a1 = a.toff_a[r + 1], b0 = a.toff_b[r], b1 = a.toff_b[r + 1];
  const PairKept k = pair_kept(a1 - a0, b1 - b0, a.R, a.trunc);
  PairPlan p;
  p.src_a = a0; p.src_b = b0;
  p.na = k.a; p.nb = k.b;
  p.len = k.a + k.b + pair_specials(a);
  p.lo = (a.flags & TM_COLLATE_PAD_LEFT) ? a.L - p.len : 0u;
  return p;
}
// the same for row r of the window form, with its pair and the index inside B of its first id
struct PairWinPlan { PairPlan p; uint64_t start; uint32_t pair; };
__device__ __forceinline__ PairWinPlan pair_win_plan(const PairArgs& a, uint64_t r) {
  PairWinPlan w;
  w.pair = a.row_doc[r];
  const uint64_t a0 = a.toff_a[w.pair], a1 = a.toff_a[w.pair + 1], b0 = a.toff_b[w.pair], b1 = a.toff_b[w.pair + 1];
  w.p.na = (uint32_t)std::min<uint64_t>(a1 - a0, a.max_first);
  const uint32_t room = a.R - w.p.na;                  // (> overlap: max_first < R - overlap, checked by the host)
  w.start = (r - a.win_off[w.pair]) * (room - a.overlap);      // (<= b - 1 for every window but an empty B's only one)
  w.p.nb = (uint32_t)std::min<uint64_t>(b1 - b0 - w.start, room);
  w.p.src_a = a0; w.p.src_b = b0 + w.start;
  w.p.len = w.p.na + w.p.nb + pair_specials(a);
  w.p.lo = (a.flags & TM_COLLATE_PAD_LEFT) ? a.L - w.p.len : 0u;
  return w;
}

// The fill of pair rows: fill_rows above with a PairPlan.  plan(r): pair_plan, or pair_win_plan's.  A column's value follows from its offset
// j = c - lo inside the entries and the boundaries bos | A | separators | B | eos.
// WHAT: 0 = the id (T of 2, 4 or 8 bytes); 1 = the mask, 1 on an entry; 2 = the type, 1 on B's ids and eos (T = uint8_t)
template <typename T, int WHAT, typename Plan>
__device__ __forceinline__ void fill_pair_rows(const PairArgs& a, const Flat& f, T* __restrict__ out, uint64_t t, Plan plan) {
  constexpr uint32_t PER = 16 / sizeof(T);
  uint64_t e0;
  uint32_t cnt;
  if (!flat_span<T>(f, t, e0, cnt)) return;
  uint64_t r;
  uint32_t c;
  if (f.n <= 0xFFFFFFFFull) { r = (uint32_t)e0 / a.L; c = (uint32_t)e0 - (uint32_t)r * a.L; }      // (a 64-bit division costs more than the store it is for)
  else { r = e0 / a.L; c = (uint32_t)(e0 - r * a.L); }
  PairPlan p = plan(r);                                // (r is a row: e0 is an element of the output)
  const uint32_t hb = a.bos != TM_NONE ? 1u : 0u;
  T vals[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    if (k < cnt) {
      const uint32_t j = c - p.lo;                     // (wraps to a large number left of the entries)
      const uint32_t ea = hb + p.na, eb = ea + a.nsep; // (the ends of A and of the separators)
      uint32_t v;
      if (WHAT == 1) v = j < p.len ? 1u : 0u;
      else if (WHAT == 2) v = (j >= eb && j < p.len) ? 1u : 0u;
      else if (j >= p.len) v = a.pad;
      else if (j < hb) v = a.bos;
      else if (j < ea) v = a.ids[p.src_a + (j - hb)];
      else if (j < eb) v = a.sep;
      else if (j < eb + p.nb) v = a.ids[p.src_b + (j - eb)];
      else v = a.eos;
      vals[k] = (T)v;
      if (++c == a.L && k + 1 < cnt) { c = 0; r++; p = plan(r); }      // (another element follows: r is a row)
    } else {
      vals[k] = 0;
    }
  }
  flat_store<T>(out, e0, cnt, vals);
}
// The pairs of the ids laid out like the pair rows (the flat output of fill_spans): a content column of either side gets its id's pair, which
// counts from that side's own document; specials and padding get (0, 0).
template <typename T, typename Plan>
__device__ __forceinline__ void fill_pair_spans(const PairArgs& a, const Flat& f, const uint32_t* __restrict__ spans, T* __restrict__ out, uint64_t t, Plan plan) {
  constexpr uint32_t PER = 16 / sizeof(T);
  uint64_t e0;
  uint32_t cnt;
  if (!flat_span<T>(f, t, e0, cnt)) return;
  const uint64_t L2 = 2ull * a.L;
  uint64_t r;
  uint64_t c;                                         // element of the row: 2 * column + component
  if (f.n <= 0xFFFFFFFFull && L2 <= 0xFFFFFFFFull) { r = (uint32_t)e0 / (uint32_t)L2; c = (uint32_t)e0 - (uint32_t)r * (uint32_t)L2; }
  else { r = e0 / L2; c = e0 - r * L2; }
  PairPlan p = plan(r);
  const uint32_t hb = a.bos != TM_NONE ? 1u : 0u;
  T vals[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    if (k < cnt) {
      const uint32_t j = (uint32_t)(c >> 1) - p.lo;      // (wraps to a large number left of the entries)
      const uint32_t ea = hb + p.na, eb = ea + a.nsep;
      uint32_t v = 0;
      if (j >= hb && j < ea) v = spans[2 * (p.src_a + (j - hb)) + (c & 1u)];
      else if (j >= eb && j < eb + p.nb) v = spans[2 * (p.src_b + (j - eb)) + (c & 1u)];
      vals[k] = (T)v;
      if (++c == L2 && k + 1 < cnt) { c = 0; r++; p = plan(r); }
    } else {
      vals[k] = 0;
    }
  }
  flat_store<T>(out, e0, cnt, vals);
}

constexpr uint64_t COLLATE_MAX_ELEMS = 1ull << 36;       // elements of one output: keeps every grid below 2^31 workgroups

inline uint32_t grid_of(uint64_t items) { return (uint32_t)((items + 255) / 256); }
inline int launch_check() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? TM_OK : hip_fail(e, "kernel launch");
}

// the arguments every layout shares (ids_out: only that it is there)
int check_how(const tm_batch* b, const tm_collate* how, const void* ids_out, const char* who);
// tm_spans.hip: no document of the run is 2^32 bytes or longer (offsets are 32 bits)
int spans_check_lengths(tm_batch* b, const char* who);
// tm_windows.hip: the batch's window buffer for nd documents (or pairs) - win_off[cap + 1] | block sums of the scan, its total behind them |
// windows per document - and the document of every row, a search over win_off, into the batch's d_win_rows on `st`
struct WinBuf { uint64_t* win_off; uint64_t* sums; uint64_t* total; uint32_t* counts; };
WinBuf win_buf(const tm_batch* b);
int win_reserve(tm_batch* b, uint32_t nd);
int win_row_docs(tm_batch* b, const uint64_t* win_off, uint32_t nd, uint64_t rows, hipStream_t st);

}  // namespace tmh

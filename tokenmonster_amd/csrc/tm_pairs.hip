// tm_pairs.hip — text pairs as fixed-shape rows: two documents of one run in a row, [bos] A [sep] B [eos] (tm_batch_pair), with the mask, the
// token types and the kept counts, the QA form in which A stands in every row and B slides (tm_batch_pair_windows), and the spans of the ids
// laid out the same way (tm_batch_pair_spans_in, tm_batch_pair_windows_spans_in).  The rule: include/tokenmonster_hip.h.
//
// Streaming kernels like tm_collate.hip's and tm_windows.hip's: no table, no LDS, the output one flat run of elements, one 16-byte vector per
// work-item.  The plan of a row is four token offsets (pair_plan, tm_collate.h) and the fill bodies are fill_pair_rows / fill_pair_spans
// there.  The window form counts the rows of every pair (k_pair_window_counts: the room for B differs from pair to pair, with the ids A keeps),
// and then goes the way of tm_windows.hip through the batch's window buffers: scan_u32 into win_off, the pair of every row once per row
// (k_window_row_docs), the fill with pair_win_plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "tm_pipeline.h"
#include "tm_collate.h"

namespace tmh {

// ---- k_pair_rows: one pair per row -------------------------------------------------------------------------------------------------------------
// The fill is fill_pair_rows (tm_collate.h) with the plan of one pair per row.  kept (ids launch only, may be null): the first `rows`
// work-items write a row's (a', b') each.
template <typename T, int WHAT>
__global__ __launch_bounds__(256) void k_pair_rows(PairArgs a, Flat f, T* __restrict__ out, uint32_t* __restrict__ kept) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (WHAT == 0 && kept && t < a.rows) {
    const PairPlan p = pair_plan(a, t);
    kept[2 * t] = p.na;
    kept[2 * t + 1] = p.nb;
  }
  fill_pair_rows<T, WHAT>(a, f, out, t, [&](uint64_t r) { return pair_plan(a, r); });
}

// ---- k_pair_spans: the pairs of the ids laid out like the rows ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_pair_spans(PairArgs a, Flat f, const uint32_t* __restrict__ spans, T* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  fill_pair_spans<T>(a, f, spans, out, t, [&](uint64_t r) { return pair_plan(a, r); });
}

// ---- k_pair_window_counts: the rows of every pair (k_window_counts with a room per pair) -------------------------------------------------------
__global__ __launch_bounds__(256) void k_pair_window_counts(const uint64_t* __restrict__ toff_a, const uint64_t* __restrict__ toff_b, uint32_t np, uint32_t R,
                                                            uint32_t max_first, uint32_t overlap, uint32_t* __restrict__ counts) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  const uint32_t room = R - (uint32_t)std::min<uint64_t>(toff_a[p + 1] - toff_a[p], max_first);      // (> overlap: checked by the host)
  // (32 bits for scan_u32, as in k_window_counts)
  counts[p] = (uint32_t)std::min<uint64_t>(window_count(toff_b[p + 1] - toff_b[p], room, room - overlap), 0xFFFFFFFFull);
}

// ---- k_pair_window_rows / k_pair_window_spans: the fills with the plan of a window -------------------------------------------------------------
// The per-row outputs (ids launch only, each may be null): the first `rows` work-items write a row's kept counts, pair and start each.
template <typename T, int WHAT>
__global__ __launch_bounds__(256) void k_pair_window_rows(PairArgs a, Flat f, T* __restrict__ out, uint32_t* __restrict__ kept, uint32_t* __restrict__ row_pair,
                                                          uint32_t* __restrict__ row_start) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (WHAT == 0 && (kept || row_pair || row_start) && t < a.rows) {
    const PairWinPlan w = pair_win_plan(a, t);
    if (kept) { kept[2 * t] = w.p.na; kept[2 * t + 1] = w.p.nb; }
    if (row_pair) row_pair[t] = w.pair;
    if (row_start) row_start[t] = (uint32_t)w.start;
  }
  fill_pair_rows<T, WHAT>(a, f, out, t, [&](uint64_t r) { return pair_win_plan(a, r).p; });
}
template <typename T>
__global__ __launch_bounds__(256) void k_pair_window_spans(PairArgs a, Flat f, const uint32_t* __restrict__ spans, T* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  fill_pair_spans<T>(a, f, spans, out, t, [&](uint64_t r) { return pair_win_plan(a, r).p; });
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
// the arguments every pair call shares (out: only that it is there); fills all of *a but the window fields
static int check_pair(const tm_batch* b, const tm_pair* how, const void* out, const char* who, PairArgs* a) {
  if (!b || !how || !out) return set_error(TM_E_INVALID, "%s: null argument", who);
  if (how->id_bytes != 2 && how->id_bytes != 4 && how->id_bytes != 8) return set_error(TM_E_INVALID, "%s: id_bytes %u (2, 4 or 8)", who, how->id_bytes);
  if (how->row_len == 0) return set_error(TM_E_INVALID, "%s: row_len 0", who);
  if (how->pad_id == TM_NONE) return set_error(TM_E_INVALID, "%s: pad_id must be given", who);
  if (how->flags & ~TM_COLLATE_PAD_LEFT)
    return set_error(TM_E_INVALID, "%s: flags %#x (TM_COLLATE_PAD_LEFT only: both sides keep their heads, no TM_COLLATE_KEEP_TAIL)", who, how->flags);
  if (how->truncation > TM_PAIR_ONLY_SECOND) return set_error(TM_E_INVALID, "%s: unknown truncation %u", who, how->truncation);
  if (how->sep_id == TM_NONE ? how->sep_count != 0 : (how->sep_count != 1 && how->sep_count != 2))
    return set_error(TM_E_INVALID, "%s: sep_count %u (1 or 2 with a sep_id, 0 without)", who, how->sep_count);
  if (how->id_bytes == 2) {
    if (b->vocab->host.n_ids > 65536u) return set_error(TM_E_INVALID, "%s: two-byte ids with a vocabulary of %u ids", who, b->vocab->host.n_ids);
    for (uint32_t s : {how->pad_id, how->bos_id, how->sep_id, how->eos_id})
      if (s != TM_NONE && s >= 65536u) return set_error(TM_E_INVALID, "%s: special id %u does not fit two bytes", who, s);
  }
  if (!b->has_output) return set_error(TM_E_INVALID, "%s: the batch holds no ids (no completed tm_batch_run or tm_batch_load_ids since the last upload)", who);
  for (uint32_t first : {how->first_a, how->first_b})
    if ((uint64_t)first + how->npairs > b->ndocs)
      return set_error(TM_E_INVALID, "%s: documents %u .. %llu of a run of %u", who, first, (unsigned long long)first + how->npairs, b->ndocs);
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + how->sep_count + (how->eos_id != TM_NONE ? 1u : 0u);
  if (how->row_len < ns) return set_error(TM_E_INVALID, "%s: row_len %u holds no %u specials", who, how->row_len, ns);
  *a = PairArgs{b->d_out, b->d_tok_offsets + how->first_a, b->d_tok_offsets + how->first_b, nullptr, nullptr, how->npairs, how->npairs, how->row_len,
                how->row_len - ns, how->pad_id, how->bos_id, how->sep_id, how->eos_id, how->sep_count, how->truncation, 0u, 0u, how->flags};
  return TM_OK;
}
// ... and of the span forms
static int check_pair_spans(const tm_batch* b, uint32_t text, uint32_t unit, uint32_t span_bytes, const char* who) {
  int rc = units_args(text, unit, who);
  if (rc != TM_OK) return rc;
  if (span_bytes != 4 && span_bytes != 8) return set_error(TM_E_INVALID, "%s: span_bytes %u (4 or 8)", who, span_bytes);
  if ((rc = spans_ready(b, who)) != TM_OK || (text == TM_TEXT_RAW && (rc = origin_ready(b, who)) != TM_OK)) return rc;
  return TM_OK;
}

template <typename T>
static void launch_pair_ids(const PairArgs& a, void* ids_out, uint32_t* kept_out, hipStream_t st) {
  const Flat f = flat_of(ids_out, a.rows * a.L, sizeof(T));
  const uint64_t items = std::max<uint64_t>(flat_items(f, sizeof(T)), kept_out ? a.rows : 0);
  const auto kern = k_pair_rows<T, 0>;
  TM_LAUNCH(kern, grid_of(items), 256, 0, st, a, f, static_cast<T*>(ids_out), kept_out);
}
template <typename T>
static void launch_pair_window_ids(const PairArgs& a, void* ids_out, uint32_t* kept_out, uint32_t* row_pair_out, uint32_t* row_start_out, hipStream_t st) {
  const Flat f = flat_of(ids_out, a.rows * a.L, sizeof(T));
  const uint64_t items = std::max<uint64_t>(flat_items(f, sizeof(T)), (kept_out || row_pair_out || row_start_out) ? a.rows : 0);
  const auto kern = k_pair_window_rows<T, 0>;
  TM_LAUNCH(kern, grid_of(items), 256, 0, st, a, f, static_cast<T*>(ids_out), kept_out, row_pair_out, row_start_out);
}
template <typename T>
static void launch_pair_spans(const PairArgs& a, bool windows, const uint32_t* spans, void* out, hipStream_t st) {
  const Flat f = flat_of(out, 2ull * a.rows * a.L, sizeof(T));
  const auto kern = windows ? k_pair_window_spans<T> : k_pair_spans<T>;
  TM_LAUNCH(kern, grid_of(flat_items(f, sizeof(T))), 256, 0, st, a, f, spans, static_cast<T*>(out));
}

// what the three window calls share: the arguments, the rows per pair and their scan on the stream of the batch's last run, and the number
// of rows read back from it (window_plan of tm_windows.hip, with a room per pair).  spans: the checks of the span form too
static int pair_window_plan(tm_batch* b, const tm_pair* how, uint32_t overlap, uint32_t max_first, const void* out, const char* who, bool spans, uint32_t text,
                            uint32_t unit, uint32_t span_bytes, PairArgs* a) {
  int rc = check_pair(b, how, out, who, a);
  if (rc != TM_OK) return rc;
  if (how->truncation != TM_PAIR_ONLY_SECOND) return set_error(TM_E_INVALID, "%s: truncation %u (pair windows cut the second side only: TM_PAIR_ONLY_SECOND)", who, how->truncation);
  if (max_first > a->R || a->R - max_first <= overlap)
    return set_error(TM_E_INVALID, "%s: max_first %u and overlap %u with room for %u ids per row (max_first + overlap < room)", who, max_first, overlap, a->R);
  if (spans && (rc = check_pair_spans(b, text, unit, span_bytes, who)) != TM_OK) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  a->max_first = max_first;
  a->overlap = overlap;
  a->rows = 0;
  if (how->npairs == 0) return TM_OK;
  if ((rc = win_reserve(b, how->npairs)) != TM_OK) return rc;
  const WinBuf w = win_buf(b);
  hipStream_t st = b->last_stream;
  (void)hipGetLastError();
  TM_LAUNCH(k_pair_window_counts, grid_of(how->npairs), 256, 0, st, a->toff_a, a->toff_b, how->npairs, a->R, max_first, overlap, w.counts);
  scan_u32(w.counts, how->npairs, w.sums, w.total, w.win_off, st);
  if ((rc = launch_check()) != TM_OK) return rc;
  if ((rc = small_d2h(b, &a->rows, w.win_off + how->npairs, 8, st)) != TM_OK || (rc = small_sync(b, st)) != TM_OK) return rc;
  a->win_off = w.win_off;
  if (a->rows * how->row_len > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "%s: %llu rows of %u ids in one call (split the pairs)", who, (unsigned long long)a->rows, how->row_len);
  return TM_OK;
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_pair(tm_batch* b, const tm_pair* how, void* stream, void* ids_out, uint8_t* mask_out, uint8_t* type_out, uint32_t* kept_out) {
  PairArgs a{};
  int rc = check_pair(b, how, ids_out, "tm_batch_pair", &a);
  if (rc != TM_OK) return rc;
  if ((uint64_t)how->npairs * how->row_len > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "tm_batch_pair: %u rows of %u ids in one call (split the pairs)", how->npairs, how->row_len);
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  if (how->npairs == 0) return TM_OK;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (how->id_bytes == 2) launch_pair_ids<uint16_t>(a, ids_out, kept_out, st);
  else if (how->id_bytes == 4) launch_pair_ids<uint32_t>(a, ids_out, kept_out, st);
  else launch_pair_ids<uint64_t>(a, ids_out, kept_out, st);
  if (mask_out) {
    const Flat f = flat_of(mask_out, a.rows * a.L, 1);
    const auto kern = k_pair_rows<uint8_t, 1>;
    TM_LAUNCH(kern, grid_of(flat_items(f, 1)), 256, 0, st, a, f, mask_out, (uint32_t*)nullptr);
  }
  if (type_out) {
    const Flat f = flat_of(type_out, a.rows * a.L, 1);
    const auto kern = k_pair_rows<uint8_t, 2>;
    TM_LAUNCH(kern, grid_of(flat_items(f, 1)), 256, 0, st, a, f, type_out, (uint32_t*)nullptr);
  }
  return launch_check();
}

int tm_batch_pair_spans_in(tm_batch* b, const tm_pair* how, void* stream, uint32_t text, uint32_t unit, void* spans_out, uint32_t span_bytes) {
  const char* who = "tm_batch_pair_spans_in";
  PairArgs a{};
  int rc = check_pair(b, how, spans_out, who, &a);
  if (rc != TM_OK || (rc = check_pair_spans(b, text, unit, span_bytes, who)) != TM_OK) return rc;
  if ((uint64_t)how->npairs * how->row_len > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "%s: %u rows of %u ids in one call (split the pairs)", who, how->npairs, how->row_len);
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the rows are all there)
  if (how->npairs == 0) return TM_OK;
  const uint64_t total = b->last_totals[1];
  hipStream_t st = (hipStream_t)stream;
  if ((rc = spans_check_lengths(b, who)) != TM_OK || (rc = batch_own_spans_on(b, st, text, unit, total)) != TM_OK) return rc;
  (void)hipGetLastError();
  a.ids = nullptr;
  if (span_bytes == 4) launch_pair_spans<uint32_t>(a, false, reinterpret_cast<const uint32_t*>(b->d_spans), spans_out, st);
  else launch_pair_spans<uint64_t>(a, false, reinterpret_cast<const uint32_t*>(b->d_spans), spans_out, st);
  return launch_check();
}

int tm_batch_pair_window_rows(tm_batch* b, const tm_pair* how, uint32_t overlap, uint32_t max_first, uint64_t* rows_needed) {
  if (!rows_needed) return set_error(TM_E_INVALID, "tm_batch_pair_window_rows: null argument");
  *rows_needed = 0;
  PairArgs a{};
  const int rc = pair_window_plan(b, how, overlap, max_first, rows_needed, "tm_batch_pair_window_rows", false, 0, 0, 0, &a);
  if (rc == TM_OK || rc == TM_E_LIMIT) *rows_needed = a.rows;
  return rc;
}

int tm_batch_pair_windows(tm_batch* b, const tm_pair* how, uint32_t overlap, uint32_t max_first, void* stream, uint64_t rows_cap, void* ids_out, uint8_t* mask_out,
                          uint8_t* type_out, uint32_t* kept_out, uint32_t* row_pair_out, uint32_t* row_start_out) {
  PairArgs a{};
  int rc = pair_window_plan(b, how, overlap, max_first, ids_out, "tm_batch_pair_windows", false, 0, 0, 0, &a);
  if (rc != TM_OK) return rc;
  if (a.rows > rows_cap) return set_error(TM_E_NOSPACE, "tm_batch_pair_windows: rows_cap %llu < %llu rows required", (unsigned long long)rows_cap, (unsigned long long)a.rows);
  if (a.rows == 0) return TM_OK;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = win_row_docs(b, a.win_off, a.np, a.rows, st)) != TM_OK) return rc;
  a.row_doc = b->d_win_rows;
  (void)hipGetLastError();
  if (how->id_bytes == 2) launch_pair_window_ids<uint16_t>(a, ids_out, kept_out, row_pair_out, row_start_out, st);
  else if (how->id_bytes == 4) launch_pair_window_ids<uint32_t>(a, ids_out, kept_out, row_pair_out, row_start_out, st);
  else launch_pair_window_ids<uint64_t>(a, ids_out, kept_out, row_pair_out, row_start_out, st);
  if (mask_out) {
    const Flat f = flat_of(mask_out, a.rows * a.L, 1);
    const auto kern = k_pair_window_rows<uint8_t, 1>;
    TM_LAUNCH(kern, grid_of(flat_items(f, 1)), 256, 0, st, a, f, mask_out, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
  }
  if (type_out) {
    const Flat f = flat_of(type_out, a.rows * a.L, 1);
    const auto kern = k_pair_window_rows<uint8_t, 2>;
    TM_LAUNCH(kern, grid_of(flat_items(f, 1)), 256, 0, st, a, f, type_out, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
  }
  return launch_check();
}

int tm_batch_pair_windows_spans_in(tm_batch* b, const tm_pair* how, uint32_t overlap, uint32_t max_first, void* stream, uint64_t rows_cap, uint32_t text, uint32_t unit,
                                   void* spans_out, uint32_t span_bytes) {
  const char* who = "tm_batch_pair_windows_spans_in";
  PairArgs a{};
  int rc = pair_window_plan(b, how, overlap, max_first, spans_out, who, true, text, unit, span_bytes, &a);
  if (rc != TM_OK) return rc;
  if (a.rows > rows_cap) return set_error(TM_E_NOSPACE, "%s: rows_cap %llu < %llu rows required", who, (unsigned long long)rows_cap, (unsigned long long)a.rows);
  if (a.rows == 0) return TM_OK;
  const uint64_t total = b->last_totals[1];
  hipStream_t st = (hipStream_t)stream;
  if ((rc = spans_check_lengths(b, who)) != TM_OK || (rc = batch_own_spans_on(b, st, text, unit, total)) != TM_OK) return rc;
  if ((rc = win_row_docs(b, a.win_off, a.np, a.rows, st)) != TM_OK) return rc;
  a.row_doc = b->d_win_rows;
  (void)hipGetLastError();
  a.ids = nullptr;
  if (span_bytes == 4) launch_pair_spans<uint32_t>(a, true, reinterpret_cast<const uint32_t*>(b->d_spans), spans_out, st);
  else launch_pair_spans<uint64_t>(a, true, reinterpret_cast<const uint32_t*>(b->d_spans), spans_out, st);
  return launch_check();
}

}  // extern "C"

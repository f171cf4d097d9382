// tm_windows.hip — sliding windows: the ragged ids a batch holds as rows [rows, L] in which a document longer than a row takes several rows
// and consecutive rows of a document share `overlap` ids (tm_batch_windows), with the row -> document map, and the byte spans of the ids laid
// out the same way (tm_batch_windows_spans, tm_batch_windows_raw_spans).  The rule: include/tokenmonster_hip.h.
//
// Four steps: the windows of every document from two token offsets (k_window_counts), their scan into win_off (scan_u32; the host reads
// win_off[nd], the number of rows), the document of every row - a binary search over win_off, a DocCursor with win_off as its keys, once per
// ROW (k_window_row_docs) - and the fill: the fill bodies tm_collate.hip's kernels run (fill_rows / fill_spans, tm_collate.h: no table, no LDS,
// the output one flat run of elements, one 16-byte vector per work-item), here with the plan of a window.  The row of a work-item's first
// element is a division, the row's document one load; when the vector crosses a row end the next row's document is looked up the same way - the
// next window of the document, or any number of documents on.  (One search per row, not one per 16-byte vector in the fill, where its
// dependent loads stood in front of every store: the measured pair is in DESIGN.md, section 4c.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "tm_pipeline.h"
#include "tm_collate.h"

namespace tmh {

// ---- k_window_counts: w(n) of every document ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window_counts(const uint64_t* __restrict__ toff, uint32_t nd, uint32_t room, uint32_t step, uint32_t* __restrict__ counts) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= nd) return;
  // (a count is 32 bits wide for scan_u32.  One that does not fit takes a document of more than 2^32 ids, and a document is shorter than
  // 2^32 bytes wherever its ids come from a walk: not reachable today.  Were it reached, the clamped count would disagree with win_plan.)
  counts[d] = (uint32_t)std::min<uint64_t>(window_count(toff[d + 1] - toff[d], room, step), 0xFFFFFFFFull);
}

// ---- k_window_row_docs: the document of every row ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window_row_docs(const uint64_t* __restrict__ win_off, uint32_t nd, uint64_t rows, uint32_t* __restrict__ row_doc) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  DocCursor cur{win_off, nd, 0u, 0, 0, 0};
  cur.seek(r, 0);                                      // (r < rows = key(nd))
  row_doc[r] = cur.d;
}

// ---- k_window_rows: the ids (or the mask) of the rows ------------------------------------------------------------------------------------------
// The fill is fill_rows (tm_collate.h) with the plan of a window.  The per-row outputs (ids launch only, each may be null): the first `rows`
// work-items write a row's length, document and start each.
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void k_window_rows(WindowArgs a, Flat f, T* __restrict__ out, uint32_t* __restrict__ lengths, uint32_t* __restrict__ row_doc,
                                                     uint32_t* __restrict__ row_start) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!MASK && (lengths || row_doc || row_start) && t < a.rows) {
    const WinPlan w = win_plan(a, t);
    if (lengths) lengths[t] = w.p.len;
    if (row_doc) row_doc[t] = w.d;
    if (row_start) row_start[t] = (uint32_t)w.start;
  }
  fill_rows<T, MASK>(a, f, out, t, [&](uint64_t r) { return win_plan(a, r).p; });
}

// ---- k_window_spans: the pairs of the ids laid out like the rows (fill_spans, tm_collate.h, with the plan of a window) ------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_window_spans(WindowArgs a, Flat f, const uint32_t* __restrict__ spans, T* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  fill_spans<T>(a, f, spans, out, t, [&](uint64_t r) { return win_plan(a, r).p; });
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
// the batch's window buffer for nd documents: win_off[cap + 1] | block sums of the scan, its total behind them | windows per document (WinBuf: tm_collate.h)
static uint64_t win_sum_words(uint32_t cap) { return ((uint64_t)cap + 1 + SCAN_CH - 1) / SCAN_CH + 1; }
WinBuf win_buf(const tm_batch* b) {
  WinBuf w;
  w.win_off = reinterpret_cast<uint64_t*>(b->d_win);
  w.sums = w.win_off + (uint64_t)b->win_cap + 1;
  w.total = w.sums + win_sum_words(b->win_cap) - 1;
  w.counts = reinterpret_cast<uint32_t*>(w.total + 1);
  return w;
}
int win_reserve(tm_batch* b, uint32_t nd) {
  if (b->d_win && nd <= b->win_cap) return TM_OK;
  auto bytes = [](uint32_t cap) { return ((uint64_t)cap + 1 + win_sum_words(cap)) * 8 + (uint64_t)cap * 4; };
  const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)nd + nd / 4 + 1024, 0xFFFFFFFFull);
  const uint64_t old_bytes = b->d_win ? bytes(b->win_cap) : 0;
  b->win_cap = 0;
  const int rc = batch_replace(b, (void**)&b->d_win, old_bytes, bytes(nd), bytes(cap), "windows");
  if (rc == TM_OK) b->win_cap = cap;
  return rc;
}

// what the four calls share: the arguments, the rows per document and their scan on the stream of the batch's last run, and the number of
// rows read back from it (synchronizes like tm_batch_totals).  spans: 0 = an ids call, 1 = normalized spans, 2 = raw spans.
static int window_plan(tm_batch* b, const tm_collate* how, uint32_t overlap, const void* out, const char* who, int spans, uint32_t span_bytes, WindowArgs* a) {
  int rc = check_how(b, how, out, who);
  if (rc != TM_OK) return rc;
  if (how->flags & TM_COLLATE_KEEP_TAIL) return set_error(TM_E_INVALID, "%s: TM_COLLATE_KEEP_TAIL has no meaning for windows (every id is kept)", who);
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + (how->eos_id != TM_NONE ? 1u : 0u);
  if (how->row_len <= ns) return set_error(TM_E_INVALID, "%s: row_len %u leaves no room beside %u specials", who, how->row_len, ns);
  const uint32_t room = how->row_len - ns;
  if (overlap >= room) return set_error(TM_E_INVALID, "%s: overlap %u with room for %u ids per row (overlap < room)", who, overlap, room);
  if (spans) {
    if (span_bytes != 4 && span_bytes != 8) return set_error(TM_E_INVALID, "%s: span_bytes %u (4 or 8)", who, span_bytes);
    if ((rc = spans_ready(b, who)) != TM_OK || (spans == 2 && (rc = origin_ready(b, who)) != TM_OK)) return rc;
  }
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  *a = WindowArgs{b->d_out, b->d_tok_offsets + how->first_doc, nullptr, nullptr, 0, how->ndocs, how->row_len, room, room - overlap, how->pad_id, how->bos_id, how->eos_id, how->flags};
  if (how->ndocs == 0) return TM_OK;
  if ((rc = win_reserve(b, how->ndocs)) != TM_OK) return rc;
  const WinBuf w = win_buf(b);
  hipStream_t st = b->last_stream;
  (void)hipGetLastError();
  TM_LAUNCH(k_window_counts, grid_of(how->ndocs), 256, 0, st, a->toff, how->ndocs, a->room, a->step, w.counts);
  scan_u32(w.counts, how->ndocs, w.sums, w.total, w.win_off, st);      // (block sums and total into the window buffer: d_scan_tmp and d_totals belong to the run)
  if ((rc = launch_check()) != TM_OK) return rc;
  if ((rc = small_d2h(b, &a->rows, w.win_off + how->ndocs, 8, st)) != TM_OK || (rc = small_sync(b, st)) != TM_OK) return rc;
  a->win_off = w.win_off;
  if (a->rows * how->row_len > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "%s: %llu rows of %u ids in one call (split the documents)", who, (unsigned long long)a->rows, how->row_len);
  return TM_OK;
}

// the document of every row into the batch's own buffer, on the stream of the fill behind it
int win_row_docs(tm_batch* b, const uint64_t* win_off, uint32_t nd, uint64_t rows, hipStream_t st) {
  const int rc = grow_batch(b, (void**)&b->d_win_rows, &b->win_rows_cap, rows, rows + rows / 4 + 1024, 4, "window rows");
  if (rc != TM_OK) return rc;
  (void)hipGetLastError();
  TM_LAUNCH(k_window_row_docs, grid_of(rows), 256, 0, st, win_off, nd, rows, b->d_win_rows);
  return launch_check();
}
static int window_row_docs(tm_batch* b, WindowArgs* a, hipStream_t st) {
  const int rc = win_row_docs(b, a->win_off, a->nd, a->rows, st);
  a->row_doc = b->d_win_rows;
  return rc;
}

template <typename T>
static void launch_window_ids(const WindowArgs& a, void* ids_out, uint32_t* lengths_out, uint32_t* row_doc_out, uint32_t* row_start_out, hipStream_t st) {
  const Flat f = flat_of(ids_out, a.rows * a.L, sizeof(T));
  const uint64_t items = std::max<uint64_t>(flat_items(f, sizeof(T)), (lengths_out || row_doc_out || row_start_out) ? a.rows : 0);
  const auto kern = k_window_rows<T, false>;
  TM_LAUNCH(kern, grid_of(items), 256, 0, st, a, f, static_cast<T*>(ids_out), lengths_out, row_doc_out, row_start_out);
}
template <typename T>
static void launch_window_spans(const WindowArgs& a, const uint32_t* spans, void* out, hipStream_t st) {
  const Flat f = flat_of(out, 2ull * a.rows * a.L, sizeof(T));
  const auto kern = k_window_spans<T>;
  TM_LAUNCH(kern, grid_of(flat_items(f, sizeof(T))), 256, 0, st, a, f, spans, static_cast<T*>(out));
}

static int windows_spans(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap, void* spans_out, uint32_t span_bytes, bool raw,
                         uint32_t unit, const char* who) {
  WindowArgs a{};
  int rc = window_plan(b, how, overlap, spans_out, who, raw ? 2 : 1, span_bytes, &a);
  if (rc != TM_OK) return rc;
  if (a.rows > rows_cap) return set_error(TM_E_NOSPACE, "%s: rows_cap %llu < %llu rows required", who, (unsigned long long)rows_cap, (unsigned long long)a.rows);
  if (a.rows == 0) return TM_OK;
  const uint64_t total = b->last_totals[1];
  hipStream_t st = (hipStream_t)stream;
  if ((rc = spans_check_lengths(b, who)) != TM_OK || (rc = batch_own_spans_on(b, st, raw ? TM_TEXT_RAW : TM_TEXT_NORMALIZED, unit, total)) != TM_OK) return rc;
  if ((rc = window_row_docs(b, &a, st)) != TM_OK) return rc;
  (void)hipGetLastError();
  a.ids = nullptr;
  if (span_bytes == 4) launch_window_spans<uint32_t>(a, reinterpret_cast<const uint32_t*>(b->d_spans), spans_out, st);
  else launch_window_spans<uint64_t>(a, reinterpret_cast<const uint32_t*>(b->d_spans), spans_out, st);
  return launch_check();
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_window_rows(tm_batch* b, const tm_collate* how, uint32_t overlap, uint64_t* rows_needed) {
  if (!rows_needed) return set_error(TM_E_INVALID, "tm_batch_window_rows: null argument");
  *rows_needed = 0;
  WindowArgs a{};
  int rc = window_plan(b, how, overlap, rows_needed, "tm_batch_window_rows", 0, 0, &a);
  if (rc == TM_OK || rc == TM_E_LIMIT) *rows_needed = a.rows;
  return rc;
}

int tm_batch_windows(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap, void* ids_out, uint8_t* mask_out,
                     uint32_t* lengths_out, uint32_t* row_doc_out, uint32_t* row_start_out) {
  WindowArgs a{};
  int rc = window_plan(b, how, overlap, ids_out, "tm_batch_windows", 0, 0, &a);
  if (rc != TM_OK) return rc;
  if (a.rows > rows_cap) return set_error(TM_E_NOSPACE, "tm_batch_windows: rows_cap %llu < %llu rows required", (unsigned long long)rows_cap, (unsigned long long)a.rows);
  if (a.rows == 0) return TM_OK;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = window_row_docs(b, &a, st)) != TM_OK) return rc;
  (void)hipGetLastError();
  if (how->id_bytes == 2) launch_window_ids<uint16_t>(a, ids_out, lengths_out, row_doc_out, row_start_out, st);
  else if (how->id_bytes == 4) launch_window_ids<uint32_t>(a, ids_out, lengths_out, row_doc_out, row_start_out, st);
  else launch_window_ids<uint64_t>(a, ids_out, lengths_out, row_doc_out, row_start_out, st);
  if (mask_out) {
    const Flat f = flat_of(mask_out, a.rows * a.L, 1);
    const auto kern = k_window_rows<uint8_t, true>;
    TM_LAUNCH(kern, grid_of(flat_items(f, 1)), 256, 0, st, a, f, mask_out, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
  }
  return launch_check();
}

int tm_batch_windows_spans(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap, void* spans_out, uint32_t span_bytes) {
  return windows_spans(b, how, overlap, stream, rows_cap, spans_out, span_bytes, false, TM_UNIT_BYTES, "tm_batch_windows_spans");
}

int tm_batch_windows_raw_spans(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap, void* spans_out, uint32_t span_bytes) {
  return windows_spans(b, how, overlap, stream, rows_cap, spans_out, span_bytes, true, TM_UNIT_BYTES, "tm_batch_windows_raw_spans");
}

int tm_batch_windows_spans_in(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap, uint32_t text, uint32_t unit,
                              void* spans_out, uint32_t span_bytes) {
  const int rc = units_args(text, unit, "tm_batch_windows_spans_in");
  if (rc != TM_OK) return rc;
  return windows_spans(b, how, overlap, stream, rows_cap, spans_out, span_bytes, text == TM_TEXT_RAW, unit, "tm_batch_windows_spans_in");
}

}  // extern "C"

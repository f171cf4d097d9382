// tm_fit.hip — whole-document packing: the ragged ids a batch holds as rows [rows, L] into which the documents are packed WHOLE, in order; a
// row is closed when the next document does not fit, and only a document longer than a row is ever cut (tm_batch_fit_rows, tm_batch_fit).
// The rule: include/tokenmonster_hip.h.
//
// tm_batch_pack is a closed form over one prefix sum.  This rule is a serial recurrence over the documents - whether document d opens a row
// depends on where the row before it was opened - and it is solved the way the match kernel solves its own: a segment summarised as an exit
// map, the maps chained, the one real chain followed.  With key(d) = toff[d] - toff[0] + d * sep (DocCursor, tm_collate.h: where document d
// begins in the stream of entries), E_d = key(d + 1) - key(d), k_d = max(1, ceil(E_d / L)) the rows an opener takes and f_d = E_d -
// (k_d - 1) * L the entries in its last row:
//   1. k_fit_next: next[d] = the first j > d with key(j + 1) - key(d + 1) > L - f_d, a binary search over the offsets.  IF d opens a row,
//      the documents d + 1 .. next[d] - 1 ride in d's last row and next[d] opens the next one (a document longer than L passes the test by itself).
//   2. k_fit_tiles: a workgroup takes a tile of FIT_TILE documents, composes (next, k) with itself in LDS by pointer doubling and leaves the
//      tile's exit map: for every document the first opener beyond the tile that the chain through it reaches and the rows opened on the way.
//   3. k_fit_resolve: one wavefront finds the root (the first document with an entry) and hops from tile to tile through the exit maps:
//      every tile's entry opener and first row (a tile the chain jumps over has none), and the number of rows.
//   4. k_fit_rows: per tile with an entry, the chain inside the tile walked in LDS; the row table (stream position of the row's first entry,
//      entries, document) of every row its openers open, the whole rows of a long document written by the whole workgroup.
//   5. k_fit_fill: the walk of rows of tm_collate.h's fill_walk, spelled out (says why), with a FitRow of the table as
//      the plan of a row and the value rule: element (r, c) is stream position P_r + c, its document found by a DocCursor that starts at the row's own document.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "tm_pipeline.h"
#include "tm_collate.h"

namespace tmh {

constexpr uint32_t FIT_TILE = 1024, FIT_T = 256, FIT_PER = FIT_TILE / FIT_T, FIT_ROUNDS = 10;      // 2^FIT_ROUNDS hops cross a tile
constexpr uint32_t FIT_NONE = 0xFFFFFFFFu;           // a tile without an opener on the real chain

struct FitArgs {
  const uint64_t* toff;       // tok_offsets + first_doc
  uint32_t nd, L, sep;
  __device__ __forceinline__ uint64_t key(uint32_t d) const { return toff[d] - toff[0] + (uint64_t)d * sep; }
};
struct FitExit { uint64_t rows; uint32_t exit, pad; };      // of a document, were it an opener: rows opened up to the first opener beyond its tile, and that opener (nd: none)
struct FitRow { uint64_t P; uint32_t len, doc; };           // a row: stream position of its first entry, its entries, the document of the first
// the rows an opener of E entries takes (a 64-bit division only for a document longer than a row)
__device__ __forceinline__ uint64_t fit_rows_of(uint64_t E, uint32_t L) { return E <= L ? 1u : (E + L - 1) / L; }

// ---- k_fit_next: the opener behind every document, were it one ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fit_next(FitArgs a, uint32_t* __restrict__ next) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= a.nd) return;
  const uint64_t k0 = a.key(d), k1 = a.key(d + 1);
  const uint64_t f = (k1 - k0) - (fit_rows_of(k1 - k0, a.L) - 1) * a.L;      // (0 .. L)
  const uint64_t lim = k1 + (a.L - f);                 // what still fits d's last row ends here
  uint32_t lo = d + 1, hi = a.nd;                      // the first j in [d + 1, nd) with key(j + 1) > lim, or nd
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.key(mid + 1) > lim) hi = mid; else lo = mid + 1;
  }
  next[d] = lo;
}

// ---- k_fit_tiles: the exit map of a tile of documents ----------------------------------------------------------------------------------------
// (jump, rows) of every document composed with the pair of its jump target while that lies inside the tile: after round n a pair covers 2^n
// hops or has left the tile.  Double-buffered: a round reads one plane and writes the other.  A row count is 64 bits wide (one document
// of a batch may take more than 2^32 rows of one id).
__global__ __launch_bounds__(FIT_T) void k_fit_tiles(FitArgs a, const uint32_t* __restrict__ next, FitExit* __restrict__ exits) {
  __shared__ uint32_t jump[2][FIT_TILE];
  __shared__ uint64_t rows[2][FIT_TILE];
  const uint32_t base = blockIdx.x * FIT_TILE, end = (uint32_t)std::min<uint64_t>((uint64_t)base + FIT_TILE, a.nd);
  for (uint32_t q = 0; q < FIT_PER; q++) {
    const uint32_t i = q * FIT_T + threadIdx.x, d = base + i;
    const bool in = d < end;
    jump[0][i] = in ? next[d] : a.nd;
    rows[0][i] = in ? fit_rows_of(a.key(d + 1) - a.key(d), a.L) : 0u;
  }
  __syncthreads();
  uint32_t cur = 0;
  for (uint32_t round = 0; round < FIT_ROUNDS; round++) {
    for (uint32_t q = 0; q < FIT_PER; q++) {
      const uint32_t i = q * FIT_T + threadIdx.x;
      uint32_t j = jump[cur][i];
      uint64_t r = rows[cur][i];
      if (j < end) { r += rows[cur][j - base]; j = jump[cur][j - base]; }      // (next[d] > d: j - base is inside the tile)
      jump[cur ^ 1][i] = j;
      rows[cur ^ 1][i] = r;
    }
    __syncthreads();
    cur ^= 1;
  }
  for (uint32_t q = 0; q < FIT_PER; q++) {
    const uint32_t i = q * FIT_T + threadIdx.x;
    if (base + i < end) exits[base + i] = FitExit{rows[cur][i], jump[cur][i], 0u};
  }
}

// ---- k_fit_resolve: the real chain from tile to tile -----------------------------------------------------------------------------------------
// One wavefront, every lane with the same opener e: the root is the first document with an entry; the entry opener of the next tile with
// one is the exit of this tile's entry.  The lanes share the writing of FIT_NONE into the tiles a jump passes over.
__global__ __launch_bounds__(64) void k_fit_resolve(FitArgs a, const FitExit* __restrict__ exits, uint32_t ntiles, uint32_t* __restrict__ tile_entry,
                                                    uint64_t* __restrict__ tile_row, uint64_t* __restrict__ total) {
  uint32_t lo = 0, hi = a.nd;                          // the first j with key(j + 1) > 0, or nd
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.key(mid + 1) > 0) hi = mid; else lo = mid + 1;
  }
  uint32_t e = lo, done = 0;                           // tiles [0, done) are written
  uint64_t R = 0;
  while (e < a.nd) {
    const uint32_t t = e / FIT_TILE;
    for (uint32_t u = done + threadIdx.x; u < t; u += 64) tile_entry[u] = FIT_NONE;
    if (threadIdx.x == 0) { tile_entry[t] = e; tile_row[t] = R; }
    const FitExit x = exits[e];
    R += x.rows;
    e = x.exit;                                        // (beyond tile t, or nd)
    done = t + 1;
  }
  for (uint32_t u = done + threadIdx.x; u < ntiles; u += 64) tile_entry[u] = FIT_NONE;
  if (threadIdx.x == 0) *total = R;
}

// ---- k_fit_rows: the row table ---------------------------------------------------------------------------------------------------------------
// The tile's (next, k) in LDS; one work-item hops along the real chain there and lists its openers with their first rows; then an opener
// per work-item writes its LAST row - from the rest of the document to where the next opener begins (key(nd), the stream's end, behind
// the last one) - and the workgroup together the whole rows in front of it, of the openers that have any.
__global__ __launch_bounds__(FIT_T) void k_fit_rows(FitArgs a, const uint32_t* __restrict__ next, const uint32_t* __restrict__ tile_entry,
                                                    const uint64_t* __restrict__ tile_row, FitRow* __restrict__ table) {
  __shared__ uint32_t nx[FIT_TILE];
  __shared__ uint64_t kk[FIT_TILE];
  __shared__ uint64_t row_of[FIT_TILE];
  __shared__ uint16_t opener[FIT_TILE], longs[FIT_TILE];
  __shared__ uint32_t n_open, n_long;
  const uint32_t entry = tile_entry[blockIdx.x];
  if (entry == FIT_NONE) return;                       // (the whole workgroup)
  const uint32_t base = blockIdx.x * FIT_TILE, end = (uint32_t)std::min<uint64_t>((uint64_t)base + FIT_TILE, a.nd);
  for (uint32_t q = 0; q < FIT_PER; q++) {
    const uint32_t i = q * FIT_T + threadIdx.x, d = base + i;
    if (d < end) { nx[i] = next[d]; kk[i] = fit_rows_of(a.key(d + 1) - a.key(d), a.L); }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t n = 0, nl = 0;
    uint64_t R = tile_row[blockIdx.x];
    for (uint32_t d = entry; d < end; d = nx[d - base]) {
      const uint32_t i = d - base;
      opener[n] = (uint16_t)i;
      row_of[n] = R;
      if (kk[i] > 1) longs[nl++] = (uint16_t)n;
      R += kk[i];
      n++;
    }
    n_open = n; n_long = nl;
  }
  __syncthreads();
  for (uint32_t m = threadIdx.x; m < n_open; m += FIT_T) {
    const uint32_t i = opener[m], d = base + i;
    const uint64_t P = a.key(d) + (kk[i] - 1) * a.L;
    table[row_of[m] + kk[i] - 1] = FitRow{P, (uint32_t)(a.key(nx[i]) - P), d};      // (<= L entries: what next[] was searched for)
  }
  for (uint32_t l = 0; l < n_long; l++) {
    const uint32_t m = longs[l], i = opener[m], d = base + i;
    const uint64_t P0 = a.key(d), R0 = row_of[m], whole = kk[i] - 1;
    for (uint64_t q = threadIdx.x; q < whole; q += FIT_T) table[R0 + q] = FitRow{P0 + q * a.L, a.L, d};
  }
}

// ---- k_fit_fill: the rows --------------------------------------------------------------------------------------------------------------------
struct FitFill {
  const uint32_t* ids;
  const uint64_t* toff;       // tok_offsets + first_doc
  const FitRow* table;
  uint64_t rows;
  uint32_t nd, L, pad, eos;   // eos: TM_NONE = none
};
// WHAT: 0 = ids (T of 2, 4 or 8 bytes), 1 = doc_index, 2 = position (T = uint32_t).  The per-row outputs (ids launch only, each may be null):
// the first `rows` work-items write a row's length, document and start each.
template <typename T, int WHAT>
__global__ __launch_bounds__(256) void k_fit_fill(FitFill a, Flat f, T* __restrict__ out, uint32_t* __restrict__ lengths, uint32_t* __restrict__ row_doc,
                                                  uint32_t* __restrict__ row_start) {
  constexpr uint32_t PER = 16 / sizeof(T);
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t sep = a.eos != TM_NONE ? 1u : 0u;
  if (WHAT == 0 && (lengths || row_doc || row_start) && t < a.rows) {
    const FitRow w = a.table[t];
    if (lengths) lengths[t] = w.len;
    if (row_doc) row_doc[t] = w.doc;
    if (row_start) row_start[t] = (uint32_t)(w.P - (a.toff[w.doc] - a.toff[0] + (uint64_t)w.doc * sep));
  }
  uint64_t e0;
  uint32_t cnt;
  if (!flat_span<T>(f, t, e0, cnt)) return;
  uint64_t r;
  uint32_t c;
  if (f.n <= 0xFFFFFFFFull) { r = (uint32_t)e0 / a.L; c = (uint32_t)e0 - (uint32_t)r * a.L; }      // (a 64-bit division costs more than the store it is for)
  else { r = e0 / a.L; c = (uint32_t)(e0 - r * a.L); }
  FitRow w = a.table[r];                               // (r is a row: e0 is an element of the output)
  // The cursor searches the documents of ITS row only - from the row's first to the next row's first, which ends behind every position of
  // this row: a handful of steps where the documents are short, not log2(nd) dependent loads in front of every store.
  const auto last_doc = [&](uint64_t row) { return row + 1 < a.rows ? a.table[row + 1].doc + 1u : a.nd; };
  DocCursor cur{a.toff, last_doc(r), sep, 0, 0, 0};
  bool have = false;                                   // the cursor stands on a document
  T vals[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    uint32_t v = 0;
    if (k < cnt) {
      if (c >= w.len) v = WHAT == 0 ? a.pad : WHAT == 1 ? 0xFFFFFFFFu : 0u;
      else {
        const uint64_t p = w.P + c;                    // (rows stand in stream order: p never decreases)
        if (have) cur.advance(p); else { cur.seek(p, w.doc); have = true; }
        const uint64_t pos = p - cur.base;
        if (WHAT == 1) v = cur.d;
        else if (WHAT == 2) v = (uint32_t)pos;
        else v = (sep && p + 1 == cur.next) ? a.eos : a.ids[a.toff[cur.d] + pos];
      }
      if (++c == a.L && k + 1 < cnt) { c = 0; r++; w = a.table[r]; cur.nd = last_doc(r); }      // (another element follows: r is a row)
    }
    vals[k] = (T)v;
  }
  flat_store<T>(out, e0, cnt, vals);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
// the batch's planning buffer for cap documents: exit maps | first row of every tile, the number of rows behind them | next | entry of every tile
struct FitBuf { FitExit* exits; uint64_t* tile_row; uint64_t* total; uint32_t* next; uint32_t* tile_entry; };
static uint64_t fit_tiles(uint32_t nd) { return ((uint64_t)nd + FIT_TILE - 1) / FIT_TILE; }
static uint64_t fit_bytes(uint32_t cap) { return (uint64_t)cap * (sizeof(FitExit) + 4) + fit_tiles(cap) * 12 + 8; }
static FitBuf fit_buf(const tm_batch* b) {
  FitBuf w;
  w.exits = reinterpret_cast<FitExit*>(b->d_fit);
  w.tile_row = reinterpret_cast<uint64_t*>(w.exits + b->fit_cap);
  w.total = w.tile_row + fit_tiles(b->fit_cap);
  w.next = reinterpret_cast<uint32_t*>(w.total + 1);
  w.tile_entry = w.next + b->fit_cap;
  return w;
}
static int fit_reserve(tm_batch* b, uint32_t nd) {
  return batch_reserve_docs(b, (void**)&b->d_fit, &b->fit_cap, nd, fit_bytes, "fit plan");
}

// what both calls share: the arguments, stages 1 to 3 on the stream of the batch's last run, and the number of rows read back from it
// through the mailbox (synchronizes like tm_batch_totals)
static int fit_plan(tm_batch* b, const tm_collate* how, const void* out, const char* who, FitArgs* a, uint64_t* rows) {
  *rows = 0;
  int rc = check_how(b, how, out, who);
  if (rc != TM_OK) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  *a = FitArgs{b->d_tok_offsets + how->first_doc, how->ndocs, how->row_len, how->eos_id != TM_NONE ? 1u : 0u};
  if (how->ndocs == 0) return TM_OK;
  if ((rc = fit_reserve(b, how->ndocs)) != TM_OK) return rc;
  const FitBuf w = fit_buf(b);
  const FitArgs fa = *a;
  const uint32_t ntiles = (uint32_t)fit_tiles(how->ndocs);
  hipStream_t st = b->last_stream;
  (void)hipGetLastError();
  TM_LAUNCH(k_fit_next, grid_of(how->ndocs), 256, 0, st, fa, w.next);
  TM_LAUNCH(k_fit_tiles, ntiles, FIT_T, 0, st, fa, w.next, w.exits);
  TM_LAUNCH(k_fit_resolve, 1, 64, 0, st, fa, w.exits, ntiles, w.tile_entry, w.tile_row, w.total);
  if ((rc = launch_check()) != TM_OK) return rc;
  if ((rc = small_d2h(b, rows, w.total, 8, st)) != TM_OK || (rc = small_sync(b, st)) != TM_OK) return rc;
  return check_row_room(who, how->row_len, 0, *rows, "documents");
}

// WHAT 0 = ids (the per-row outputs may be given), 1 = doc_index, 2 = position
template <typename T, int WHAT>
static void launch_fit(const FitFill& a, void* out, hipStream_t st, uint32_t* lengths_out = nullptr, uint32_t* row_doc_out = nullptr, uint32_t* row_start_out = nullptr) {
  launch_flat(k_fit_fill<T, WHAT>, st, static_cast<T*>(out), a.rows * a.L, (lengths_out || row_doc_out || row_start_out) ? a.rows : 0, a, static_cast<T*>(out), lengths_out,
              row_doc_out, row_start_out);
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_fit_rows(tm_batch* b, const tm_collate* how, uint64_t* rows_needed) {
  if (!rows_needed) return set_error(TM_E_INVALID, "tm_batch_fit_rows: null argument");
  *rows_needed = 0;
  FitArgs a{};
  uint64_t rows = 0;
  const int rc = fit_plan(b, how, rows_needed, "tm_batch_fit_rows", &a, &rows);
  if (rc == TM_OK || rc == TM_E_LIMIT) *rows_needed = rows;
  return rc;
}

int tm_batch_fit(tm_batch* b, const tm_collate* how, void* stream, uint64_t rows_cap, void* ids_out, uint32_t* doc_index_out, uint32_t* position_out,
                 uint32_t* lengths_out, uint32_t* row_doc_out, uint32_t* row_start_out) {
  FitArgs a{};
  uint64_t rows = 0;
  int rc = fit_plan(b, how, ids_out, "tm_batch_fit", &a, &rows);
  if (rc != TM_OK || (rc = check_rows_cap("tm_batch_fit", rows_cap, rows)) != TM_OK) return rc;
  if (rows == 0) return TM_OK;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = grow_batch(b, (void**)&b->d_fit_rows, &b->fit_rows_cap, rows, rows + rows / 4 + 1024, sizeof(FitRow), "fit rows")) != TM_OK) return rc;
  const FitBuf w = fit_buf(b);
  FitRow* table = reinterpret_cast<FitRow*>(b->d_fit_rows);
  (void)hipGetLastError();
  TM_LAUNCH(k_fit_rows, (uint32_t)fit_tiles(how->ndocs), FIT_T, 0, st, a, w.next, w.tile_entry, w.tile_row, table);
  const FitFill fa{b->d_out, a.toff, table, rows, how->ndocs, how->row_len, how->pad_id, how->eos_id};
  with_id_type(how->id_bytes, [&](auto z) { launch_fit<decltype(z), 0>(fa, ids_out, st, lengths_out, row_doc_out, row_start_out); });
  if (doc_index_out) launch_fit<uint32_t, 1>(fa, doc_index_out, st);
  if (position_out) launch_fit<uint32_t, 2>(fa, position_out, st);
  return launch_check();
}

}  // extern "C"

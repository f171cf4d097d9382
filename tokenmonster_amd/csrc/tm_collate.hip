// tm_collate.hip — fixed-shape id tensors from the ragged ids a batch holds, and back: tm_batch_collate (one document per row, padded or
// truncated, BOS / EOS, mask, lengths), tm_batch_pack (one EOS-separated stream cut into rows, with document numbers and positions) and
// tm_batch_load_ids (a [rows, L] tensor of ids -> the batch's ragged ids and offsets, ready for tm_batch_decode).
//
// All three are streaming kernels: no table, no LDS, a few bytes read per byte written.  Every output is treated as ONE flat run of
// elements (a [rows, L] tensor is contiguous): the elements in front of the first 16-byte boundary and behind the last whole 16 bytes are
// stored one by one, everything between as 16-byte vectors, one per work-item, so that a wavefront writes 1 KiB of consecutive bytes per
// store instruction whatever L and the element size are.  A work-item finds the row (the document) of its first element once - a division,
// or a binary search over the offsets - and steps to the next one when its vector crosses a row (document) end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "tm_pipeline.h"
#include "tm_collate.h"

namespace tmh {

// ---- k_collate_rows: one document per row (the flat output and the plan of a row: tm_collate.h) ------------------------------------------------
// The fill is fill_rows (tm_collate.h) with the plan of one document per row.  lengths (ids launch only, may be null): the first `rows`
// work-items write a row's length each.
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void k_collate_rows(CollateArgs a, Flat f, T* __restrict__ out, uint32_t* __restrict__ lengths) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!MASK && lengths && t < a.rows) lengths[t] = row_plan(a, t).len;
  fill_rows<T, MASK>(a, f, out, t, [&](uint64_t r) { return row_plan(a, r); });
}

// ---- k_pack_stream: ids(doc0) [eos] ids(doc1) [eos] ... cut into rows -------------------------------------------------------------------------------------
struct PackArgs {
  const uint32_t* ids;
  const uint64_t* toff;       // tok_offsets + first_doc
  uint32_t nd, pad, eos;      // eos: TM_NONE = none
  uint64_t stream_len;        // key(nd)
};
// WHAT: 0 = ids (T of 2, 4 or 8 bytes), 1 = doc_index, 2 = position (T = uint32_t)
template <typename T, int WHAT>
__global__ __launch_bounds__(256) void k_pack_stream(PackArgs a, Flat f, T* __restrict__ out) {
  constexpr uint32_t PER = 16 / sizeof(T);
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t e0;
  uint32_t cnt;
  if (!flat_span<T>(f, t, e0, cnt)) return;
  const uint32_t sep = a.eos != TM_NONE ? 1u : 0u;
  DocCursor cur{a.toff, a.nd, sep, 0, 0, 0};
  if (e0 < a.stream_len) cur.seek(e0, 0);
  T vals[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    const uint64_t p = e0 + k;
    uint32_t v = 0;
    if (k < cnt) {
      if (p >= a.stream_len) v = WHAT == 0 ? a.pad : WHAT == 1 ? 0xFFFFFFFFu : 0u;
      else {
        cur.advance(p);
        const uint64_t pos = p - cur.base;
        if (WHAT == 1) v = cur.d;
        else if (WHAT == 2) v = (uint32_t)pos;
        else v = (sep && p + 1 == cur.next) ? a.eos : a.ids[a.toff[cur.d] + pos];
      }
    }
    vals[k] = (T)v;
  }
  flat_store<T>(out, e0, cnt, vals);
}

// ---- k_ids_from_rows: [rows, L] -> ragged ids ----------------------------------------------------------------------------------------------------
struct LoadArgs {
  const void* rows;
  const uint32_t* lengths;    // may be null
  uint32_t nrows, L, pad, bos, eos;      // TM_NONE = not given
};
// One wavefront per row, lanes stride over its columns: the leading run of pad ids, one BOS, then the entries up to lengths[r] (if given) and
// to the first EOS (if given) -> where the row's ids begin (col) and how many they are (ntok).  Work-item 0 leaves the batch's totals and
// error word as a run leaves them (the id total comes from the scan behind this kernel).
template <typename T>
__global__ __launch_bounds__(256) void k_row_extents(LoadArgs a, uint32_t* __restrict__ ntok, uint32_t* __restrict__ col, uint32_t* __restrict__ missing,
                                                     uint64_t* __restrict__ totals, uint32_t* __restrict__ error) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { totals[0] = 0; totals[2] = 0; totals[3] = 0; *error = 0u; }
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  if (r >= a.nrows) return;                          // (the whole wavefront leaves)
  const T* __restrict__ row = static_cast<const T*>(a.rows) + r * a.L;
  uint32_t start = 0;
  if (a.pad != TM_NONE) {
    start = a.L;
    for (uint32_t base = 0; base < a.L; base += 64) {
      const uint32_t c = base + lane;
      const unsigned long long m = __ballot(c < a.L && (uint64_t)row[c] != (uint64_t)a.pad);
      if (m) { start = base + (uint32_t)__ffsll(m) - 1u; break; }
    }
  }
  uint32_t end = a.L;
  if (a.lengths) end = (uint32_t)std::min<uint64_t>((uint64_t)start + a.lengths[r], a.L);
  if (a.bos != TM_NONE && start < end && (uint64_t)row[start] == (uint64_t)a.bos) start++;
  if (a.eos != TM_NONE) {
    for (uint32_t base = start; base < end; base += 64) {
      const uint32_t c = base + lane;
      const unsigned long long m = __ballot(c < end && (uint64_t)row[c] == (uint64_t)a.eos);
      if (m) { end = base + (uint32_t)__ffsll(m) - 1u; break; }
    }
  }
  if (lane == 0) { ntok[r] = end - start; col[r] = start; missing[r] = 0u; }
}
// the gather behind the scan: four ids per work-item, one 16-byte store into the batch's id buffer (which holds nrows * L + 4 ids at least;
// the count is read from the device: toff[nrows])
template <typename T>
__global__ __launch_bounds__(256) void k_ids_from_rows(LoadArgs a, const uint64_t* __restrict__ toff, const uint32_t* __restrict__ col, uint32_t* __restrict__ out) {
  const uint64_t e0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const uint64_t total = toff[a.nrows];
  if (e0 >= total) return;
  DocCursor cur{toff, a.nrows, 0u, 0, 0, 0};
  cur.seek(e0, 0);
  const T* __restrict__ rows = static_cast<const T*>(a.rows);
  uint32_t vals[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint64_t p = e0 + k;
    uint32_t v = 0;
    if (p < total) {
      cur.advance(p);
      v = (uint32_t)rows[(uint64_t)cur.d * a.L + col[cur.d] + (p - cur.base)];
    }
    vals[k] = v;
  }
  flat_store<uint32_t>(out, e0, 4, vals);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
// the arguments both layouts share (ids_out: only that it is there)
int check_how(const tm_batch* b, const tm_collate* how, const void* ids_out, const char* who) {
  if (!b || !how || !ids_out) return set_error(TM_E_INVALID, "%s: null argument", who);
  if (how->id_bytes != 2 && how->id_bytes != 4 && how->id_bytes != 8) return set_error(TM_E_INVALID, "%s: id_bytes %u (2, 4 or 8)", who, how->id_bytes);
  if (how->row_len == 0) return set_error(TM_E_INVALID, "%s: row_len 0", who);
  if (how->pad_id == TM_NONE) return set_error(TM_E_INVALID, "%s: pad_id must be given", who);
  if (how->flags & ~(TM_COLLATE_PAD_LEFT | TM_COLLATE_KEEP_TAIL)) return set_error(TM_E_INVALID, "%s: unknown flags %#x", who, how->flags);
  if (how->id_bytes == 2) {
    if (b->vocab->host.n_ids > 65536u) return set_error(TM_E_INVALID, "%s: two-byte ids with a vocabulary of %u ids", who, b->vocab->host.n_ids);
    for (uint32_t s : {how->pad_id, how->bos_id, how->eos_id})
      if (s != TM_NONE && s >= 65536u) return set_error(TM_E_INVALID, "%s: special id %u does not fit two bytes", who, s);
  }
  if (!b->has_output) return set_error(TM_E_INVALID, "%s: the batch holds no ids (no completed tm_batch_run or tm_batch_load_ids since the last upload)", who);
  if ((uint64_t)how->first_doc + how->ndocs > b->ndocs)
    return set_error(TM_E_INVALID, "%s: documents %u .. %llu of a run of %u", who, how->first_doc, (unsigned long long)how->first_doc + how->ndocs, b->ndocs);
  return TM_OK;
}

template <typename T>
static void launch_collate(const CollateArgs& a, void* ids_out, uint32_t* lengths_out, hipStream_t st) {
  const Flat f = flat_of(ids_out, (uint64_t)a.rows * a.L, sizeof(T));
  const uint64_t items = std::max<uint64_t>(flat_items(f, sizeof(T)), lengths_out ? a.rows : 0);
  const auto kern = k_collate_rows<T, false>;
  TM_LAUNCH(kern, grid_of(items), 256, 0, st, a, f, static_cast<T*>(ids_out), lengths_out);
}
template <typename T>
static void launch_pack_ids(const PackArgs& a, void* ids_out, uint64_t n, hipStream_t st) {
  const Flat f = flat_of(ids_out, n, sizeof(T));
  const auto kern = k_pack_stream<T, 0>;
  TM_LAUNCH(kern, grid_of(flat_items(f, sizeof(T))), 256, 0, st, a, f, static_cast<T*>(ids_out));
}

// stream length of the documents [first, first + nd) with `sep` separators each: two offsets from the device (synchronizes like tm_batch_totals)
static int pack_stream_len(tm_batch* b, const tm_collate* how, uint64_t* stream_len) {
  *stream_len = 0;
  if (how->ndocs == 0) return TM_OK;
  uint64_t lo = 0, hi = 0;
  int rc = small_d2h(b, &lo, b->d_tok_offsets + how->first_doc, 8, b->last_stream);
  if (rc == TM_OK) rc = small_d2h(b, &hi, b->d_tok_offsets + how->first_doc + how->ndocs, 8, b->last_stream);
  if (rc == TM_OK) rc = small_sync(b, b->last_stream);
  if (rc != TM_OK) return rc;
  *stream_len = hi - lo + (how->eos_id != TM_NONE ? (uint64_t)how->ndocs : 0);
  return TM_OK;
}
static int pack_rows(tm_batch* b, const tm_collate* how, const void* ids_out, const char* who, uint64_t* stream_len, uint64_t* rows) {
  int rc = check_how(b, how, ids_out, who);
  if (rc != TM_OK) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK || (rc = pack_stream_len(b, how, stream_len)) != TM_OK) return rc;
  *rows = (*stream_len + how->row_len - 1) / how->row_len;
  if (*rows * how->row_len > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "%s: %llu rows of %u ids in one call (split the documents)", who, (unsigned long long)*rows, how->row_len);
  return TM_OK;
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_collate(tm_batch* b, const tm_collate* how, void* stream, void* ids_out, uint8_t* mask_out, uint32_t* lengths_out) {
  int rc = check_how(b, how, ids_out, "tm_batch_collate");
  if (rc != TM_OK) return rc;
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + (how->eos_id != TM_NONE ? 1u : 0u);
  if (how->row_len < ns) return set_error(TM_E_INVALID, "tm_batch_collate: row_len %u holds no %u specials", how->row_len, ns);
  if ((uint64_t)how->ndocs * how->row_len > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "tm_batch_collate: %u rows of %u ids in one call (split the documents)", how->ndocs, how->row_len);
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  if (how->ndocs == 0) return TM_OK;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  const CollateArgs a{b->d_out, b->d_tok_offsets + how->first_doc, how->ndocs, how->row_len, how->pad_id, how->bos_id, how->eos_id, how->flags};
  if (how->id_bytes == 2) launch_collate<uint16_t>(a, ids_out, lengths_out, st);
  else if (how->id_bytes == 4) launch_collate<uint32_t>(a, ids_out, lengths_out, st);
  else launch_collate<uint64_t>(a, ids_out, lengths_out, st);
  if (mask_out) {
    const Flat f = flat_of(mask_out, (uint64_t)a.rows * a.L, 1);
    const auto kern = k_collate_rows<uint8_t, true>;
    TM_LAUNCH(kern, grid_of(flat_items(f, 1)), 256, 0, st, a, f, mask_out, (uint32_t*)nullptr);
  }
  return launch_check();
}

int tm_batch_pack_rows(tm_batch* b, const tm_collate* how, uint64_t* rows_needed) {
  if (!rows_needed) return set_error(TM_E_INVALID, "tm_batch_pack_rows: null argument");
  *rows_needed = 0;
  uint64_t stream_len = 0;
  return pack_rows(b, how, rows_needed, "tm_batch_pack_rows", &stream_len, rows_needed);
}

int tm_batch_pack(tm_batch* b, const tm_collate* how, void* stream, uint64_t rows_cap, void* ids_out, uint32_t* doc_index_out, uint32_t* position_out) {
  uint64_t stream_len = 0, rows = 0;
  int rc = pack_rows(b, how, ids_out, "tm_batch_pack", &stream_len, &rows);
  if (rc != TM_OK) return rc;
  if (rows > rows_cap) return set_error(TM_E_NOSPACE, "tm_batch_pack: rows_cap %llu < %llu rows required", (unsigned long long)rows_cap, (unsigned long long)rows);
  if (rows == 0) return TM_OK;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  const uint64_t n = rows * how->row_len;
  const PackArgs a{b->d_out, b->d_tok_offsets + how->first_doc, how->ndocs, how->pad_id, how->eos_id, stream_len};
  if (how->id_bytes == 2) launch_pack_ids<uint16_t>(a, ids_out, n, st);
  else if (how->id_bytes == 4) launch_pack_ids<uint32_t>(a, ids_out, n, st);
  else launch_pack_ids<uint64_t>(a, ids_out, n, st);
  if (doc_index_out) {
    const Flat f = flat_of(doc_index_out, n, 4);
    const auto kern = k_pack_stream<uint32_t, 1>;
    TM_LAUNCH(kern, grid_of(flat_items(f, 4)), 256, 0, st, a, f, doc_index_out);
  }
  if (position_out) {
    const Flat f = flat_of(position_out, n, 4);
    const auto kern = k_pack_stream<uint32_t, 2>;
    TM_LAUNCH(kern, grid_of(flat_items(f, 4)), 256, 0, st, a, f, position_out);
  }
  return launch_check();
}

int tm_batch_load_ids(tm_batch* b, const void* rows, uint32_t nrows, uint32_t row_len, uint32_t id_bytes, const uint32_t* lengths, uint32_t pad_id,
                      uint32_t bos_id, uint32_t eos_id, void* stream) {
  if (!b || (nrows && !rows)) return set_error(TM_E_INVALID, "tm_batch_load_ids: null argument");
  if (id_bytes != 2 && id_bytes != 4 && id_bytes != 8) return set_error(TM_E_INVALID, "tm_batch_load_ids: id_bytes %u (2, 4 or 8)", id_bytes);
  if (nrows && row_len == 0) return set_error(TM_E_INVALID, "tm_batch_load_ids: row_len 0");
  if (nrows && reinterpret_cast<uintptr_t>(rows) % id_bytes) return set_error(TM_E_INVALID, "tm_batch_load_ids: rows not aligned to id_bytes");
  if (id_bytes == 2) {
    if (b->vocab->host.n_ids > 65536u) return set_error(TM_E_INVALID, "tm_batch_load_ids: two-byte ids with a vocabulary of %u ids", b->vocab->host.n_ids);
    for (uint32_t s : {pad_id, bos_id, eos_id})
      if (s != TM_NONE && s >= 65536u) return set_error(TM_E_INVALID, "tm_batch_load_ids: special id %u does not fit two bytes", s);
  }
  if (nrows > b->max_docs) return set_error(TM_E_LIMIT, "tm_batch_load_ids: %u rows, workspace sized for %u documents", nrows, b->max_docs);
  const uint64_t bound = (uint64_t)nrows * row_len;
  if (bound > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "tm_batch_load_ids: %u rows of %u ids in one call (split the rows)", nrows, row_len);
  { int rc = enter_device(b->vocab); if (rc != TM_OK) return rc; }
  hipError_t e;
  hipStream_t st = (hipStream_t)stream;
  if (bound + 4 > b->out_cap) {          // (the gather stores whole 16 bytes)
    // what the last run left may still be read on its stream
    if ((e = hipStreamSynchronize(b->last_stream)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    const int rc = grow_batch(b, (void**)&b->d_out, &b->out_cap, bound + 4, bound + bound / 4 + 1024, 4, "ids");
    if (rc != TM_OK) return rc;
  }
  (void)hipGetLastError();
  b->has_output = false;
  b->row_form = -1;                      // (these ids come from no walk: they have no spans)
  b->ndocs = nrows;
  b->last_stream = st;
  b->nbytes = 0; b->nseg = 0;
  const LoadArgs a{rows, lengths, nrows, row_len, pad_id, bos_id, eos_id};
  if (nrows == 0) {
    if ((e = hipMemsetAsync(b->d_totals, 0, 40, st)) != hipSuccess || (e = hipMemsetAsync(b->d_tok_offsets, 0, 8, st)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    b->has_output = true;
    return TM_OK;
  }
  const uint32_t g1 = (nrows + 3) / 4;
  if (id_bytes == 2) TM_LAUNCH(k_row_extents<uint16_t>, g1, 256, 0, st, a, b->d_doc_ntok, b->d_doc_events, b->d_doc_missing, b->d_totals, b->d_error);
  else if (id_bytes == 4) TM_LAUNCH(k_row_extents<uint32_t>, g1, 256, 0, st, a, b->d_doc_ntok, b->d_doc_events, b->d_doc_missing, b->d_totals, b->d_error);
  else TM_LAUNCH(k_row_extents<uint64_t>, g1, 256, 0, st, a, b->d_doc_ntok, b->d_doc_events, b->d_doc_missing, b->d_totals, b->d_error);
  scan_u32(b->d_doc_ntok, nrows, b->d_scan_tmp, b->d_totals + 1, b->d_tok_offsets, st);
  const uint32_t g2 = grid_of((bound + 3) / 4);
  if (id_bytes == 2) TM_LAUNCH(k_ids_from_rows<uint16_t>, g2, 256, 0, st, a, b->d_tok_offsets, b->d_doc_events, b->d_out);
  else if (id_bytes == 4) TM_LAUNCH(k_ids_from_rows<uint32_t>, g2, 256, 0, st, a, b->d_tok_offsets, b->d_doc_events, b->d_out);
  else TM_LAUNCH(k_ids_from_rows<uint64_t>, g2, 256, 0, st, a, b->d_tok_offsets, b->d_doc_events, b->d_out);
  int rc = launch_check();
  if (rc == TM_OK) b->has_output = true;
  return rc;
}

}  // extern "C"

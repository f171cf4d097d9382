// tm_collate.hip — fixed-shape id tensors from the ragged ids a batch holds, and back: tm_batch_collate (one document per row, padded or
// truncated, BOS / EOS, mask, lengths), tm_batch_collate_select (the same rows for a LIST of document numbers: any order, repeats, a shuffled
// or length-grouped batch), tm_batch_pack (one EOS-separated stream cut into rows, with document numbers and positions) and
// tm_batch_load_ids (a [rows, L] tensor of ids -> the batch's ragged ids and offsets, ready for tm_batch_decode).
//
// All are streaming kernels: no table, a few bytes read per byte written (LDS only where the selection stages its rows' plans).  Every output is treated as ONE flat run of
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
// The fill is fill_walk (tm_collate.h) with the plan of one document per row and RowValue.  lengths (ids launch only, may be null): the first `rows`
// work-items write a row's length each.
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void k_collate_rows(CollateArgs a, Flat f, T* __restrict__ out, uint32_t* __restrict__ lengths) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!MASK && lengths && t < a.rows) lengths[t] = row_plan(a, t).len;
  fill_walk<T>(f, a.L, out, t, [&](uint64_t r) { return row_plan(a, r); }, RowValue<MASK, CollateArgs>{a});
}

// ---- k_collate_select: document doc_index[r] in row r ---------------------------------------------------------------------------------------------
// The same fill with select_plan.  A workgroup takes SEL_VECS vectors per work-item, 256 consecutive ones at a time; they cover consecutive
// elements, so few rows - one or two at the row lengths of a model: their plans (doc_index[r], then that document's two offsets) are staged
// in LDS by one work-item each, once per workgroup, and the fill reads them there.  A row outside the staged run - beyond SEL_STAGE rows
// where rows are a few ids long, or the single elements in front of and behind the vectors - is planned from global memory as before.
constexpr uint32_t SEL_STAGE = 256, SEL_VECS = 4;
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void k_collate_select(SelectArgs s, Flat f, T* __restrict__ out, uint32_t* __restrict__ lengths) {
  constexpr uint32_t PER = 16 / sizeof(T);
  __shared__ RowPlan plans[SEL_STAGE];
  const uint64_t t0 = (uint64_t)blockIdx.x * (256 * SEL_VECS);
  uint64_t r0 = 0;
  uint32_t staged = 0;
  if (t0 < f.nvec) {                                   // rows of the first and the last element of this workgroup's vectors
    const uint64_t e0 = f.head + t0 * PER, e1 = f.head + std::min<uint64_t>(t0 + 256 * SEL_VECS, f.nvec) * PER - 1;
    uint64_t r1;
    if (f.n <= 0xFFFFFFFFull) { r0 = (uint32_t)e0 / s.a.L; r1 = (uint32_t)e1 / s.a.L; }      // (as in fill_walk: no 64-bit division where 32 bits do)
    else { r0 = e0 / s.a.L; r1 = e1 / s.a.L; }
    staged = (uint32_t)std::min<uint64_t>(r1 - r0 + 1, SEL_STAGE);
  }
  if (threadIdx.x < staged) plans[threadIdx.x] = select_plan(s, r0 + threadIdx.x);      // (rows of elements of the output)
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < SEL_VECS; k++) {
    const uint64_t t = t0 + k * 256 + threadIdx.x;
    if (!MASK && lengths && t < s.a.rows) lengths[t] = select_plan(s, t).len;
    fill_walk<T>(f, s.a.L, out, t, [&](uint64_t r) { return r - r0 < staged ? plans[r - r0] : select_plan(s, r); }, RowValue<MASK, CollateArgs>{s.a});
  }
}
// the rows whose index is no document of the run: one workgroup, one plain store (bad_out may be page-locked host memory)
__global__ __launch_bounds__(1024) void k_select_bad(const uint32_t* __restrict__ doc_index, uint32_t rows, uint32_t run_docs, uint32_t* __restrict__ bad) {
  __shared__ uint32_t wsum[16];
  uint32_t c = 0;
  for (uint64_t r = threadIdx.x; r < rows; r += blockDim.x) c += doc_index[r] >= run_docs ? 1u : 0u;
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < blockDim.x / 64; w++) c += wsum[w];
    *bad = c;
  }
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
// ... in the two parts a layout's own checks (its flags) stand between: the shape of a row, and that the batch's ids fit the output
int check_row_shape(bool given, uint32_t id_bytes, uint32_t row_len, uint32_t pad_id, const char* who) {
  if (!given) return set_error(TM_E_INVALID, "%s: null argument", who);
  if (id_bytes != 2 && id_bytes != 4 && id_bytes != 8) return set_error(TM_E_INVALID, "%s: id_bytes %u (2, 4 or 8)", who, id_bytes);
  if (row_len == 0) return set_error(TM_E_INVALID, "%s: row_len 0", who);
  if (pad_id == TM_NONE) return set_error(TM_E_INVALID, "%s: pad_id must be given", who);
  return TM_OK;
}
int check_ids_fit(const tm_batch* b, uint32_t id_bytes, std::initializer_list<uint32_t> specials, const char* who) {
  if (id_bytes == 2) {
    if (b->vocab->host.n_ids > 65536u) return set_error(TM_E_INVALID, "%s: two-byte ids with a vocabulary of %u ids", who, b->vocab->host.n_ids);
    for (uint32_t s : specials)
      if (s != TM_NONE && s >= 65536u) return set_error(TM_E_INVALID, "%s: special id %u does not fit two bytes", who, s);
  }
  if (!b->has_output) return set_error(TM_E_INVALID, "%s: the batch holds no ids (no completed tm_batch_run or tm_batch_load_ids since the last upload)", who);
  return TM_OK;
}
int check_how(const tm_batch* b, const tm_collate* how, const void* ids_out, const char* who) {
  int rc = check_row_shape(b && how && ids_out, how ? how->id_bytes : 0, how ? how->row_len : 0, how ? how->pad_id : 0, who);
  if (rc != TM_OK) return rc;
  if (how->flags & ~(TM_COLLATE_PAD_LEFT | TM_COLLATE_KEEP_TAIL)) return set_error(TM_E_INVALID, "%s: unknown flags %#x", who, how->flags);
  if ((rc = check_ids_fit(b, how->id_bytes, {how->pad_id, how->bos_id, how->eos_id}, who)) != TM_OK) return rc;
  if ((uint64_t)how->first_doc + how->ndocs > b->ndocs)
    return set_error(TM_E_INVALID, "%s: documents %u .. %llu of a run of %u", who, how->first_doc, (unsigned long long)how->first_doc + how->ndocs, b->ndocs);
  return TM_OK;
}
int check_row_room(const char* who, uint32_t row_len, uint32_t ns, uint64_t rows, const char* what) {
  if (row_len < ns) return set_error(TM_E_INVALID, "%s: row_len %u holds no %u specials", who, row_len, ns);
  if (rows * row_len > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "%s: %llu rows of %u ids in one call (split the %s)", who, (unsigned long long)rows, row_len, what);
  return TM_OK;
}
int check_rows_cap(const char* who, uint64_t rows_cap, uint64_t rows) {
  if (rows > rows_cap) return set_error(TM_E_NOSPACE, "%s: rows_cap %llu < %llu rows required", who, (unsigned long long)rows_cap, (unsigned long long)rows);
  return TM_OK;
}

// the launches: ids (lengths_out may be given) or, MASK, the mask; a workgroup of the selection takes 256 * SEL_VECS work-items
template <typename T, bool MASK>
static void launch_collate(const CollateArgs& a, void* out, hipStream_t st, uint32_t* lengths_out = nullptr) {
  launch_flat(k_collate_rows<T, MASK>, st, static_cast<T*>(out), (uint64_t)a.rows * a.L, lengths_out ? a.rows : 0, a, static_cast<T*>(out), lengths_out);
}
template <typename T, bool MASK>
static void launch_select(const SelectArgs& s, void* out, hipStream_t st, uint32_t* lengths_out = nullptr) {
  launch_flat<256 * SEL_VECS>(k_collate_select<T, MASK>, st, static_cast<T*>(out), (uint64_t)s.a.rows * s.a.L, lengths_out ? s.a.rows : 0, s, static_cast<T*>(out), lengths_out);
}
void launch_select_bad(const uint32_t* doc_index, uint32_t rows, uint32_t run_docs, uint32_t* bad_out, hipStream_t st) {
  TM_LAUNCH(k_select_bad, 1, 1024, 0, st, doc_index, rows, run_docs, bad_out);
}
template <typename T, int WHAT>
static void launch_pack(const PackArgs& a, void* out, uint64_t n, hipStream_t st) {
  launch_flat(k_pack_stream<T, WHAT>, st, static_cast<T*>(out), n, 0, a, static_cast<T*>(out));
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
  return check_row_room(who, how->row_len, 0, *rows, "documents");
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_collate(tm_batch* b, const tm_collate* how, void* stream, void* ids_out, uint8_t* mask_out, uint32_t* lengths_out) {
  int rc = check_how(b, how, ids_out, "tm_batch_collate");
  if (rc != TM_OK) return rc;
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + (how->eos_id != TM_NONE ? 1u : 0u);
  if ((rc = check_row_room("tm_batch_collate", how->row_len, ns, how->ndocs, "documents")) != TM_OK) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  if (how->ndocs == 0) return TM_OK;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  const CollateArgs a{b->d_out, b->d_tok_offsets + how->first_doc, how->ndocs, how->row_len, how->pad_id, how->bos_id, how->eos_id, how->flags};
  with_id_type(how->id_bytes, [&](auto z) { launch_collate<decltype(z), false>(a, ids_out, st, lengths_out); });
  if (mask_out) launch_collate<uint8_t, true>(a, mask_out, st);
  return launch_check();
}

int tm_batch_collate_select(tm_batch* b, const tm_collate* how, const uint32_t* doc_index, void* stream, void* ids_out, uint8_t* mask_out, uint32_t* lengths_out,
                            uint32_t* bad_out) {
  static const char who[] = "tm_batch_collate_select";
  if (!how) return set_error(TM_E_INVALID, "%s: null argument", who);
  tm_collate any = *how;                               // (ndocs counts rows here, not documents of the run: nothing of it for check_how's range)
  any.ndocs = 0;
  int rc = check_how(b, &any, ids_out, who);
  if (rc != TM_OK) return rc;
  if (how->first_doc != 0) return set_error(TM_E_INVALID, "%s: first_doc %u (the indices count from the run's first document: 0)", who, how->first_doc);
  if (how->ndocs && !doc_index) return set_error(TM_E_INVALID, "%s: null doc_index", who);
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + (how->eos_id != TM_NONE ? 1u : 0u);
  if ((rc = check_row_room(who, how->row_len, ns, how->ndocs, "rows")) != TM_OK) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (bad_out) launch_select_bad(doc_index, how->ndocs, b->ndocs, bad_out, st);
  if (how->ndocs == 0) return bad_out ? launch_check() : TM_OK;
  const SelectArgs s{CollateArgs{b->d_out, b->d_tok_offsets, how->ndocs, how->row_len, how->pad_id, how->bos_id, how->eos_id, how->flags}, doc_index, b->ndocs};
  with_id_type(how->id_bytes, [&](auto z) { launch_select<decltype(z), false>(s, ids_out, st, lengths_out); });
  if (mask_out) launch_select<uint8_t, true>(s, mask_out, st);
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
  if (rc != TM_OK || (rc = check_rows_cap("tm_batch_pack", rows_cap, rows)) != TM_OK) return rc;
  if (rows == 0) return TM_OK;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  const uint64_t n = rows * how->row_len;
  const PackArgs a{b->d_out, b->d_tok_offsets + how->first_doc, how->ndocs, how->pad_id, how->eos_id, stream_len};
  with_id_type(how->id_bytes, [&](auto z) { launch_pack<decltype(z), 0>(a, ids_out, n, st); });
  if (doc_index_out) launch_pack<uint32_t, 1>(a, doc_index_out, n, st);
  if (position_out) launch_pack<uint32_t, 2>(a, position_out, n, st);
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
  with_id_type(id_bytes, [&](auto z) { TM_LAUNCH(k_row_extents<decltype(z)>, g1, 256, 0, st, a, b->d_doc_ntok, b->d_doc_events, b->d_doc_missing, b->d_totals, b->d_error); });
  scan_u32(b->d_doc_ntok, nrows, b->d_scan_tmp, b->d_totals + 1, b->d_tok_offsets, st);
  const uint32_t g2 = grid_of((bound + 3) / 4);
  with_id_type(id_bytes, [&](auto z) { TM_LAUNCH(k_ids_from_rows<decltype(z)>, g2, 256, 0, st, a, b->d_tok_offsets, b->d_doc_events, b->d_out); });
  int rc = launch_check();
  if (rc == TM_OK) b->has_output = true;
  return rc;
}

}  // extern "C"

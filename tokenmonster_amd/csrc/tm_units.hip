// tm_units.hip — character offsets: the (begin, end) pairs of the ids counted in code points or UTF-16 units instead of bytes (the rule:
// tokenmonster_hip.h, "character offsets"; its host statement: tm_utf8_units, tm_build.h).
//
// Two kernels.  k_unit_index streams over the resident text - the raw text as uploaded (d_raw) or the normalized text (d_text) - and writes, per
// UNIT_BLOCK bytes of the buffer, the number of non-continuation bytes and (UTF-16 only) of bytes >= 0xF0; the run's scan kernels (scan_u32) turn
// the counts into prefixes over the whole buffer.  k_unit_spans then converts the ragged byte pairs where they lie, a work-item per pair: U at an
// absolute position of the buffer is the prefix of its block plus a count over the part of the block in front of it, and the value at the
// document's begin is subtracted.  The collate and window fills read the converted pairs unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tm_pipeline.h"
#include "tm_collate.h"

namespace tmh {

typedef uint32_t span_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t UNIT_BLOCK = 256;                       // bytes of text per index entry
constexpr uint32_t UNIT_LANES = UNIT_BLOCK / 16;           // lanes that share an entry: 16 bytes each
constexpr uint32_t UNIT_TILE = 4 * 256 * 16;               // bytes of text per workgroup and trip: four 16-byte loads per lane
static_assert(UNIT_LANES == 16 && 64 % UNIT_LANES == 0, "an index entry is summed inside one wavefront: xor 8, 4, 2, 1");

// per 32-bit word of text: the bytes that are continuation bytes (bit 7 set, bit 6 clear), the bytes >= 0xF0 (bits 7 .. 4 set) - as bit 7 of each
__device__ __forceinline__ uint32_t cont_mask(uint32_t w) { return w & ~(w << 1) & 0x80808080u; }
__device__ __forceinline__ uint32_t f0_mask(uint32_t w) { return w & (w << 1) & (w << 2) & (w << 3) & 0x80808080u; }

struct UnitCount { uint32_t nc, f0; };      // non-continuation bytes, bytes >= 0xF0

template <bool F0>
__device__ __forceinline__ void count_word(uint32_t w, uint32_t nbytes, UnitCount& c) {      // the low `nbytes` bytes of w
  if (nbytes < 4u) w = (w & ((1u << (8u * nbytes)) - 1u)) | (0x80808080u << (8u * nbytes));      // (the rest become continuation bytes: they count for nothing)
  c.nc += 4u - (uint32_t)__popc(cont_mask(w));
  if (F0) c.f0 += (uint32_t)__popc(f0_mask(w));
}

// the counts over text[x, y): single bytes up to a word boundary, words up to a 16-byte boundary, 16-byte loads, then words and bytes again.
// Nothing outside [x, y) is read.
template <bool F0>
__device__ __forceinline__ UnitCount count_range(const uint8_t* __restrict__ text, uint64_t x, uint64_t y) {
  UnitCount c{0u, 0u};
  const uint8_t* p = text + x;
  const uint8_t* const e = text + y;
  while (p < e && (reinterpret_cast<uintptr_t>(p) & 3u)) { count_word<F0>(*p, 1u, c); p++; }
  while (p + 4 <= e && (reinterpret_cast<uintptr_t>(p) & 15u)) { count_word<F0>(*reinterpret_cast<const uint32_t*>(p), 4u, c); p += 4; }
  while (p + 16 <= e) {
    const u32x4 q = *reinterpret_cast<const u32x4*>(p);
    count_word<F0>(q.x, 4u, c); count_word<F0>(q.y, 4u, c); count_word<F0>(q.z, 4u, c); count_word<F0>(q.w, 4u, c);
    p += 16;
  }
  while (p + 4 <= e) { count_word<F0>(*reinterpret_cast<const uint32_t*>(p), 4u, c); p += 4; }
  while (p < e) { count_word<F0>(*p, 1u, c); p++; }
  return c;
}

// The same counts for the conversion's short ranges - a token, the bytes between two neighbouring begins -, where the five loops above cost a
// wavefront the longest trip count of each: ONE loop over the aligned 32-bit words that cover [x, y), the bytes outside the range masked into
// continuation bytes.  A word may reach up to 3 bytes in front of x and behind y: `readable` says how far the buffer may be read (its allocation,
// not the text's end); a range that reaches beyond it or is longer than a block, and every range of a buffer that is not aligned, goes through
// count_range.
template <bool F0>
__device__ __forceinline__ UnitCount count_short(const uint8_t* __restrict__ text, uint64_t x, uint64_t y, uint64_t readable, uint32_t aligned) {
  const uint64_t a0 = x & ~3ull;
  if (!aligned || y - a0 > UNIT_BLOCK || ((y + 3u) & ~3ull) > readable) return count_range<F0>(text, x, y);
  UnitCount c{0u, 0u};
  const uint32_t nb = (uint32_t)(y - a0), skip = (uint32_t)(x - a0);      // bytes from the first word's begin to y; of the first word, the bytes in front of x
  const uint32_t* __restrict__ wp = reinterpret_cast<const uint32_t*>(text + a0);
  for (uint32_t o = 0; o < nb; o += 4u) {
    const uint32_t hi = nb - o;                                            // the word's bytes [lo, hi) lie in the range
    uint32_t keep = hi >= 4u ? 0xFFFFFFFFu : (1u << (8u * hi)) - 1u;
    if (o == 0u) keep &= ~((1u << (8u * skip)) - 1u);
    count_word<F0>((wp[o >> 2] & keep) | (0x80808080u & ~keep), 4u, c);
  }
  return c;
}

// ---- k_unit_index: the counts per UNIT_BLOCK bytes of text[0, n) -----------------------------------------------------------------------------------
// Lane l of a workgroup's trip reads the 16 bytes at tile + k * 4096 + 16 l, k = 0 .. 3 - a wavefront 1 KiB per load instruction, all four in flight
// before the first count -, counts by mask and popcount, and the 16 lanes of an entry add up through the wavefront's cross-lane network.  The
// lane at the head of an entry stores.  aligned: `text` lies on a 16-byte boundary (every buffer of a batch does); the last, partial 16 bytes of
// the text - and all of it otherwise - go through count_range, which reads nothing behind n.  CP / F0: which of the two planes are wanted.
template <bool CP, bool F0>
__global__ __launch_bounds__(256) void k_unit_index(const uint8_t* __restrict__ text, uint64_t n, uint32_t aligned, uint32_t* __restrict__ cnt_cp,
                                                    uint32_t* __restrict__ cnt_f0) {
  const uint64_t ntiles = (n + UNIT_TILE - 1) / UNIT_TILE;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = tile * UNIT_TILE + (uint64_t)threadIdx.x * 16u;
    u32x4 q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t at = base + (uint64_t)k * 4096u;
      q[k] = (u32x4)(0x80808080u);
      if (aligned && at + 16u <= n) q[k] = TM_STREAM_LOAD(reinterpret_cast<const u32x4*>(text + at));
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t at = base + (uint64_t)k * 4096u;
      UnitCount c{0u, 0u};
      if (aligned && at + 16u <= n) { count_word<F0>(q[k].x, 4u, c); count_word<F0>(q[k].y, 4u, c); count_word<F0>(q[k].z, 4u, c); count_word<F0>(q[k].w, 4u, c); }
      else if (at < n) c = count_range<F0>(text, at, std::min<uint64_t>(at + 16u, n));
      uint32_t v = F0 ? (c.nc | (c.f0 << 16)) : c.nc;      // (both fit: at most 256 per entry)
#pragma unroll
      for (int m = UNIT_LANES / 2; m > 0; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
      if ((threadIdx.x & (UNIT_LANES - 1u)) == 0u && at < n) {
        const uint64_t blk = at / UNIT_BLOCK;
        if (CP) cnt_cp[blk] = v & 0xFFFFu;
        if (F0) cnt_f0[blk] = v >> 16;
      }
    }
  }
}

// ---- k_unit_spans: the byte pairs of the run converted where they lie ------------------------------------------------------------------------------
// Id t of the run belongs to the document d found by doc_of_id (tm_collate.h); the document is text[dbegin[d], dend[d]) (clamped to the n bytes
// the index covers).  U at the absolute position p: pre[p / UNIT_BLOCK] plus the count over [p rounded down, p) - 128 bytes on average, and the
// value at the document's begin is to be subtracted: two long counts.  But the 64 ids of a wavefront follow one another in a document and their
// begins never decrease, so only the HEAD of a stretch pays them - lane 0, the first id of a document, a begin that lies in front of the lane's
// before (no walk produces one) -; every other lane counts the few bytes between its neighbour's begin and its own, and a segmented scan over the
// wavefront adds them up.  The end of a non-empty pair counts on from its begin.  A work-item reads and writes its own pair only; no lane leaves
// before the scan.
template <bool F0>
__global__ __launch_bounds__(256) void k_unit_spans(span_t* pairs, const uint64_t* __restrict__ tok_offsets, uint32_t ndocs, const uint64_t* __restrict__ dbegin,
                                                    const uint64_t* __restrict__ dend, const uint8_t* __restrict__ text, uint64_t n,
                                                    uint64_t readable, uint32_t aligned, const uint64_t* __restrict__ pre_cp, const uint64_t* __restrict__ pre_f0,
                                                    uint64_t total) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = t < total;
  const int lane = (int)(threadIdx.x & 63u);
  auto units = [&](const UnitCount& c) { return c.nc + (F0 ? c.f0 : 0u); };
  auto U = [&](uint64_t p) {                          // p: an absolute position of the buffer, <= n
    const uint64_t blk = p / UNIT_BLOCK;
    return pre_cp[blk] + (F0 ? pre_f0[blk] : 0ull) + units(count_range<F0>(text, blk * UNIT_BLOCK, p));
  };
  uint32_t d = 0;
  uint64_t d0 = 0, b = 0, e = 0;
  span_t s;
  s.x = s.y = 0u;
  if (live) {
    d = doc_of_id(tok_offsets, ndocs, t);
    d0 = std::min<uint64_t>(dbegin[d], n);
    const uint64_t len = std::min<uint64_t>(std::max<uint64_t>(dend[d], d0), n) - d0;
    s = pairs[t];
    b = std::min<uint64_t>(s.x, len);
    e = std::min<uint64_t>(s.y, len);
    if (b < len && (text[d0 + b] & 0xC0u) == 0x80u) { // char_start: at most 3 bytes back, never in front of the document
      for (uint64_t k = 1; k <= 3u && k <= b; k++) if ((text[d0 + b - k] & 0xC0u) != 0x80u) { b -= k; break; }
    }
  }
  const unsigned long long p = d0 + b;
  const int before = lane > 0 ? lane - 1 : 0;
  const unsigned long long pp = __shfl(p, before);
  const uint32_t pd = (uint32_t)__shfl((int)d, before);
  uint32_t head = (!live || lane == 0 || pd != d || pp > p) ? 1u : 0u;
  uint32_t v = 0;                                     // U(p) - U(d0) for a head, else the units of [the lane before's begin, p)
  if (live) v = head ? (uint32_t)(U(p) - U(d0)) : units(count_short<F0>(text, pp, p, readable, aligned));
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int src = lane >= off ? lane - off : 0;
    const uint32_t pv = (uint32_t)__shfl((int)v, src), ph = (uint32_t)__shfl((int)head, src);
    if (lane >= off) { if (!head) v += pv; head |= ph; }
  }
  if (live) {
    span_t r;
    r.x = v;
    r.y = v;
    if (s.y > s.x && e > b) r.y = v + units(count_short<F0>(text, d0 + b, d0 + e, readable, aligned));
    pairs[t] = r;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
// One plane of an index for `cap` blocks: pre[cap + 1] (u64, the scan's output: pre[k] = the count in front of block k) | the scan's block sums,
// its total behind them (u64) | the counts (u32).  An index holds two planes: non-continuation bytes, bytes >= 0xF0.
struct UnitPlane { uint64_t* pre; uint64_t* sums; uint64_t* total; uint32_t* cnt; };
static uint64_t unit_sum_words(uint64_t cap) { return (cap + 1 + SCAN_CH - 1) / SCAN_CH + 1; }
static uint64_t unit_plane_bytes(uint64_t cap) { return ((cap + 1 + unit_sum_words(cap)) * 8 + cap * 4 + 15) & ~15ull; }
static UnitPlane unit_plane(const tm_batch* b, int kind, int plane) {
  UnitPlane p;
  p.pre = reinterpret_cast<uint64_t*>(b->d_units[kind] + (uint64_t)plane * unit_plane_bytes(b->units_cap[kind]));
  p.sums = p.pre + b->units_cap[kind] + 1;
  p.total = p.sums + unit_sum_words(b->units_cap[kind]) - 1;
  p.cnt = reinterpret_cast<uint32_t*>(p.total + 1);
  return p;
}

int units_args(uint32_t text, uint32_t unit, const char* who) {
  if (text != TM_TEXT_NORMALIZED && text != TM_TEXT_RAW) return set_error(TM_E_INVALID, "%s: text %u (TM_TEXT_NORMALIZED or TM_TEXT_RAW)", who, text);
  if (unit != TM_UNIT_BYTES && unit != TM_UNIT_CODEPOINTS && unit != TM_UNIT_UTF16) return set_error(TM_E_INVALID, "%s: unit %u (TM_UNIT_BYTES, TM_UNIT_CODEPOINTS or TM_UNIT_UTF16)", who, unit);
  return TM_OK;
}

// the planes `unit` needs of the index of this text, where the batch does not hold them yet
static int unit_index_on(tm_batch* b, hipStream_t st, int kind, uint32_t unit, const uint8_t* text, uint64_t n) {
  const uint32_t want = unit == TM_UNIT_UTF16 ? 3u : 1u;
  const uint64_t nblk = (n + UNIT_BLOCK - 1) / UNIT_BLOCK;
  if (b->units_have[kind] && b->units_blocks[kind] != nblk) b->units_have[kind] = 0;      // (cannot happen: new text forgets the index)
  const uint32_t make = want & ~b->units_have[kind];
  if (!make) return TM_OK;
  if (!b->d_units[kind] || nblk > b->units_cap[kind]) {
    const uint64_t cap = nblk + nblk / 8 + 16;          // (two planes of 12 bytes per 256 of text and an eighth of headroom: below 1/8 of the text)
    const uint64_t old_bytes = b->d_units[kind] ? 2 * unit_plane_bytes(b->units_cap[kind]) : 0;
    b->units_cap[kind] = 0;
    b->units_have[kind] = 0;
    const int rc = batch_replace(b, (void**)&b->d_units[kind], old_bytes, 2 * unit_plane_bytes(nblk), 2 * unit_plane_bytes(cap), "unit index");
    if (rc != TM_OK) return rc;
    b->units_cap[kind] = cap;
  }
  const uint32_t todo = want & ~b->units_have[kind];
  const UnitPlane cp = unit_plane(b, kind, 0), f0 = unit_plane(b, kind, 1);
  (void)hipGetLastError();
  if (nblk) {
    const uint64_t ntiles = (n + UNIT_TILE - 1) / UNIT_TILE;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, 8192);
    const uint32_t aligned = (reinterpret_cast<uintptr_t>(text) & 15u) == 0 ? 1u : 0u;
    if (todo == 3u) { const auto kern = k_unit_index<true, true>; TM_LAUNCH(kern, grid, 256, 0, st, text, n, aligned, cp.cnt, f0.cnt); }
    else if (todo == 1u) { const auto kern = k_unit_index<true, false>; TM_LAUNCH(kern, grid, 256, 0, st, text, n, aligned, cp.cnt, f0.cnt); }
    else { const auto kern = k_unit_index<false, true>; TM_LAUNCH(kern, grid, 256, 0, st, text, n, aligned, cp.cnt, f0.cnt); }
  }
  if (todo & 1u) scan_u32(cp.cnt, nblk, cp.sums, cp.total, cp.pre, st);
  if (todo & 2u) scan_u32(f0.cnt, nblk, f0.sums, f0.total, f0.pre, st);
  const int rc = launch_check();
  if (rc == TM_OK) { b->units_have[kind] |= todo; b->units_blocks[kind] = nblk; }
  return rc;
}

// the ragged BYTE pairs in `pairs` (device or page-locked, as batch_spans_on / batch_raw_spans_on left them for this `text`) converted in place on
// `st` - the unit index of the text first where the batch does not hold it yet; nothing at all for TM_UNIT_BYTES
static int batch_units_on(tm_batch* b, hipStream_t st, uint32_t text, uint32_t unit, void* pairs, uint64_t total) {
  if (unit == TM_UNIT_BYTES || total == 0 || b->ndocs == 0) return TM_OK;
  const int kind = text == TM_TEXT_RAW ? 1 : 0;
  const uint8_t* buf;
  uint64_t n, readable;                                // readable: the bytes of the buffer that may be loaded (k_unit_spans loads whole aligned words)
  const uint64_t *dbegin, *dend;
  if (kind == 1) { buf = b->d_raw; n = b->raw_bytes; readable = b->raw_cap; dbegin = b->d_raw_off; dend = b->d_raw_off + 1; }      // the text as uploaded, never the filter pass's
  else {
    pack_text(b, st);                                  // (the normalized text out of the normalizer's slabs where it still lies there)
    buf = b->d_text; n = b->nbytes; readable = b->text_borrowed ? n : b->max_bytes + 256; dbegin = b->d_doc_begin; dend = b->d_doc_end;
  }
  int rc = unit_index_on(b, st, kind, unit, buf, n);
  if (rc != TM_OK) return rc;
  const UnitPlane cp = unit_plane(b, kind, 0), f0 = unit_plane(b, kind, 1);
  const uint32_t aligned = (reinterpret_cast<uintptr_t>(buf) & 15u) == 0 ? 1u : 0u;
  readable = std::max(readable, n);
  (void)hipGetLastError();
  if (unit == TM_UNIT_UTF16) { const auto kern = k_unit_spans<true>; TM_LAUNCH(kern, grid_of(total), 256, 0, st, static_cast<span_t*>(pairs), b->d_tok_offsets, b->ndocs, dbegin, dend, buf, n, readable, aligned, cp.pre, f0.pre, total); }
  else { const auto kern = k_unit_spans<false>; TM_LAUNCH(kern, grid_of(total), 256, 0, st, static_cast<span_t*>(pairs), b->d_tok_offsets, b->ndocs, dbegin, dend, buf, n, readable, aligned, cp.pre, f0.pre, total); }
  return launch_check();
}

// the byte pairs of `text` into `out`, then their conversion; ms[4]: the parts of tm_batch_raw_spans_timed and the unit work, between HIP events on `st`
int batch_spans_in_on(tm_batch* b, hipStream_t st, uint32_t text, uint32_t unit, void* out, uint64_t total, uint32_t* host_docs, float* ms) {
  if (host_docs) *host_docs = 0;
  if (ms) ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
  const bool raw = text == TM_TEXT_RAW;
  EventBracket ev(st, ms ? 3 : 0);
  ev.mark(0);
  int rc = raw ? batch_raw_spans_on(b, st, out, total, host_docs, ms)      // (fills ms[0..2] and synchronizes when ms is given)
               : batch_spans_on(b, st, out, total);
  ev.mark(1);
  if (rc == TM_OK) rc = batch_units_on(b, st, text, unit, out, total);
  ev.mark(2);
  float parts[2] = {0.f, 0.f};                        // the byte pairs, the unit work
  rc = ev.finish(parts, rc);
  if (ms) { if (!raw) ms[0] = parts[0]; ms[3] = parts[1]; }
  return rc;
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_spans_in(tm_batch* b, void* stream, uint32_t text, uint32_t unit, uint32_t* spans_out, uint64_t spans_cap, uint32_t* host_docs, float* ms) {
  return ragged_spans_impl(b, stream, text, unit, spans_out, spans_cap, host_docs, ms, "tm_batch_spans_in");
}

int tm_batch_collate_spans_in(tm_batch* b, const tm_collate* how, void* stream, uint32_t text, uint32_t unit, void* spans_out, uint32_t span_bytes) {
  int rc = units_args(text, unit, "tm_batch_collate_spans_in");
  if (rc != TM_OK) return rc;
  return collate_spans_impl(b, how, stream, text, unit, spans_out, span_bytes, "tm_batch_collate_spans_in");
}

}  // extern "C"

// tm_masked.hip — tm_batch_collate_masked: the rows of tm_batch_collate / tm_batch_collate_select with a share of their content ids replaced
// by a mask id or a random id, and the originals as labels (BERT / RoBERTa dynamic masking, SpanBERT-style spans).  The rule:
// include/tokenmonster_hip.h.  It is keyed by the place g of an id in the batch's id buffer, never by its place in a row, so a seed masks
// a document the same way whatever row, padding side, cut or batch it lands in.
//
// One kernel, organised by ROW (the spans run along a row's content), not by flat vector as the fills of tm_collate.h are:
//   - a wavefront owns a tile of 64 * PER consecutive columns of ONE row, PER = 16 / sizeof(T) per lane; a workgroup's four wavefronts own
//     four consecutive tiles in (row, tile) order - of one row where rows are long, of up to four rows where a row is one tile.  The tile's
//     number comes through readfirstlane, so the row's plan (doc_index[r], the document's two offsets: row_plan of tm_collate.h) is read
//     once per wavefront with scalar loads;
//   - a tile without content ids (padding, specials) runs no Philox at all: it stores and leaves;
//   - every lane runs Philox4x32-10 for its PER content ids in registers.  An id that opens a span of `reach` ids at position p of the tile
//     ENDS it at p + reach, and an id is selected iff the largest end over the ids of its document at or in front of it lies behind it.
//     That is the rule's recurrence rem(g) = max(reach(g), rem(g - 1) - 1) with g added on both sides: the pair (a, n) of f(x) = max(a, x - n)
//     collapses into ONE number whose composition is max, so the wavefront's scan is a six-step running maximum of the lanes' largest ends;
//   - what enters a tile from the ids in front of its first content id - the previous tile's, or ids of the same document that the row has
//     cut off (KEEP_TAIL) - is at most span_max - 1 <= 31 ids, never beyond the document's first: lanes 0 .. span_max - 2 recompute the
//     reach of one such id each and a butterfly maximum makes it the scan's seed.  Token masking (span_max == 1) has nothing to carry and
//     skips both the recomputation and the scan (a uniform branch);
//   - ids and labels leave as one 16-byte store per lane where the tile's first element is 16-byte aligned (uniform per wavefront) and
//     the lane's columns are all inside the row, else element by element; the mask as one store of PER bytes where that is aligned;
//   - the first tile of a row writes lengths_out[r].  The count of bad rows is k_select_bad's (tm_collate.hip): a plain store, no cleared word.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "tm_pipeline.h"
#include "tm_collate.h"
#include "tm_philox.h"

namespace tmh {

struct MaskedArgs {
  SelectArgs s;               // s.doc_index null: row r holds document r of s.a.toff (tok_offsets + first_doc), s.run_docs = the rows
  uint64_t units;             // rows * tiles: the wavefronts with work
  uint32_t tiles;             // of a row
  uint32_t key0, key1;        // the seed
  uint32_t span_min, span_n, span_max;      // span_n = span_max - span_min + 1
  uint64_t start_thr, mask_thr, random_end; // random_end = mask_thr + random_thr
  uint32_t mask_id, random_lo, random_n;
  uint64_t ignore;            // label_ignore, sign-extended
};

// what a selected id becomes
__device__ __forceinline__ uint32_t corrupted(const MaskedArgs& m, const uint32_t w[4], uint32_t id) {
  if ((uint64_t)w[2] < m.mask_thr) return m.mask_id;
  if ((uint64_t)w[2] < m.random_end) return m.random_lo + mulhi32(w[3], m.random_n);
  return id;
}

// a lane's 16 / sizeof(T) elements from position pos0 of a tile of nt elements at `tile`: one 16-byte store where the tile begins on a
// 16-byte boundary (the same for every lane of the wavefront) and the lane's elements are all inside the row
template <typename T>
__device__ __forceinline__ void tile_store(T* __restrict__ tile, uint32_t pos0, uint32_t nt, const T* vals) {
  constexpr uint32_t PER = 16 / sizeof(T);
  if (pos0 + PER <= nt && (reinterpret_cast<uintptr_t>(tile) & 15u) == 0) {
    uint4 v;
    __builtin_memcpy(&v, vals, 16);
    *reinterpret_cast<uint4*>(tile + pos0) = v;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < PER; k++)
      if (pos0 + k < nt) tile[pos0 + k] = vals[k];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_collate_masked(MaskedArgs m, T* __restrict__ ids_out, T* __restrict__ labels, uint8_t* __restrict__ mask_out,
                                                        uint32_t* __restrict__ lengths) {
  constexpr uint32_t PER = 16 / sizeof(T), TILE = 64 * PER;
  using MaskWord = typename std::conditional<PER == 2, uint16_t, typename std::conditional<PER == 4, uint32_t, uint64_t>::type>::type;
  const CollateArgs& a = m.s.a;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((uint32_t)(threadIdx.x >> 6));
  const uint64_t u = (uint64_t)blockIdx.x * 4 + wave;
  if (u >= m.units) return;                            // (the whole wavefront)
  uint64_t r;
  uint32_t tile;
  if (m.units <= 0xFFFFFFFFull) { r = (uint32_t)u / m.tiles; tile = (uint32_t)u - (uint32_t)r * m.tiles; }
  else { r = u / m.tiles; tile = (uint32_t)(u - r * m.tiles); }
  // the row's plan, once per wavefront; t0: where its document begins in the id buffer
  const uint32_t d = m.s.doc_index ? m.s.doc_index[r] : (uint32_t)r;
  const bool good = d < m.s.run_docs;
  const RowPlan p = good ? row_plan(a, d) : RowPlan{0, 0, 0};
  const uint64_t t0 = good ? a.toff[d] : 0;
  const uint32_t hb = a.bos != TM_NONE ? 1u : 0u, he = a.eos != TM_NONE ? 1u : 0u;
  const uint32_t c0 = tile * TILE, nt = std::min<uint32_t>(TILE, a.L - c0);      // the tile: columns c0 .. c0 + nt - 1 (c0 < L)
  // the content columns [ca, cb) of the row as positions [pa, pb) of the tile
  const uint32_t ca = p.lo + hb, cb = ca + (p.len > hb + he ? p.len - hb - he : 0u);      // (a row of a bad index has no entries at all)
  const uint32_t pa = ca > c0 ? std::min<uint32_t>(ca - c0, nt) : 0u, pb = cb > c0 ? std::min<uint32_t>(cb - c0, nt) : 0u;
  const bool spans = pb > pa && m.start_thr != 0;      // (uniform: the tile holds content ids, and ids are selected at all)

  const uint32_t pos0 = lane * PER;
  uint32_t orig[PER], cand[PER];
  int32_t end[PER];
  bool content[PER];
  int32_t lane_end = NO_END;
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    const uint32_t pos = pos0 + k, j = c0 + pos - p.lo;      // (j wraps to a large number left of the entries; pos >= nt: not used)
    content[k] = pos >= pa && pos < pb;
    uint32_t v = a.pad;
    if (pos < nt && j < p.len) v = (hb && j == 0) ? a.bos : (he && j == p.len - 1) ? a.eos : a.ids[p.src + (j - hb)];
    orig[k] = cand[k] = v;
    end[k] = NO_END;
    if (spans && content[k]) {
      uint32_t w[4];
      philox4x32_10(p.src + (j - hb), m.key0, m.key1, w);
      const uint32_t reach = reach_of(m, w);
      if (reach) end[k] = (int32_t)(pos + reach);
      cand[k] = corrupted(m, w, v);
      lane_end = std::max(lane_end, end[k]);
    }
  }
  // the largest end in front of this lane's first position: the ids in front of the tile's first content id, then the lanes before
  int32_t run = NO_END;
  if (spans && m.span_max > 1) {
    const uint64_t gf = p.src + (c0 + pa - ca);        // the tile's first content id; ids t0 .. gf - 1 of its document stand before it
    int32_t carry = NO_END;
    if (lane + 1 < m.span_max && (uint64_t)lane < gf - t0) {
      uint32_t w[4];
      philox4x32_10(gf - 1 - lane, m.key0, m.key1, w);
      const uint32_t reach = reach_of(m, w);
      if (reach) carry = (int32_t)pa - 1 - (int32_t)lane + (int32_t)reach;
    }
    for (int off = 32; off > 0; off >>= 1) carry = std::max(carry, __shfl_xor(carry, off));
    int32_t inc = lane_end;
    for (uint32_t off = 1; off < 64; off <<= 1) {
      const int32_t up = __shfl(inc, (int)((lane - off) & 63u));
      if (lane >= off) inc = std::max(inc, up);
    }
    const int32_t before = __shfl(inc, (int)((lane - 1) & 63u));
    run = lane ? std::max(before, carry) : carry;
  }
  T vals[PER], labs[PER];
  uint8_t ent[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    const uint32_t pos = pos0 + k;
    run = std::max(run, end[k]);
    const bool sel = content[k] && run > (int32_t)pos;
    vals[k] = (T)(sel ? cand[k] : orig[k]);
    labs[k] = sel ? (T)orig[k] : (T)m.ignore;
    ent[k] = (c0 + pos - p.lo) < p.len ? 1 : 0;
  }
  // the stores
  const uint64_t e0 = r * a.L + c0;                    // the tile's first element
  const bool whole = pos0 + PER <= nt;
  tile_store<T>(ids_out + e0, pos0, nt, vals);
  if (labels) tile_store<T>(labels + e0, pos0, nt, labs);
  if (mask_out) {
    uint8_t* const dst = mask_out + e0 + pos0;
    if (whole && (reinterpret_cast<uintptr_t>(dst) & (PER - 1)) == 0) {
      MaskWord v;
      __builtin_memcpy(&v, ent, PER);
      *reinterpret_cast<MaskWord*>(dst) = v;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < PER; k++)
        if (pos0 + k < nt) dst[k] = ent[k];
    }
  }
  if (lengths && tile == 0 && lane == 0) lengths[r] = p.len;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
static int check_masking(const tm_masking* m, uint32_t id_bytes, const char* who) {
  constexpr uint64_t ONE = 1ull << 32;
  if (!m) return set_error(TM_E_INVALID, "%s: null masking", who);
  if (m->span_min < 1 || m->span_min > m->span_max || m->span_max > 32) return set_error(TM_E_INVALID, "%s: spans of %u .. %u ids (1 <= span_min <= span_max <= 32)", who, m->span_min, m->span_max);
  if (m->start_thr > ONE || m->mask_thr > ONE || m->random_thr > ONE || m->mask_thr + m->random_thr > ONE)
    return set_error(TM_E_INVALID, "%s: a threshold, or mask_thr + random_thr, above 2^32", who);
  if (m->random_thr && m->random_n == 0) return set_error(TM_E_INVALID, "%s: random ids asked for and random_n 0", who);
  const uint64_t top = id_bytes == 2 ? 0xFFFFull : 0xFFFFFFFFull;
  if (m->mask_id > top) return set_error(TM_E_INVALID, "%s: mask_id %u does not fit %u bytes", who, m->mask_id, id_bytes);
  if (m->random_n && (uint64_t)m->random_lo + m->random_n - 1 > top)
    return set_error(TM_E_INVALID, "%s: random ids %u .. %llu do not fit %u bytes", who, m->random_lo, (unsigned long long)m->random_lo + m->random_n - 1, id_bytes);
  if (id_bytes == 2 && (m->label_ignore < 0 || m->label_ignore > 0xFFFF)) return set_error(TM_E_INVALID, "%s: label_ignore %d does not fit two bytes", who, m->label_ignore);
  return TM_OK;
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_collate_masked(tm_batch* b, const tm_collate* how, const tm_masking* m, const uint32_t* doc_index, void* stream, void* ids_out, void* labels_out,
                            uint8_t* mask_out, uint32_t* lengths_out, uint32_t* bad_out) {
  static const char who[] = "tm_batch_collate_masked";
  if (!how) return set_error(TM_E_INVALID, "%s: null argument", who);
  tm_collate any = *how;                               // (with a list ndocs counts rows, not documents of the run: tm_batch_collate_select)
  if (doc_index) any.ndocs = 0;
  int rc = check_how(b, &any, ids_out, who);
  if (rc != TM_OK || (rc = check_masking(m, how->id_bytes, who)) != TM_OK) return rc;
  if (doc_index && how->first_doc != 0) return set_error(TM_E_INVALID, "%s: first_doc %u (the indices count from the run's first document: 0)", who, how->first_doc);
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + (how->eos_id != TM_NONE ? 1u : 0u);
  if ((rc = check_row_room(who, how->row_len, ns, how->ndocs, doc_index ? "rows" : "documents")) != TM_OK) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (bad_out) launch_select_bad(doc_index, doc_index ? how->ndocs : 0, b->ndocs, bad_out, st);      // (no list: no row is bad)
  if (how->ndocs == 0) return bad_out ? launch_check() : TM_OK;
  const uint32_t tile = 64 * (16 / how->id_bytes);
  MaskedArgs k;
  k.s = SelectArgs{CollateArgs{b->d_out, b->d_tok_offsets + (doc_index ? 0 : how->first_doc), how->ndocs, how->row_len, how->pad_id, how->bos_id, how->eos_id, how->flags},
                   doc_index, doc_index ? b->ndocs : how->ndocs};
  k.tiles = (uint32_t)(((uint64_t)how->row_len + tile - 1) / tile);
  k.units = (uint64_t)how->ndocs * k.tiles;            // (< 2^33: a row is at least one tile, and rows * row_len <= 2^36)
  k.key0 = (uint32_t)m->seed; k.key1 = (uint32_t)(m->seed >> 32);
  k.span_min = m->span_min; k.span_max = m->span_max; k.span_n = m->span_max - m->span_min + 1;
  k.start_thr = m->start_thr; k.mask_thr = m->mask_thr; k.random_end = m->mask_thr + m->random_thr;
  k.mask_id = m->mask_id; k.random_lo = m->random_lo; k.random_n = m->random_n;
  k.ignore = (uint64_t)(int64_t)m->label_ignore;
  const uint32_t grid = (uint32_t)((k.units + 3) / 4);
  with_id_type(how->id_bytes, [&](auto z) {
    using T = decltype(z);
    TM_LAUNCH(k_collate_masked<T>, grid, 256, 0, st, k, static_cast<T*>(ids_out), static_cast<T*>(labels_out), mask_out, lengths_out);
  });
  return launch_check();
}

}  // extern "C"

// tm_spans.hip — where in the text every id came from: the byte span [begin, end) of each id of a run, in the slot order of the ids
// (tm_batch_spans), laid out like tm_batch_collate's rows (tm_batch_collate_spans).  Offsets count from the document's start in the
// NORMALIZED text the walk ran on.
//
// The span pass is a sibling of K4's position-staging walk (k_emit_list, tm_kernels.hip): it reads what a run leaves behind - the T(p,0)
// rows, the side lists / the dense T(p,1) array, the per-segment records of k_seg_params - walks every chain again and writes, for the
// output slot K4 wrote an id to, the position the walk stood on and that position plus the advance.  It reads only the advance / flag byte of
// a position, never an id, adds to no counter and writes nothing but its output.
//
// The collated form is tm_collate.h's fill body for pairs (fill_spans) with the plan of one document per row; tm_windows.hip runs the same body
// with the plan of a window.  The host side holds the bodies the span calls share: ragged_spans_impl (the ragged calls, tm_units.hip's
// included), batch_own_spans_on (the pairs into the batch's own buffer: the collate and window span calls, the one-shot calls of tm_host.hip)
// and collate_spans_impl.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "tm_pipeline.h"
#include "tm_collate.h"

namespace tmh {

typedef uint32_t span_t __attribute__((ext_vector_type(2)));      // (begin, end): one 8-byte store

// The flag byte of position pp of segment g where it lies in HBM.  FORM (k_match_branch's `narrow`, recorded by the run): 0 = one plane of
// u32 words, whose top byte IS the flag byte (advance [0..5] | fd' [6] | missing [7]); 1 = u16 ids + u8 flags; 2 = u32 ids + u8 flags.
template <int FORM>
__device__ __forceinline__ uint32_t flag_byte(const uint32_t* __restrict__ R0, uint64_t g, uint32_t pp) {
  if (FORM == 0) return R0[g * SEG + pp] >> 24;
  constexpr uint64_t RS = FORM == 2 ? R0_WIDE : R0_NARROW, FO = FORM == 2 ? 4 * SEG : 2 * SEG;
  return reinterpret_cast<const uint8_t*>(R0)[g * RS + FO + pp];
}

// k_emit_list without the id fetch.  A wavefront takes TSL consecutive segments: the flag plane of their rows goes to LDS, lane s walks the
// chain of segment s and stages - in the bytes it has passed - the position of every output slot (the same position twice in a row: the
// second slot is the delete token behind the token of the first); a second phase of the whole wavefront turns every listed position p into
// (seg_off + p, seg_off + p + adv(p)), the delete slot into the end twice, with adv from the flag plane where it lies in HBM (the walk has
// written its list over the copy in LDS), one 8-byte store per slot.  Slots of a forward-delete state - whose advance is the side list's, not
// the plane's - are written by the walk itself and marked in the segment's bit map, like the delete slot behind them; so is everything from
// the first slot on that no longer fits in front of the byte being read, or belongs to a step that consumes no byte (stage_after = 512, test
// hook 10: every slot).  seg_off = (g - doc_seg_start[doc]) * SEG.  total: the number of slots (= ids) of the run; nothing is written beyond it.
template <int FORM>
__global__ __launch_bounds__(64) void k_span_list(const uint32_t* __restrict__ R0, const uint2* __restrict__ side, const uint32_t* __restrict__ R1,
                                                  const uint4* __restrict__ par, uint64_t nseg, const uint32_t* __restrict__ seg_doc,
                                                  const uint64_t* __restrict__ doc_seg_start, uint64_t total, span_t* __restrict__ out,
                                                  uint32_t stage_after, uint32_t nounk) {
  alignas(16) __shared__ uint8_t s_m[TSL][TROW_L];
  __shared__ uint32_t s_side[TSL][9];                 // (a word of slack: slot numbers up to TROW_L - 1 are looked up)
  __shared__ uint32_t s_n[TSL], s_off[TSL];
  __shared__ uint64_t s_base[TSL];
  const int lane = threadIdx.x;
  const uint64_t g0 = (uint64_t)blockIdx.x * TSL;
  if (g0 >= nseg) return;
  const int nv = (int)(nseg - g0 < (uint64_t)TSL ? nseg - g0 : (uint64_t)TSL);
  const TileSeg t = tile_segment(par, g0 + lane, lane < TSL, nseg);
  constexpr uint32_t SLACK = TSLACK_L;
  {
    // lane l fetches the flag bytes of positions 4l .. 4l+3 of every row; all loads before the first LDS write
    uint32_t vb[TSL];
#pragma unroll
    for (int s = 0; s < TSL; s++) {
      const int ss = s < nv ? s : nv - 1;
      const uint32_t len = s < nv ? (uint32_t)__shfl((int)t.seglen, ss) : 0u;
      vb[s] = 0u;
      if (4u * (uint32_t)lane < len) {
        if (FORM == 0) {
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          const u32x4 q = TM_STREAM_LOAD(reinterpret_cast<const u32x4*>(R0 + (g0 + (uint64_t)ss) * SEG) + lane);
          vb[s] = (q.x >> 24) | ((q.y >> 24) << 8) | ((q.z >> 24) << 16) | (q.w & 0xFF000000u);
        } else {
          constexpr uint64_t RS = FORM == 2 ? R0_WIDE : R0_NARROW, FO = FORM == 2 ? 4 * SEG : 2 * SEG;
          vb[s] = TM_STREAM_LOAD(reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(R0) + (g0 + (uint64_t)ss) * RS + FO) + lane);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < TSL; s++) *reinterpret_cast<uint32_t*>(&s_m[s][TSLACK_L + 4 * lane]) = vb[s];
#pragma unroll
    for (int i = lane; i < TSL * 9; i += 64) reinterpret_cast<uint32_t*>(s_side)[i] = 0u;
    static_assert((TSL & (TSL - 1)) == 0 && TSL >= 8 && TSL <= 64 && SEG == 256, "a lane per segment, lane & (TSL - 1); a lane fetches four flag bytes of a row");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
  }
  uint32_t staged = 0, off = 0;
  {
    const int rl = lane & (TSL - 1);                                     // (lanes >= TSL have no segment; they only need valid pointers)
    uint8_t* rowm = s_m[rl];
    uint32_t* smap = s_side[rl];
    const uint2* __restrict__ sl = side + (g0 + rl) * SIDE_STRIDE;
    if (t.have) { const uint64_t g = g0 + lane; off = (uint32_t)((g - doc_seg_start[seg_doc[g]]) * SEG); }      // (a document is shorter than 2^32 bytes: checked by the host)
    const uint32_t seglen = t.have ? t.seglen : 0u;
    uint32_t p = t.entry >> 1, fd = t.entry & 1u, E = 0, direct = 0, hop = 0;
    // gate: as in k_emit_list (>= 0: straight-line step; GATE_DEAD < gate < 0: general step; GATE_DEAD: the chain has left the segment)
    constexpr int GATE_DEAD = -(1 << 24);
    const int slack0 = (int)SLACK - 2 - (int)stage_after;
    int gate = p < seglen ? slack0 + (int)p - (int)(fd << 16) : GATE_DEAD;
    auto put = [&](uint32_t slot, uint32_t a, uint32_t e) __attribute__((always_inline)) {
      if (t.base + slot < total) { span_t v; v.x = a; v.y = e; TM_STREAM_STORE(&out[t.base + slot], v); }
    };
    auto fast_step = [&]() __attribute__((always_inline)) {
      const uint32_t m8 = rowm[SLACK + p];
      const uint32_t miss = m8 >> 7, fdn = (m8 >> 6) & 1u, adv = m8 & 63u;
      const uint32_t has = 1u - (miss & nounk);
      rowm[E] = (uint8_t)p; E += has; rowm[E] = (uint8_t)p;              // the id's slot, then (same position again) the delete token's
      E += fdn;
      gate += (int)adv - (int)(fdn * 0x10001u + has);
      fd = fdn;
      p += max(adv, 1u);
      gate = p < seglen ? gate : GATE_DEAD;
    };
    for (;;) {
#ifndef TM_EMU
      if (gate >= 0) {
        do fast_step(); while (__builtin_amdgcn_ballot_w64(gate < 0) == 0ull);       // (a ballot of the lanes in the loop)
      }
#else
      if (__builtin_amdgcn_ballot_w64(gate >= 0) != 0ull) {
        const bool in = gate >= 0;
        do { if (in) fast_step(); } while (__builtin_amdgcn_ballot_w64(in && gate < 0) == 0ull);
      }
#endif
      const bool general = (uint32_t)gate > (uint32_t)GATE_DEAD;      // GATE_DEAD < gate < 0
      if (__builtin_amdgcn_ballot_w64(general) != 0ull) {
        if (general) {
          // the step of state (p, fd): T(p,1) from the segment's side list, T(p,0) from the flag byte in LDS
          uint32_t has, adv, fdn;
          bool bad = hop > 2u * SEG;
          if (fd != 0u) {
            const uint32_t w = side_word(sl, R1, g0 + rl, p);
            bad = bad || w == R_INVALID;
            has = (w & ID_NONE) != ID_NONE ? 1u : 0u; adv = (w >> 24) & 63u; fdn = (w >> 30) & 1u;
          } else {
            const uint32_t m8 = rowm[SLACK + p];
            has = 1u - ((m8 >> 7) & nounk); adv = m8 & 63u; fdn = (m8 >> 6) & 1u;
          }
          if (bad) { p = seglen; gate = GATE_DEAD; }      // cannot happen on a chain K1/K3 produced (the run's error word said so: ensure_output); the walk ends
          else {
            // staged only while the list can say it (k_emit_list): room in front of the byte being read, a byte consumed, no delete token
            // without a token in front of it
            const bool fits = direct == 0u && slack0 + (int)p - (int)E >= 0 && adv != 0u && !(has == 0u && fdn != 0u);
            if (!fits && direct == 0u) { direct = 1u; staged = E; }      // from here on the segment's spans go straight to HBM
            const uint32_t a = off + p, e = a + adv;
            if (fits && fd == 0u) {
              if (has) rowm[E++] = (uint8_t)p;
              if (fdn) rowm[E++] = (uint8_t)p;
            } else {
              // (the advance of a forward-delete state is not in the plane: its slots go out here and are marked as written - listed all the
              // same, so that the slot behind them has a neighbour to differ from)
              if (has) { if (fits) { smap[E >> 5] |= 1u << (E & 31u); rowm[E] = (uint8_t)p; } put(E, a, e); E++; }
              if (fdn) { if (fits) { smap[E >> 5] |= 1u << (E & 31u); rowm[E] = (uint8_t)p; } put(E, e, e); E++; }
            }
            fd = fdn;
            p += adv;                                                      // (0 is possible: a one-byte alternative of a forward-delete state)
            hop++;
            gate = p < seglen ? slack0 + (int)p - (int)E - (int)((fd | direct) << 16) : GATE_DEAD;
          }
        }
      } else if (__builtin_amdgcn_ballot_w64(gate >= 0) == 0ull) break;                 // no lane can step: every chain has left its segment
    }
    if (direct == 0u) staged = E;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  // second phase: the spans of the listed positions.  A round takes 64 slots of EVERY segment of the tile (k_emit_list): the flag bytes of a round
  // are fetched back to back, then its stores.  Nothing branches before the stores: a lane without a slot reads the last byte of the row
  // and fetches some flag byte of the row (a list entry is a byte: every position it names lies inside the row).
  if (lane < TSL) { s_n[lane] = lane < nv ? staged : 0u; s_base[lane] = t.base; s_off[lane] = off; }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  uint32_t nmax = 0;
#pragma unroll
  for (int s = 0; s < TSL; s++) nmax = max(nmax, s_n[s]);
  nmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)nmax);
  for (uint32_t j0 = 0; j0 < nmax; j0 += 64u) {
    const uint32_t j = j0 + (uint32_t)lane, jj = min(j, (uint32_t)TROW_L - 1u), jp = max(jj, 1u) - 1u;
#pragma unroll 1
    for (int s0 = 0; s0 < TSL; s0 += 8) {
      span_t sv[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int s = s0 + k, ss = s < nv ? s : nv - 1;
        const uint32_t pp = s_m[s][jj], prev = s_m[s][jp];
        const uint32_t adv = flag_byte<FORM>(R0, g0 + (uint64_t)ss, pp) & 63u;
        const uint32_t a = s_off[s] + pp, e = a + adv;
        sv[k].x = (pp == prev && j != 0u) ? e : a;
        sv[k].y = e;
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int s = s0 + k;
        const uint64_t base = s_base[s];
        const bool written = ((s_side[s][jj >> 5] >> (jj & 31u)) & 1u) != 0u;
        if (j < s_n[s] && !written && base + j < total) TM_STREAM_STORE(&out[base + j], sv[k]);
      }
    }
  }
}

// ---- k_collate_spans: the pairs laid out like tm_batch_collate's rows (fill_spans, tm_collate.h, with the plan of one document per row) -------------
template <typename T>
__global__ __launch_bounds__(256) void k_collate_spans(CollateArgs a, Flat f, const uint32_t* __restrict__ spans, T* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  fill_spans<T>(a, f, spans, out, t, [&](uint64_t r) { return row_plan(a, r); });
}

// ---- k_raw_spans: the pairs mapped back through the normalizer ----------------------------------------------------------------------------------------
// Id t of the run, with the normalized pair (nb, ne) of its document d: own[nbegin[d] + n] is the raw offset of the unit that owns normalized
// byte n (the origin pass, tm_norm.hip).  The raw pair is (own(nb), next(ne - 1)) - next(n) the owner of the first byte behind n that has
// another one, or the raw length of the document - and (x, x) with x = next(nb - 1), or 0 at the document's start, for an id without bytes.
// A unit writes a bounded number of bytes, so next() is a short scan.  `in` and `out` may be the same array: a work-item reads and writes its
// own pair only.
__global__ __launch_bounds__(256) void k_raw_spans(const span_t* in, const uint64_t* __restrict__ tok_offsets, uint32_t ndocs,
                                                   const uint64_t* __restrict__ nbegin, const uint64_t* __restrict__ nend, const uint64_t* __restrict__ raw_off,
                                                   const uint32_t* __restrict__ own, uint64_t total, span_t* out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint32_t d = doc_of_id(tok_offsets, ndocs, t);
  const span_t s = in[t];
  const uint64_t nlen = nend[d] - nbegin[d];
  const uint32_t rawlen = (uint32_t)(raw_off[d + 1] - raw_off[d]);
  const uint32_t* __restrict__ o = own + nbegin[d];
  auto next = [&](uint64_t n) {
    const uint32_t me = o[n];
    for (n++; n < nlen; n++) { const uint32_t v = o[n]; if (v != me) return v; }
    return rawlen;
  };
  span_t r;
  if (s.y > s.x && s.y <= nlen) { r.x = o[s.x]; r.y = next((uint64_t)s.y - 1u); }
  else { r.x = (s.x == 0u || s.x > nlen) ? 0u : next((uint64_t)s.x - 1u); r.y = r.x; }
  out[t] = r;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
int spans_ready(const tm_batch* b, const char* who) {
  if (!b->has_output || b->row_form < 0 || b->d_ctl)
    return set_error(TM_E_INVALID, "%s: the batch's ids did not come from a walk (no completed tm_batch_run since the last upload, or tm_batch_load_ids since)", who);
  return TM_OK;
}

// the batch's own buffer (d_spans) for n pairs
static int spans_reserve(tm_batch* b, uint64_t n) { return grow_batch(b, (void**)&b->d_spans, &b->spans_cap, n, n + n / 4 + 1024, 8, "spans"); }

// offsets are 32 bits: no document of the run may be 2^32 bytes or longer.  Only a run of 2^24 segments or more can hold one; then the
// documents' ranges are fetched and looked at (the stream of the run has been waited for).
int spans_check_lengths(tm_batch* b, const char* who) {
  if (b->nseg < (1ull << 32) / SEG) return TM_OK;
  std::vector<uint64_t> lo(b->ndocs), hi(b->ndocs);
  hipError_t e;
  if ((e = hipMemcpy(lo.data(), b->d_doc_begin, (size_t)b->ndocs * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(hi.data(), b->d_doc_end, (size_t)b->ndocs * 8, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "D2H document ranges");
  for (uint32_t d = 0; d < b->ndocs; d++)
    if (hi[d] - lo[d] >= (1ull << 32)) return set_error(TM_E_LIMIT, "%s: document %u has %llu normalized bytes (offsets are 32 bits)", who, d, (unsigned long long)(hi[d] - lo[d]));
  return TM_OK;
}

int batch_spans_on(tm_batch* b, hipStream_t st, void* out, uint64_t total) {
  if (total == 0 || b->nseg == 0) return TM_OK;
  (void)hipGetLastError();
  const uint32_t grid = (uint32_t)((b->nseg + TSL - 1) / TSL);
  const uint32_t stage_after = (debug_flags() & 1024) ? 512u : 0u;      // (test hook 10: every span stored by the walk itself)
  const uint32_t nounk = b->vocab->tables.unk_id != TM_NONE ? 0u : 1u;   // a character without a token leaves no id, hence no slot
  span_t* o = static_cast<span_t*>(out);
  if (b->row_form == 0) TM_LAUNCH(k_span_list<0>, grid, 64, 0, st, b->d_R0, b->d_side, b->d_R1, b->d_seg_par, b->nseg, b->d_seg_doc, b->d_doc_seg_start, total, o, stage_after, nounk);
  else if (b->row_form == 1) TM_LAUNCH(k_span_list<1>, grid, 64, 0, st, b->d_R0, b->d_side, b->d_R1, b->d_seg_par, b->nseg, b->d_seg_doc, b->d_doc_seg_start, total, o, stage_after, nounk);
  else TM_LAUNCH(k_span_list<2>, grid, 64, 0, st, b->d_R0, b->d_side, b->d_R1, b->d_seg_par, b->nseg, b->d_seg_doc, b->d_doc_seg_start, total, o, stage_after, nounk);
  return launch_check();
}

// the raw pairs of the run into `out` (device or page-locked, 8-byte aligned): the normalized pairs into the batch's own buffer, the owners
// (origin pass), then the map
// ms (tm_batch_raw_spans_timed): the three parts between HIP events on `st` - normalized pairs, origin pass, map; synchronizes
int batch_raw_spans_on(tm_batch* b, hipStream_t st, void* out, uint64_t total, uint32_t* host_docs, float* ms) {
  if (host_docs) *host_docs = 0;
  if (ms) ms[0] = ms[1] = ms[2] = 0.f;
  if (total == 0 || b->nseg == 0) return TM_OK;
  EventBracket ev(st, ms ? 4 : 0);
  int rc = TM_OK;
  ev.mark(0);
  // capcode 0 without normalization flags: the normalizer is the identity and so is the map, byte for byte (no rounding to characters)
  const bool identity = b->vocab->host.capcode == 0 && b->vocab->host.norm_flag == 0;
  if (identity) rc = batch_spans_on(b, st, out, total);
  else if ((rc = spans_reserve(b, total)) == TM_OK) rc = batch_spans_on(b, st, b->d_spans, total);
  ev.mark(1);
  if (rc == TM_OK && !identity) rc = origin_pass_on(b, st, host_docs);
  ev.mark(2);
  if (rc == TM_OK && !identity) {
    (void)hipGetLastError();
    TM_LAUNCH(k_raw_spans, grid_of(total), 256, 0, st, reinterpret_cast<const span_t*>(b->d_spans), b->d_tok_offsets, b->ndocs, b->d_doc_begin, b->d_doc_end,
              b->d_raw_off, b->d_own, total, static_cast<span_t*>(out));
    rc = launch_check();
  }
  ev.mark(3);
  return ev.finish(ms, rc);
}

// the ragged pairs of `text` into the batch's own buffer (the raw ones where the normalized ones lay), counted in `unit` (tm_units.hip): what the
// collate and window fills and the one-shot span calls read
int batch_own_spans_on(tm_batch* b, hipStream_t st, uint32_t text, uint32_t unit, uint64_t total) {
  const int rc = spans_reserve(b, total);
  return rc != TM_OK ? rc : batch_spans_in_on(b, st, text, unit, b->d_spans, total, nullptr, nullptr);
}

template <typename T>
static void launch_collate_spans(const CollateArgs& a, const uint32_t* spans, void* out, hipStream_t st) {
  const Flat f = flat_of(out, 2ull * a.rows * a.L, sizeof(T));
  const auto kern = k_collate_spans<T>;
  TM_LAUNCH(kern, grid_of(flat_items(f, sizeof(T))), 256, 0, st, a, f, spans, static_cast<T*>(out));
}

// the one body of tm_batch_collate_spans, tm_batch_collate_raw_spans and tm_batch_collate_spans_in: the ragged pairs of `text` into the batch's own
// buffer, counted in `unit` (tm_units.hip), then the fill
int collate_spans_impl(tm_batch* b, const tm_collate* how, void* stream, uint32_t text, uint32_t unit, void* spans_out, uint32_t span_bytes, const char* who) {
  int rc = check_how(b, how, spans_out, who);
  if (rc != TM_OK) return rc;
  const bool raw = text == TM_TEXT_RAW;
  if (span_bytes != 4 && span_bytes != 8) return set_error(TM_E_INVALID, "%s: span_bytes %u (4 or 8)", who, span_bytes);
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + (how->eos_id != TM_NONE ? 1u : 0u);
  if (how->row_len < ns) return set_error(TM_E_INVALID, "%s: row_len %u holds no %u specials", who, how->row_len, ns);
  if ((uint64_t)how->ndocs * how->row_len > COLLATE_MAX_ELEMS) return set_error(TM_E_LIMIT, "%s: %u rows of %u ids in one call (split the documents)", who, how->ndocs, how->row_len);
  if ((rc = spans_ready(b, who)) != TM_OK || (raw && (rc = origin_ready(b, who)) != TM_OK)) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the rows are all there)
  if (how->ndocs == 0) return TM_OK;
  const uint64_t total = b->last_totals[1];
  hipStream_t st = (hipStream_t)stream;
  if ((rc = spans_check_lengths(b, who)) != TM_OK || (rc = batch_own_spans_on(b, st, text, unit, total)) != TM_OK) return rc;
  (void)hipGetLastError();
  const CollateArgs a{nullptr, b->d_tok_offsets + how->first_doc, how->ndocs, how->row_len, how->pad_id, how->bos_id, how->eos_id, how->flags};
  if (span_bytes == 4) launch_collate_spans<uint32_t>(a, reinterpret_cast<const uint32_t*>(b->d_spans), spans_out, st);
  else launch_collate_spans<uint64_t>(a, reinterpret_cast<const uint32_t*>(b->d_spans), spans_out, st);
  return launch_check();
}

// the one body of tm_batch_spans, tm_batch_raw_spans(_timed) and tm_batch_spans_in: the arguments, then the pairs of `text` in `unit` straight
// into the caller's array.  ms: the four parts of tm_batch_spans_in (may be null)
int ragged_spans_impl(tm_batch* b, void* stream, uint32_t text, uint32_t unit, uint32_t* spans_out, uint64_t spans_cap, uint32_t* host_docs, float* ms, const char* who) {
  if (!b) return set_error(TM_E_INVALID, "%s: null argument", who);
  if (host_docs) *host_docs = 0;
  int rc = units_args(text, unit, who);               // (only tm_batch_spans_in can fail here: the others pass constants)
  if (rc != TM_OK || (rc = spans_ready(b, who)) != TM_OK || (text == TM_TEXT_RAW && (rc = origin_ready(b, who)) != TM_OK)) return rc;
  if (reinterpret_cast<uintptr_t>(spans_out) % 8) return set_error(TM_E_INVALID, "%s: spans_out not aligned to 8 bytes (a pair leaves in one store)", who);
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the rows are all there)
  const uint64_t total = b->ndocs ? b->last_totals[1] : 0;
  if (total > spans_cap) return set_error(TM_E_NOSPACE, "%s: spans_cap %llu < %llu ids", who, (unsigned long long)spans_cap, (unsigned long long)total);
  if (total && !spans_out) return set_error(TM_E_INVALID, "%s: null argument", who);
  if ((rc = spans_check_lengths(b, who)) != TM_OK) return rc;
  return batch_spans_in_on(b, (hipStream_t)stream, text, unit, spans_out, total, host_docs, ms);
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_spans(tm_batch* b, void* stream, uint32_t* spans_out, uint64_t spans_cap) {
  return ragged_spans_impl(b, stream, TM_TEXT_NORMALIZED, TM_UNIT_BYTES, spans_out, spans_cap, nullptr, nullptr, "tm_batch_spans");
}

int tm_batch_collate_spans(tm_batch* b, const tm_collate* how, void* stream, void* spans_out, uint32_t span_bytes) {
  return collate_spans_impl(b, how, stream, TM_TEXT_NORMALIZED, TM_UNIT_BYTES, spans_out, span_bytes, "tm_batch_collate_spans");
}

int tm_batch_raw_spans(tm_batch* b, void* stream, uint32_t* spans_out, uint64_t spans_cap, uint32_t* host_docs) {
  return tm_batch_raw_spans_timed(b, stream, spans_out, spans_cap, host_docs, nullptr);
}

int tm_batch_raw_spans_timed(tm_batch* b, void* stream, uint32_t* spans_out, uint64_t spans_cap, uint32_t* host_docs, float* ms) {
  float parts[4] = {0.f, 0.f, 0.f, 0.f};      // (the caller's array holds three: the unit work of bytes is nothing)
  const int rc = ragged_spans_impl(b, stream, TM_TEXT_RAW, TM_UNIT_BYTES, spans_out, spans_cap, host_docs, ms ? parts : nullptr, "tm_batch_raw_spans");
  if (ms) std::memcpy(ms, parts, 3 * sizeof(float));
  return rc;
}

int tm_batch_collate_raw_spans(tm_batch* b, const tm_collate* how, void* stream, void* spans_out, uint32_t span_bytes) {
  return collate_spans_impl(b, how, stream, TM_TEXT_RAW, TM_UNIT_BYTES, spans_out, span_bytes, "tm_batch_collate_raw_spans");
}

}  // extern "C"

// tm_denoise.hip — tm_batch_collate_denoise: T5 / UL2 span corruption of the rows of tm_batch_collate / tm_batch_collate_select.  Every noise
// span of a row's content shrinks to ONE sentinel in the input row, and the spans stand behind their sentinels in a target row of its own.
// The rule: include/tokenmonster_hip.h.  The selection is tm_batch_collate_masked's (tm_philox.h): keyed by the place g of an id in the
// batch's id buffer, so a seed corrupts a document the same way in any row or batch.
//
// Unlike the masked rows these COMPACT: an entry's column depends on what was selected in front of it.  So the unit of work is the row:
//   - one workgroup of four wavefronts owns a row and walks its content in trips of 256 * PER ids, PER = 16 / sizeof(T) consecutive ids per
//     lane (a row of 512 int64 ids is one trip).  The row's number is uniform, so its plan (doc_index[r], the document's two offsets:
//     row_plan of tm_collate.h) is read once per wavefront with scalar loads;
//   - every lane runs Philox4x32-10 for its PER ids in registers.  The selection is the running maximum of span ends of tm_masked.hip: a
//     six-step scan over the lanes, handed from wavefront to wavefront through four LDS words and from trip to trip in a uniform register.
//     The first trip's seed is recomputed from the up to span_max - 1 ids of the document in front of the row's first (KEEP_TAIL);
//   - two counts per lane - ids selected, span starts - packed into one word are scanned once over the workgroup (registers inside a
//     wavefront, four LDS words between them) and carried across trips.  The third, ids kept, follows from them: the spans are numbered by
//     the count of starts, the noise ends in front of span number sentinel_n, so the ids dropped in front of an id are the ids selected in
//     front of it, or - behind that span's start - the ids selected in front of THAT start.  The one lane that holds that start hands the
//     number over through one more LDS word, in the one trip of a row where it happens;
//   - nothing is scattered to global memory: a trip's input entries and target entries are compacted into two LDS staging buffers, each
//     shifted so that an LDS vector and its global vector begin on the same 16-byte boundary, and leave as 16-byte stores with single
//     elements at an unaligned head and tail;
//   - the same workgroup then writes BOS and EOS, pad_id, label_ignore, the mask bytes and the two lengths.  No atomics: the count of bad
//     rows is k_select_bad's (tm_collate.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tm_pipeline.h"
#include "tm_collate.h"
#include "tm_philox.h"

namespace tmh {

struct DenoiseArgs {
  SelectArgs s;               // s.doc_index null: row r holds document r of s.a.toff (tok_offsets + first_doc), s.run_docs = the rows
  uint32_t key0, key1;        // the seed
  uint32_t span_min, span_n, span_max;      // span_n = span_max - span_min + 1
  uint64_t start_thr;
  uint32_t sent_first, sent_step, sent_n;   // span k: sent_first + k * sent_step (mod 2^32: the host has checked every one)
  uint32_t T;                 // target_len
  uint64_t ignore;            // label_ignore, sign-extended
};

// elements [0, n) of dst = (j < ones ? a : b), by the workgroup's 256 work-items: 16-byte stores between an unaligned head and tail
template <typename T>
__device__ __forceinline__ void row_fill(T* __restrict__ dst, uint32_t n, uint32_t ones, T a, T b, uint32_t tid) {
  constexpr uint32_t PER = 16 / sizeof(T);
  const uintptr_t at = reinterpret_cast<uintptr_t>(dst);
  uint32_t head = n;                                   // (a base that is no multiple of the element size has no vectors at all)
  if (at % sizeof(T) == 0) head = std::min<uint32_t>(n, (uint32_t)(((16 - (at & 15u)) & 15u) / sizeof(T)));
  const uint32_t nvec = (n - head) / PER, singles = n - nvec * PER;
  for (uint32_t v = tid; v < nvec; v += 256) {
    const uint32_t j0 = head + v * PER;
    T vals[PER];
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) vals[k] = j0 + k < ones ? a : b;
    uint4 q;
    __builtin_memcpy(&q, vals, 16);
    *reinterpret_cast<uint4*>(dst + j0) = q;
  }
  for (uint32_t s = tid; s < singles; s += 256) {
    const uint32_t j = s < head ? s : s + nvec * PER;
    dst[j] = j < ones ? a : b;
  }
}

// where entry 0 of a staging buffer stands so that LDS element q and global element dst[q - shift] share their place inside a 16-byte vector
template <typename T>
__device__ __forceinline__ uint32_t stage_shift(const T* dst) {
  return (uint32_t)(reinterpret_cast<uintptr_t>(dst) / sizeof(T)) & (16 / sizeof(T) - 1);
}
// the cnt entries lds[shift .. shift + cnt) -> dst[0 .. cnt): whole vectors where both ends are inside, else element by element
template <typename T>
__device__ __forceinline__ void stage_out(T* __restrict__ dst, const T* lds, uint32_t shift, uint32_t cnt, uint32_t tid) {
  constexpr uint32_t PER = 16 / sizeof(T);
  const bool vec = reinterpret_cast<uintptr_t>(dst) % sizeof(T) == 0;
  const uint32_t stop = shift + cnt;
  for (uint32_t lo = tid * PER; lo < stop; lo += 256 * PER) {
    if (vec && lo >= shift && lo + PER <= stop) {
      uint4 q;
      __builtin_memcpy(&q, lds + lo, 16);
      *reinterpret_cast<uint4*>(dst + (lo - shift)) = q;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < PER; k++)
        if (lo + k >= shift && lo + k < stop) dst[lo + k - shift] = lds[lo + k];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_collate_denoise(DenoiseArgs m, T* __restrict__ ids_out, T* __restrict__ targets, uint8_t* __restrict__ mask_out,
                                                         uint32_t* __restrict__ lengths, uint32_t* __restrict__ tlengths) {
  constexpr uint32_t PER = 16 / sizeof(T), TRIP = 256 * PER;
  __shared__ int32_t s_end[4];                         // a wavefront's largest span end
  __shared__ uint32_t s_cnt[4];                        // a wavefront's ids selected | span starts << 16
  __shared__ uint32_t s_sn;                            // the ids selected in front of span number sent_n
  alignas(16) __shared__ T s_in[TRIP + PER];           // a trip's input entries: at most one per id
  alignas(16) __shared__ T s_tg[2 * TRIP + PER];       // a trip's target entries: at most a sentinel and the id per id
  const CollateArgs& a = m.s.a;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((uint32_t)(threadIdx.x >> 6));
  const uint32_t hb = a.bos != TM_NONE ? 1u : 0u, he = a.eos != TM_NONE ? 1u : 0u;
  const uint32_t N = m.sent_n, tcut = m.T - he;        // tcut: the content entries a target row holds (T >= 1 >= he)
  for (uint64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
    // the row's plan, once per wavefront; t0: where its document begins in the id buffer
    const uint32_t d = m.s.doc_index ? m.s.doc_index[r] : (uint32_t)r;
    const bool good = d < m.s.run_docs;
    T* const in_row = ids_out + r * a.L;
    T* const tg_row = targets ? targets + r * m.T : nullptr;
    uint32_t in_len = 0, tg_len = 0;                   // the entries of the input row; of the target row as it is written
    uint64_t tg_uncut = 0;
    if (good) {
      const RowPlan p = row_plan(a, d);                // (p.lo == 0: no left padding here)
      const uint64_t t0 = a.toff[d];
      const uint32_t n = p.len - hb - he;              // the content ids W = [p.src, p.src + n)
      // the largest end, as a position of the first trip, of the spans that open in front of W: ids t0 .. p.src - 1 stand there
      int32_t carry = NO_END;
      if (n && m.span_max > 1) {
        if (lane + 1 < m.span_max && (uint64_t)lane < p.src - t0) {
          uint32_t w[4];
          philox4x32_10(p.src - 1 - lane, m.key0, m.key1, w);
          const uint32_t reach = reach_of(m, w);
          if (reach) carry = -1 - (int32_t)lane + (int32_t)reach;
        }
        for (int off = 32; off > 0; off >>= 1) carry = std::max(carry, __shfl_xor(carry, off));
      }
      uint32_t selrow = 0, strow = 0, sn = 0;          // in front of the trip: ids selected, span starts; sn: s_sn once span N has opened
      uint32_t in_base = 0;                            // input entries in front of the trip, BOS apart
      uint64_t tg_base = 0;                            // target entries in front of the trip
      for (uint64_t i0 = 0; i0 < n; i0 += TRIP) {
        const uint32_t left = (uint32_t)std::min<uint64_t>(n - i0, TRIP), e0 = tid * PER;
        uint32_t id[PER];
        int32_t end[PER], lane_end = NO_END;
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
          id[k] = 0;
          end[k] = NO_END;
          if (e0 + k < left) {
            const uint64_t g = p.src + i0 + e0 + k;
            id[k] = a.ids[g];
            uint32_t w[4];
            philox4x32_10(g, m.key0, m.key1, w);
            const uint32_t reach = reach_of(m, w);
            if (reach) end[k] = (int32_t)(e0 + k + reach);
            lane_end = std::max(lane_end, end[k]);
          }
        }
        // the largest end in front of this lane's first position: the trips before, the wavefronts before, the lanes before
        int32_t inc = lane_end;
        for (uint32_t off = 1; off < 64; off <<= 1) {
          const int32_t up = __shfl(inc, (int)((lane - off) & 63u));
          if (lane >= off) inc = std::max(inc, up);
        }
        if (lane == 63) s_end[wave] = inc;
        __syncthreads();
        int32_t run = carry, all = carry;
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
          const int32_t v = s_end[w];
          if (w < wave) run = std::max(run, v);
          all = std::max(all, v);
        }
        const int32_t before = __shfl(inc, (int)((lane - 1) & 63u));
        if (lane) run = std::max(run, before);
        carry = std::max(all - (int32_t)TRIP, NO_END);
        // selected: the largest end at or in front of an id lies behind it.  A start: selected, and the id in front is not, or there is none in W
        uint32_t selm = 0, stm = 0;                    // bit k: this lane's id k
        bool prev = run > (int32_t)e0 - 1;
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
          run = std::max(run, end[k]);
          const bool sel = e0 + k < left && run > (int32_t)(e0 + k);
          const bool st = sel && (!prev || (i0 == 0 && e0 + k == 0));
          selm |= (sel ? 1u : 0u) << k;
          stm |= (st ? 1u : 0u) << k;
          prev = sel;
        }
        // the two counts in front of this lane, one scan: at most 2048 of either in a trip
        const uint32_t mine = (uint32_t)__popc(selm) | (uint32_t)__popc(stm) << 16;
        uint32_t sum = mine;
        for (uint32_t off = 1; off < 64; off <<= 1) {
          const uint32_t up = __shfl(sum, (int)((lane - off) & 63u));
          if (lane >= off) sum += up;
        }
        if (lane == 63) s_cnt[wave] = sum;
        __syncthreads();
        uint32_t front = sum - mine, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
          const uint32_t v = s_cnt[w];
          if (w < wave) front += v;
          total += v;
        }
        const uint32_t sel_after = selrow + (total & 0xFFFFu), st_after = strow + (total >> 16);
        // span number N opens in this trip: the noise ends in front of it, and every id behind needs to know where
        if (strow <= N && st_after > N) {
          uint32_t sl = selrow + (front & 0xFFFFu), sb = strow + (front >> 16);
#pragma unroll
          for (uint32_t k = 0; k < PER; k++) {
            if ((stm >> k & 1u) && sb == N) s_sn = sl;
            sl += selm >> k & 1u;
            sb += stm >> k & 1u;
          }
          __syncthreads();
          sn = s_sn;
        }
        // the trip's entries into the staging buffers
        const uint32_t noise_row = strow <= N ? selrow : sn, caps_row = std::min(strow, N);
        const uint32_t noise_after = st_after <= N ? sel_after : sn, caps_after = std::min(st_after, N);
        const uint32_t in_shift = stage_shift(in_row + hb + in_base), tg_shift = tg_row ? stage_shift(tg_row + tg_base) : 0u;
        {
          uint32_t sl = selrow + (front & 0xFFFFu), sb = strow + (front >> 16);      // ids selected, span starts in front of this id
#pragma unroll
          for (uint32_t k = 0; k < PER; k++) {
            const uint32_t sel = selm >> k & 1u, st = stm >> k & 1u;
            if (e0 + k < left) {
              const uint32_t span = sb + st - 1;       // (of a selected id)
              const bool noise = sel && span < N;
              const T sentinel = (T)(m.sent_first + span * m.sent_step);
              if (!noise || st) {
                const uint32_t gone = sb <= N ? sl : sn;      // noise ids in front of this one
                s_in[in_shift + (e0 + k) - (gone - noise_row) + (std::min(sb, N) - caps_row)] = noise ? sentinel : (T)id[k];
              }
              if (noise && tg_row) {                   // (strow < N: tg_base == selrow + strow)
                const uint32_t c = tg_shift + (sl - selrow) + (sb - strow);
                if (st) s_tg[c] = sentinel;
                s_tg[c + st] = (T)id[k];
              }
            }
            sl += sel;
            sb += st;
          }
        }
        __syncthreads();
        const uint32_t in_cnt = left - (noise_after - noise_row) + (caps_after - caps_row);
        const uint32_t tg_cnt = (noise_after - noise_row) + (caps_after - caps_row);
        stage_out<T>(in_row + hb + in_base, s_in, in_shift, in_cnt, tid);
        if (tg_row && tg_base < tcut) stage_out<T>(tg_row + tg_base, s_tg, tg_shift, (uint32_t)std::min<uint64_t>(tg_cnt, tcut - tg_base), tid);
        in_base += in_cnt;
        tg_base += tg_cnt;
        selrow = sel_after;
        strow = st_after;
      }
      in_len = hb + in_base + he;
      tg_uncut = tg_base + he;
      const uint32_t kept = (uint32_t)std::min<uint64_t>(tg_base, tcut);
      tg_len = kept + he;
      if (tid == 0) {
        if (hb) in_row[0] = (T)a.bos;
        if (he) in_row[in_len - 1] = (T)a.eos;
        if (he && tg_row) tg_row[kept] = (T)a.eos;
      }
    }
    // behind the entries, and the per-row outputs
    row_fill<T>(in_row + in_len, a.L - in_len, 0, (T)0, (T)a.pad, tid);
    if (tg_row) row_fill<T>(tg_row + tg_len, m.T - tg_len, 0, (T)0, (T)m.ignore, tid);
    if (mask_out) row_fill<uint8_t>(mask_out + r * a.L, a.L, in_len, 1, 0, tid);
    if (tid == 0) {
      if (lengths) lengths[r] = in_len;
      if (tlengths) tlengths[r] = (uint32_t)std::min<uint64_t>(tg_uncut, 0xFFFFFFFFull);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
static int check_denoise(const tm_denoise* dn, const tm_collate* how, const char* who) {
  constexpr uint64_t ONE = 1ull << 32;
  if (!dn) return set_error(TM_E_INVALID, "%s: null denoising", who);
  if (dn->span_min < 1 || dn->span_min > dn->span_max || dn->span_max > 32)
    return set_error(TM_E_INVALID, "%s: spans of %u .. %u ids (1 <= span_min <= span_max <= 32)", who, dn->span_min, dn->span_max);
  if (dn->start_thr > ONE) return set_error(TM_E_INVALID, "%s: start_thr above 2^32", who);
  if (dn->sentinel_step == 0 || dn->sentinel_n == 0) return set_error(TM_E_INVALID, "%s: sentinel_step 0 or sentinel_n 0", who);
  if (dn->target_len == 0) return set_error(TM_E_INVALID, "%s: target_len 0", who);
  const int64_t top = how->id_bytes == 2 ? 0xFFFF : 0xFFFFFFFFll, last = (int64_t)dn->sentinel_first + (int64_t)(dn->sentinel_n - 1) * dn->sentinel_step;
  if ((int64_t)dn->sentinel_first > top || last < 0 || last > top)
    return set_error(TM_E_INVALID, "%s: sentinels %u .. %lld do not fit %u bytes", who, dn->sentinel_first, (long long)last, how->id_bytes);
  if (how->id_bytes == 2 && (dn->label_ignore < 0 || dn->label_ignore > 0xFFFF)) return set_error(TM_E_INVALID, "%s: label_ignore %d does not fit two bytes", who, dn->label_ignore);
  if (how->flags & TM_COLLATE_PAD_LEFT) return set_error(TM_E_INVALID, "%s: TM_COLLATE_PAD_LEFT (the compacted length is not known before the first store; encoder-decoder models pad right)", who);
  if ((uint64_t)how->ndocs * dn->target_len > COLLATE_MAX_ELEMS)
    return set_error(TM_E_INVALID, "%s: %u rows of %u target ids in one call (split the rows)", who, how->ndocs, dn->target_len);
  return TM_OK;
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_collate_denoise(tm_batch* b, const tm_collate* how, const tm_denoise* dn, const uint32_t* doc_index, void* stream, void* ids_out, void* targets_out,
                             uint8_t* mask_out, uint32_t* lengths_out, uint32_t* target_lengths_out, uint32_t* bad_out) {
  static const char who[] = "tm_batch_collate_denoise";
  if (!how) return set_error(TM_E_INVALID, "%s: null argument", who);
  tm_collate any = *how;                               // (with a list ndocs counts rows, not documents of the run: tm_batch_collate_select)
  if (doc_index) any.ndocs = 0;
  int rc = check_how(b, &any, ids_out, who);
  if (rc != TM_OK || (rc = check_denoise(dn, how, who)) != TM_OK) return rc;
  if (doc_index && how->first_doc != 0) return set_error(TM_E_INVALID, "%s: first_doc %u (the indices count from the run's first document: 0)", who, how->first_doc);
  const uint32_t ns = (how->bos_id != TM_NONE ? 1u : 0u) + (how->eos_id != TM_NONE ? 1u : 0u);
  if ((rc = check_row_room(who, how->row_len, ns, how->ndocs, doc_index ? "rows" : "documents")) != TM_OK) return rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the ids are all there)
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  if (bad_out) launch_select_bad(doc_index, doc_index ? how->ndocs : 0, b->ndocs, bad_out, st);      // (no list: no row is bad)
  if (how->ndocs == 0) return bad_out ? launch_check() : TM_OK;
  DenoiseArgs k;
  k.s = SelectArgs{CollateArgs{b->d_out, b->d_tok_offsets + (doc_index ? 0 : how->first_doc), how->ndocs, how->row_len, how->pad_id, how->bos_id, how->eos_id, how->flags},
                   doc_index, doc_index ? b->ndocs : how->ndocs};
  k.key0 = (uint32_t)dn->seed; k.key1 = (uint32_t)(dn->seed >> 32);
  k.span_min = dn->span_min; k.span_max = dn->span_max; k.span_n = dn->span_max - dn->span_min + 1;
  k.start_thr = dn->start_thr;
  k.sent_first = dn->sentinel_first; k.sent_step = (uint32_t)dn->sentinel_step; k.sent_n = dn->sentinel_n;
  k.T = dn->target_len;
  k.ignore = (uint64_t)(int64_t)dn->label_ignore;
  const uint32_t grid = std::min<uint32_t>(how->ndocs, 1u << 22);      // a workgroup per row; beyond 2^22 rows a workgroup takes several
  with_id_type(how->id_bytes, [&](auto z) {
    using T = decltype(z);
    TM_LAUNCH(k_collate_denoise<T>, grid, 256, 0, st, k, static_cast<T*>(ids_out), static_cast<T*>(targets_out), mask_out, lengths_out, target_lengths_out);
  });
  return launch_check();
}

}  // extern "C"

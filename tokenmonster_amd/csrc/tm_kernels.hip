// tm_kernels.hip — gfx950 kernels of the ungreedy tokenization path and the tm_batch pipeline.
//
// Reference path: go/tokenmonster.go:1017-1279 (Vocab.tokenize).  Restated as a specification in
// SURVEY.md Appendix B; the property everything here rests on (derived from go :1051-1267) is that
// the walk's whole carried state at a token boundary is (i, forwardDelete): `index/length` are always
// the longest match at i (or of ' '+data[i:] when forwardDelete == 1).  Hence
//     T(i, fd) -> (emitted id, advance, fd')
// is a pure function of the text around i and can be evaluated for EVERY byte position independently.
//
// Pipeline (one wavefront owns one <=512-byte document segment; LDS holds its text and the per-position
// second-token descriptors, i.e. the live cursors of all six branches of every position at once):
//   K0 segments      doc -> segment table (binary search per segment)
//   K1 match_branch  per position: longest match (trie walk) and forward-delete match -> descriptors in
//                    LDS; then the 6-branch score/select of go :1068-1262 per (position, fd) -> R[p] = {T(p,0), T(p,1)}
//   K2 link          per segment: follow T from each of the 80 possible entry states to the segment exit
//                    -> exit map (next entry state, #tokens, #forward-deletes, #missing)
//   K3 resolve       per document: chain the exit maps -> entry state + token base of every segment
//   K4 emit          per segment: follow T from the true entry state, write token ids densely
// All integer/byte work: no MFMA.  HBM-side traffic is streaming (text in, R out/in, ids out); the
// vocabulary tables (<= a few MB) live in L2 / Infinity Cache and are the gather-bound part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <type_traits>
#include <vector>

#include "tm_pipeline.h"

namespace tmh {

// R word: id[0..23] | advance[24..29] | fd'[30] | missing[31]

// ------------------------------------------------------------------------------------------------
// small utilities
// ------------------------------------------------------------------------------------------------
// Documents are given as doc_begin[d] .. doc_end[d] (for packed batches doc_end == doc_begin + 1 of the same
// offsets array; for the scoring pass they are arbitrary disjoint strips of the dataset).
// (zero_word: a word this launch clears on the side - the batch's error word - instead of a memset command of its own: a chunk of the
// host-to-host pipeline is some thirty commands, and four lanes' commands queue on one lock of the runtime)
__global__ void k_doc_nseg(const uint64_t* __restrict__ doc_begin, const uint64_t* __restrict__ doc_end, uint32_t ndocs,
                           uint32_t* __restrict__ doc_nseg, uint32_t unit = SEG, uint32_t* __restrict__ zero_word = nullptr) {
  uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (zero_word && d == 0) *zero_word = 0u;
  if (d < ndocs) {
    uint64_t len = doc_end[d] - doc_begin[d];
    doc_nseg[d] = (uint32_t)((len + unit - 1) / unit);
  }
}

// exclusive scan u32 -> u64, three phases, SCAN_CH elements per block

__global__ void k_scan_partial(const uint32_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ block_sums) {
  __shared__ uint64_t s[SCAN_T];
  uint64_t base = (uint64_t)blockIdx.x * SCAN_CH + (uint64_t)threadIdx.x * SCAN_PER;
  uint64_t acc = 0;
  for (int k = 0; k < SCAN_PER; k++) if (base + k < n) acc += in[base + k];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int st = SCAN_T / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) block_sums[blockIdx.x] = s[0];
}

__global__ void k_scan_sums(uint64_t* __restrict__ block_sums, uint32_t nblocks, uint64_t* __restrict__ total) {
  // single workgroup; serial over chunks of SCAN_T
  __shared__ uint64_t s[SCAN_T];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nblocks; base += SCAN_T) {
    uint32_t i = base + threadIdx.x;
    uint64_t v = i < nblocks ? block_sums[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int st = 1; st < SCAN_T; st <<= 1) {
      uint64_t t = (int)threadIdx.x >= st ? s[threadIdx.x - st] : 0;
      __syncthreads();
      s[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nblocks) block_sums[i] = carry + s[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += s[SCAN_T - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ void k_scan_final(const uint32_t* __restrict__ in, uint64_t n, const uint64_t* __restrict__ block_sums,
                             uint64_t* __restrict__ out) {
  __shared__ uint64_t s[SCAN_T];
  uint64_t base = (uint64_t)blockIdx.x * SCAN_CH + (uint64_t)threadIdx.x * SCAN_PER;
  uint32_t v[SCAN_PER];
  uint64_t acc = 0;
  for (int k = 0; k < SCAN_PER; k++) { v[k] = base + k < n ? in[base + k] : 0; acc += v[k]; }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 1; st < SCAN_T; st <<= 1) {
    uint64_t t = (int)threadIdx.x >= st ? s[threadIdx.x - st] : 0;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  uint64_t run = block_sums[blockIdx.x] + s[threadIdx.x] - acc;
  for (int k = 0; k < SCAN_PER; k++) {
    if (base + k < n) out[base + k] = run;
    run += v[k];
  }
  if (base <= n && n < base + SCAN_PER) out[n] = run - 0;  // one-past-the-end = grand total (run == prefix up to n)
}

// K0: segment g belongs to the document d with doc_seg_start[d] <= g < doc_seg_start[d+1]
// (ctl, here and in the kernels below: the control words of a chunk of the host-to-host ring, k_chunk_ctl - when given, the number of segments /
// documents is what the DEVICE has found, ctl[0] / ctl[1], and the kernel argument is only the bound the grid was sized for)
__global__ void k_segments(const uint64_t* __restrict__ doc_seg_start, uint32_t ndocs, uint64_t nseg,
                           uint32_t* __restrict__ seg_doc, const uint64_t* __restrict__ ctl = nullptr) {
  uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ctl) nseg = ctl[0];
  if (g >= nseg) return;
  uint32_t lo = 0, hi = ndocs;   // invariant: start[lo] <= g < start[hi]
  while (hi - lo > 1) {
    uint32_t mid = lo + (hi - lo) / 2;
    if (doc_seg_start[mid] <= g) lo = mid; else hi = mid;
  }
  seg_doc[g] = lo;
}

// exit map of a segment as K3 reads it: next entry state [0..7] | #ids << 8, R_INVALID = the entry state cannot occur (k_match_branch, step C)
__device__ __forceinline__ uint32_t exit_entry(const uint16_t* __restrict__ exit16, const uint32_t* __restrict__ exit_wide, uint64_t idx) {
  const uint32_t x = exit16[idx];
  if (x == 0xFFFFu) return R_INVALID;
  const uint32_t c = x >> 7;
  return c == 511u ? exit_wide[idx] : ((x & 0x7Fu) | (c << 8));
}

// ------------------------------------------------------------------------------------------------
// K1: match + branch
// ------------------------------------------------------------------------------------------------
// While the walks run, D[p] holds the length of the longest match and X[p] its node value.
// Step A2 then folds everything a *second* token contributes to a branch score (go/tokenmonster.go:1075-1084) into the
// final descriptor, so that scoring a branch is a handful of adds instead of re-deriving it six times per state:
//   beginsWithLetter[0] | len[1..6] | beginsOnCapcode[8] | S[9..20]
//   S - 4 = len + allLetters/allPunct + max0(nWords-1) + beginsWithSpace (plain look-up only) + nextIsSpace
//           + (nWords + nextIsNotLetter) * 100 - 3 * (endsWithLetter & nextIsLetter)
// The two cross terms of the penalty need the first token: begins-with-letter and begins-on-capcode sit in bit 0 of bytes 0 and 1,
// so that the penalty is ONE dot product of (descriptor & first-token bits) with the bytes {103, 100} (v_dot4_u32_u8).
constexpr uint32_t D_LEN_SHIFT = 1, D_S_SHIFT = 9, D_NEXT_SPACE = 30, D_HAS_B = 0x80000000u;
__device__ __forceinline__ uint32_t desc_len(uint32_t d) { return (d >> D_LEN_SHIFT) & 63u; }
__device__ __forceinline__ uint32_t make_sdesc(uint32_t len, uint32_t v, uint32_t nb, bool bvariant, uint32_t hint) {
  const uint32_t f5 = v >> 27, snw = (v >> 22) & 31u;
  const int send = (int)(f5 & 1u), sbegl = (int)((f5 >> 1) & 1u), sbegs = (int)((f5 >> 2) & 1u & ~((f5 >> 1) & hint)), sbegc = (int)((f5 >> 3) & 1u),
            sall = (int)((f5 >> 4) & 1u);
  const int S = (int)len + sall + max((int)snw - 1, 0) + (bvariant ? 0 : sbegs) + (int)((nb >> 2) & 1u) + ((int)snw + (int)(nb >> 3)) * 100 -
                (send & (int)(nb & 1u)) * 3;
  // bit 30: the byte behind the token is of the space class (begin_byte 12: the fast exit of go :1057 asks for it when this token is the FIRST
  // of a step); bit 31 (D[] only, set by step A3): the position also has a forward-delete descriptor in Db[] - most do not, and step B then
  // does not look
  return (uint32_t)sbegl | (len << D_LEN_SHIFT) | ((uint32_t)sbegc << 8) | ((uint32_t)(S + 4) << D_S_SHIFT) | (((nb >> 2) & 1u) << D_NEXT_SPACE);
}

// child filter (tm_tables.h): can the node have a child over byte c?
__device__ __forceinline__ bool child_possible32(uint32_t m, uint32_t c) { return bit_of(m, c) != 0u; }

// one in-flight trie walk of a lane: text byte number d of the string being matched is text[tbase + d].
// An idle slot has key == KEY_IDLE (no entry's check word) and gathers the always-empty entry behind the double array,
// so it needs no flag of its own: it never hits, and its bestlen of 0 keeps it from storing anything.
struct Walk { int pos, tbase, depth, limit, bestlen; uint32_t hoff, key, bestv, tw; };      // tw: the chain word of the node the walk stands on, if it has to take a chain next (tm_tables.h), else 0
constexpr uint32_t KEY_IDLE = 0xFFFFFFFDu;
__device__ __forceinline__ bool walk_idle(const Walk& k) { return k.key == KEY_IDLE; }

// consume one probe of the double array: follow the edge, remember the deepest accepting node, arm the next probe or stop
// (pansearch LongestSubstring semantics, tokenmonster.cpp:786-877: longest prefix that is a key).
// Written without branches: every lane executes the same instructions.  `c` is the text byte after the one being matched
// (text[tbase+depth+1]), read from LDS while the probe was in flight.  Returns true when the slot is (or has become) idle.
__device__ __forceinline__ bool walk_consume(const Tables& T, Walk& k, const uint4 e, const uint32_t c) {
  const bool hit = e.x == k.key;
  const uint32_t nid = node_id(e.y);
  k.depth += hit ? 1 : 0;
  const bool acc = hit && nid < T.n_info;
  k.bestv = acc ? e.y : k.bestv;
  k.bestlen = acc ? k.depth : k.bestlen;
  const bool cont = hit && k.depth < k.limit && child_possible32(e.z, c);
  const bool chain = cont && is_tail_word(e.w);            // the node begins a one-child chain: the next round compares the whole chain (walk_chain)
  k.tw = chain ? e.w : 0u;
  k.key = (cont && !chain) ? nid : KEY_IDLE;
  k.hoff = (cont && !chain) ? (e.w + c) << 4 : T.idle_off;
  return !cont;
}

// score of one branch, go/tokenmonster.go:1075-1084 (plain), :1096-1105 (forward-delete variant); alternatives add :1132-1133.
//   fpart  what the candidate first token contributes on its own: flen + allLetters + max0(w-1) + w*100, w = nWords - fd (go :1071,1117,1169)
//   fb     its endsWithLetter (byte 0) and endsOnCapcode (byte 1) bits, lined up with the descriptor's beginsWithLetter / beginsOnCapcode
__device__ __forceinline__ int branch_score(int fpart, uint32_t fb, uint32_t dS, bool bvariant) {
  const int S = (int)((dS >> D_S_SHIFT) & 0xFFFu) - 4;
  // plain: (endsWithLetter & beginsWithLetter) * 103 + (endsOnCapcode & beginsOnCapcode) * 100; forward-delete variant: endsWithLetter * 103 + 1 + ...
  const uint32_t t = (bvariant ? (dS | 1u) : dS) & fb;
  const int pen = (int)__builtin_amdgcn_udot4(t, 0x00006467u, bvariant ? 1u : 0u, false);
  return fpart + S - pen;
}
// go :1132-1133: an alternative's branch that ends short of the greedy token loses 100, one that ends exactly there 10 000
__device__ __forceinline__ int alt_penalty(int flen, uint32_t dS, int len) {
  const int BL = flen + (int)desc_len(dS);
  return (BL < len ? 100 : 0) + (BL == len ? 10000 : 0);
}

// A walk that stands on a node with a chain word and may go on (tm_tables.h, "tails"): compares the next tail_len bytes of text (LDS byte
// address ta) with the chain's string in one go.  Rare - a wavefront meets a handful of them - so all of it sits behind a wave-uniform test at
// the call sites, and the lanes that are not `on` gather the always-empty entry.  Returns whether the lane's walk now stands on the chain's end
// node, with *h = the record's header (link format: node | len << 20, value of the end node or 0, its child filter, its base word).
__device__ __forceinline__ bool tail_compare(const char* __restrict__ tabb, uint32_t idle_off, uint32_t last_rec, bool on, uint32_t word, uint32_t ta, int room, uint4* h) {
  typedef TM_LDS_SPACE_UNALIGNED uint32_t lds_u32u;
  const char* rp = tabb + (on ? (size_t)min(tail_record(word), last_rec) << 4 : (size_t)idle_off);      // (clamped: tm_tables.h, last_rec)
  *h = *reinterpret_cast<const uint4*>(rp);
  const uint4 s0 = *reinterpret_cast<const uint4*>(rp + 16);
  const int len = (int)tail_len(h->x);
  // bytes [0, len) of the string against the text; a dword's bytes at and behind len do not count
  auto differ = [&](uint32_t sw, int k) -> uint32_t {
    const uint32_t tw = *TM_LDS_PTR(lds_u32u, ta + 4u * (uint32_t)k);
    const int nb = len - 4 * k;
    const uint32_t mask = nb >= 4 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u));
    return (tw ^ sw) & mask;
  };
  uint32_t bad = differ(s0.x, 0) | differ(s0.y, 1) | differ(s0.z, 2) | differ(s0.w, 3);
  if (__any(on && len > 16)) {
    const uint4 s1 = *reinterpret_cast<const uint4*>(rp + 32);
    bad |= differ(s1.x, 4) | differ(s1.y, 5) | differ(s1.z, 6) | differ(s1.w, 7);
  }
  return on && bad == 0u && len <= room;
}

struct WaveLds {
  // (arrays of NPOS, not NPOS_PAD, entries: with the 256 bytes of begin_byte[] a workgroup takes exactly 20 KB, 8 workgroups = 32
  // wavefronts per CU fill the 160 KB; the loops over NPOS_PAD positions guard p < NPOS)
  alignas(16) uint32_t X[NPOS];        // node value of D's token (node id = record ordinal)
  alignas(16) uint8_t text[TEXT_LEN];  // (between X and D: D[p] lies 6 * 256 bytes behind X[p], and step A1 stores both with one ds_write2st64_b32)
  uint32_t D[NPOS];        // longest match at p                      (second-token descriptor); Db must follow (step C addresses Db[40..] from D)
  uint32_t Db[NPOS];       // longest match of ' '+text[p:], if usable (forward-delete descriptor), 0 = none
  uint32_t Xb[SEG];        // node value of Db's token
  uint16_t xch[64];        // dense task list of the forward-delete walks (step A3), one batch at a time
};
static_assert(offsetof(WaveLds, D) - offsetof(WaveLds, X) == 6 * 256 && offsetof(WaveLds, Db) == offsetof(WaveLds, D) + 4 * NPOS, "WaveLds layout");

// T(p, fd): go/tokenmonster.go:1051-1276
template <int FD>
__device__ __forceinline__ uint32_t transition(const Tables& T, const WaveLds& w, const uint8_t* s_bb, int p, int dl,
                                               uint32_t d, const Row& O) {
  if (d == 0) return (T.unk_id != TM_NONE ? T.unk_id : ID_NONE) | (1u << 24) | (1u << 31);   // go :1269-1276
  const int len = (int)desc_len(d);
  const uint32_t id = O.x & kRowIdMask;
  const int i1 = p + len;
  uint32_t res = id | ((uint32_t)len << 24);                                                   // go :1265-1267
  if (i1 < dl && ((O.w & (1u << 21)) == 0 || ((d >> D_NEXT_SPACE) & 1u) == 0u)) {               // go :1057 (flag 32: a whole word, followed by a space)
    const int len1 = (int)(O.w & 63u), len2 = (int)((O.w >> 6) & 63u);
    // candidate first tokens: the match itself, alternative 1, alternative 2 (lengths and constants of a forward-delete state: tm_tables.h)
    const int flen[3] = {len, len1 - FD, len2 - FD};
    const int fpart[3] = {len + (int)(O.x >> kRowIdBits) - FD * (100 + (int)((O.w >> 18) & 1u)),
                          (int)(O.y >> kRowIdBits) - FD * (101 + (int)((O.w >> 19) & 1u)),
                          (int)(O.z >> kRowIdBits) - FD * (101 + (int)((O.w >> 20) & 1u))};
    const uint32_t fb[3] = {((O.w >> 12) & 1u) | (((O.w >> 15) & 1u) << 8), ((O.w >> 13) & 1u) | (((O.w >> 16) & 1u) << 8),
                            ((O.w >> 14) & 1u) | (((O.w >> 17) & 1u) << 8)};
    const int nk = len1 == 0 ? 1 : (len2 == 0 ? 2 : 3);                                      // go :1111, :1163
    // the first maximum in the order 1,2,3,1b,2b,3b wins (go :1217-1262): a later score replaces the best only if it is larger
    // within its group, and a forward-delete (b) score only if it is larger than every plain one
    int best = NOSCORE, bestb = NOSCORE;
    uint32_t resb = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (k < nk) {
        const int ik = p + flen[k];
        const uint32_t dS = w.D[ik];
        if (dS != 0) {
          int sc = branch_score(fpart[k], fb[k], dS, false);
          if (k > 0) sc -= alt_penalty(flen[k], dS, len);
          const uint32_t rk = (k == 0 ? id : ((k == 1 ? O.y : O.z) & kRowIdMask)) | ((uint32_t)flen[k] << 24);
          if (sc > best) { best = sc; res = rk; }
          if (dS & D_HAS_B) {
            const uint32_t dB = w.Db[ik];
            int sb = branch_score(fpart[k], fb[k], dB, true);
            if (k > 0) sb -= alt_penalty(flen[k], dB, len);
            if (sb > bestb) { bestb = sb; resb = rk | (1u << 30); }
          }
        }
      }
    }
    if (bestb > best) res = resb;
  }
  return res;
}

// Development switches (per-phase cycle timers, phases of this kernel switched off for profiling) live in tools/devel/tm_devel.h and exist
// only in builds that ask for them (-DTM_DEVEL / -DTM_PHASE_TIMERS: tools/, never the product); here they are these no-ops.
#if defined(TM_DEVEL) || defined(TM_PHASE_TIMERS)
#include "../../tools/devel/tm_devel.h"
#else
#define TM_DBG_ON(x) false
#define PH_INIT
#define PH_INC(i)
#define PH_FLUSH
#define PH(i)
#define PH_COUNT(i, n)
#endif


// Halo sharing (measured -1.7 % alone, -4.9 % together with the non-temporal streams, profiles/r03_k1_variants_ab.txt): the 40 halo positions of a
// segment — 13.5 % of the positions steps A1 - A3 work on — are the first 40 positions of the NEXT segment; when the wavefront of that
// segment sits in the same workgroup and the same document, this wavefront walks 256 positions instead of 296 (runs of 4 instead of 5
// per lane) and copies the neighbour's descriptors after ONE workgroup barrier.  Step C's table of contracted (p,1) hops (J1) therefore
// overlays Db[40..], so that a wavefront never overwrites what its left neighbour may still be copying (D[0..40), Db[0..40)).
// Host model (round 2): 70 % of the wavefronts share, 26.5 -> 24.3 rounds per wavefront in step A1.
// K0: everything k_match_branch has to know about its segment before it can ask for the text, in one 16-byte record, so that a wavefront
// starts with ONE load behind its kernel arguments instead of a chain of five (segment -> document -> ranges -> place of the text):
//   packed text:                 x = begin[0..31]   y = begin[32..39]   z = 0
//   text in the normalizer's slabs (tm_norm.hip): x = the piece the segment begins in   y = the offset of its first byte in that piece's slab
//                                z = the bytes the piece holds from there (piece_off = the pieces' places in the packed text that never was)
//   w = bytes of text from the segment's begin on that may be looked at, clamped to 2^20 [0..20] | positions of the segment [21..29] |
//       the next segment exists and belongs to the same document [30] | text follows the segment's positions [31] (step C)
// The same launch finds the segment's document (seg_doc: K4's records and the span pass read it).  The records live in d_seg_par, which K4's
// parameters (k_seg_params) take over behind K3.  ctl: the number of segments is the device's (a chunk of the host-to-host ring).
constexpr uint32_t SP_DL_BITS = 21, SP_LEN_SHIFT = 21, SP_LEN_BITS = 9, SP_SAME_DOC = 1u << 30, SP_MORE_TEXT = 1u << 31, SP_DL_MAX = 1u << 20;
static_assert(SP_DL_MAX < (1u << SP_DL_BITS) && SEG < (1 << SP_LEN_BITS) && SP_LEN_SHIFT + SP_LEN_BITS == 30, "the packed word of a segment record");
__global__ void k_seg_fill(const uint64_t* __restrict__ doc_seg_start, uint32_t ndocs, const uint64_t* __restrict__ doc_begin, const uint64_t* __restrict__ doc_end,
                           const uint64_t* __restrict__ doc_vis, const uint64_t* __restrict__ doc_piece_start, const uint64_t* __restrict__ piece_off, uint64_t nseg,
                           uint32_t* __restrict__ seg_doc, uint4* __restrict__ seg_src, const uint64_t* __restrict__ ctl = nullptr) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ctl) nseg = ctl[0];
  if (g >= nseg) return;
  uint32_t dl = 0, dh = ndocs;   // invariant: start[dl] <= g < start[dh]
  while (dh - dl > 1) {
    const uint32_t mid = dl + (dh - dl) / 2;
    if (doc_seg_start[mid] <= g) dl = mid; else dh = mid;
  }
  seg_doc[g] = dl;
  const uint64_t begin = doc_begin[dl] + (g - doc_seg_start[dl]) * SEG;
  // A document owns the positions [doc_begin, doc_end) but may LOOK at text up to doc_vis >= doc_end: a byte range of a dataset
  // that is scored as part of the whole-buffer walk (training/trainvocab.go:909-922) sees the text that follows it, and tokens that
  // begin inside the range may end behind it.  For ordinary documents doc_vis == doc_end: the text ends with the document.
  const uint64_t rem = doc_end[dl] - begin, remv = doc_vis[dl] - begin;
  const uint32_t look = remv > (uint64_t)SP_DL_MAX ? SP_DL_MAX : (uint32_t)remv;
  const uint32_t seglen = rem < (uint64_t)SEG ? (uint32_t)rem : (uint32_t)SEG;
  const bool same = g + 1 < nseg && doc_seg_start[dl + 1] > g + 1;
  const uint32_t w = look | (seglen << SP_LEN_SHIFT) | (same ? SP_SAME_DOC : 0u) | (remv > (uint64_t)seglen ? SP_MORE_TEXT : 0u);
  if (doc_piece_start == nullptr) { seg_src[g] = make_uint4((uint32_t)begin, (uint32_t)(begin >> 32) & 0xFFu, 0u, w); return; }
  uint64_t lo = doc_piece_start[dl], hi = doc_piece_start[dl + 1];          // the last piece of the document that begins at or before `begin`
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (piece_off[mid] <= begin) lo = mid; else hi = mid;
  }
  seg_src[g] = make_uint4((uint32_t)lo, (uint32_t)(begin - piece_off[lo]), (uint32_t)(piece_off[lo + 1] - begin), w);
}

constexpr int J_SKIP = NPOS - SEG, J_PLANE = NPOS;     // step C: the contracted hop of state (p, 1) lives at word J_SKIP + J_PLANE + p of {D, Db}
// Walks that leave the loop of step A1: three words a task - base or chain word, node, position | depth << 16 - in the part of Db that nothing
// touches before step A3 (the dump words of streams without positions lie in Db[0..63]; the words used are zeroed again behind the walks, as
// step A3 expects all of Db).  A chain head that finds the list full marks its position in a bitmap (Xb[160..169]; the dump words reach
// Xb[151]) and is walked again from its first byte behind the tasks.
constexpr int TAIL_TASK0 = 64, TAIL_TASKS = (NPOS - TAIL_TASK0) / 3, REDO0 = 160, REDO_WORDS = (NPOS + 31) / 32;
static_assert(REDO0 + REDO_WORDS <= SEG && offsetof(WaveLds, Db) + 4 * 63 + 6 * 256 + 4 <= offsetof(WaveLds, Xb) + 4 * REDO0, "the bitmap lies behind the dump words");
// par: the segment records of k_seg_fill.  slab == nullptr: the text is packed (`text`); else it lies in the normalizer's slabs.
__global__ __launch_bounds__(WAVES * 64, 8) void k_match_branch(Tables T, const uint8_t* __restrict__ text, uint64_t nseg,
                                                                uint32_t* __restrict__ R0, uint2* __restrict__ side,
                                                                uint32_t* __restrict__ R1, uint32_t* __restrict__ exitmap, uint16_t* __restrict__ exit16,
                                                                int narrow, int dbg, const uint8_t* __restrict__ slab, const uint4* __restrict__ par,
                                                                const uint64_t* __restrict__ ctl = nullptr) {
  __shared__ uint8_t s_bb[256];
  __shared__ WaveLds s_wave[WAVES];
  const int lane = threadIdx.x & 63, wvi = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: the segment and its lengths live in SGPRs
  TM_LDS_OBJECTS(s_bb, s_wave);
  PH_INIT
  // The prologue is two dependent rounds of loads, not more: the segment's record (with the device's segment count, where there is one), then
  // every word of its text at once.  A wavefront's life is a chain of memory round trips, and nothing in front of step A1 needs more of them.
  const uint64_t g = (uint64_t)blockIdx.x * WAVES + wvi;
  const uint8_t* const bbp = T.begin_byte;
  const uint4 rec = par[g < nseg ? g : nseg - 1];          // (nseg here: the bound the grid was sized for - a record that exists, whatever the device's count says)
  if (ctl) nseg = ctl[0];
  // (left alone, the compiler fetches a kernel argument where it is first used and the record behind the test of g, a wait each: naming them
  // here has the arguments of the prologue fetched with one wait, and the record asked for beside the device's count.  Behind the two
  // loads, which stay scalar loads only in front of an asm statement.)
  TM_HAVE_IN_SGPRS6(rec.x, rec.w, nseg, text, slab, bbp);
  // begin_byte[] (first read by step A2): every wavefront stores all 256 bytes, a dword per lane, so that it waits for nobody's stores but its
  // own - the four wavefronts write the same values - and the workgroup has no barrier in front of the one behind step A3.  The load is issued
  // here and comes back with the text.
  const uint32_t bbw = reinterpret_cast<const uint32_t*>(bbp)[lane];
  if (g >= nseg) return;
  WaveLds& w = s_wave[wvi];
  const int Lmax = TM_DBG_ON(dbg & 0x180000) ? min((dbg & 0x80000) ? 12 : 20, (int)T.max_len) : (int)T.max_len;      // (devel bits 19 / 20: no walk deeper than 12 / 20 bytes - what the deep tail of step A1 costs)
  const uint32_t idle_off = T.idle_off;                   // the always-empty entry behind the double array
  const uint32_t rw = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.w);
  const int dl = (int)(rw & ((1u << SP_DL_BITS) - 1u));   // bytes of text from the segment's begin on that can be looked at (clamped)
  const int seglen = (int)((rw >> SP_LEN_SHIFT) & ((1u << SP_LEN_BITS) - 1u));  // positions of this segment
  const bool share = wvi + 1 < WAVES && (rw & SP_SAME_DOC) != 0u;      // the next segment is this document's and its wavefront sits in this workgroup (then the text goes on)
  const bool more_text = (rw & SP_MORE_TEXT) != 0u;       // text follows the segment: step C's chains leave it into an entry state

  // stage the text with (unaligned) dword loads; bytes at and after the end of the document read as 0: the pad
  // byte of go/tokenmonster.go:1038-1046 (quirk Q1: we define it as 0 like tokenmonster.cpp:1724-1726)
  // One form for both places of the text: byte i of the segment is byte i of s0 while i < len0 and byte i of s1 behind that.  Packed text is
  // one piece without an end.  In the slabs (one 2 KiB slab per piece of a document, the pieces' bytes never packed: tm_batch_normalize skips
  // its compaction pass, that was 2.2 GB of traffic per GiB for something these loads do on the way) the record names the piece the segment
  // begins in; a piece that is not the last of its document holds at least TEXT_LEN bytes - tm_batch_normalize packs the text after all when
  // one does not -, so two pieces cover what a segment looks at.
  typedef uint32_t __attribute__((aligned(1))) u32u;
  const uint32_t rx = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.x), ry = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.y),
                 rz = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.z);
  const uint8_t *s0, *s1;
  int len0;
  if (slab == nullptr) { s0 = s1 = text + ((uint64_t)rx | ((uint64_t)ry << 32)); len0 = 0x7FFFFFF0; }
  else { s0 = slab + (uint64_t)rx * SLAB_BYTES + ry; len0 = (int)rz; s1 = slab + ((uint64_t)rx + 1) * SLAB_BYTES - len0; }
  // a lane's two words (TEXT_LEN / 4 = 88 over 64 lanes) and, where a word lies across the end of the first piece, the first piece's bytes of
  // it: all of them are asked for before the first is waited for
  static_assert(TEXT_LEN / 4 > 64 && TEXT_LEN / 4 <= 128 && TEXT_LEN % 4 == 0, "two words of text per lane");
  const int i0 = 4 * lane, i1 = 4 * lane + 256;
  const bool h0 = i0 < dl, h1 = i1 < TEXT_LEN && i1 < dl;
  const int n00 = len0 - i0, n01 = len0 - i1;               // bytes of the word that lie in the first piece
  const bool x0 = h0 && n00 > 0 && n00 < 4, x1 = h1 && n01 > 0 && n01 < 4;
  uint32_t tw0 = 0u, tw1 = 0u, twx = 0u;
  // (non-temporal: with ordinary loads the kernel FETCHES 20 % more - the text lines push table lines out of the L2 - at the same time)
  if (h0) tw0 = TM_STREAM_LOAD(reinterpret_cast<const u32u*>((n00 >= 4 ? s0 : s1) + i0));
  if (h1) tw1 = TM_STREAM_LOAD(reinterpret_cast<const u32u*>((n01 >= 4 ? s0 : s1) + i1));
  if (x0 || x1) twx = TM_STREAM_LOAD(reinterpret_cast<const u32u*>(s0 + (x0 ? i0 : i1)));      // (at most one word of a segment)
  // ... and while they are under way: D, Db and the bitmap of step A1 zeroed
  static_assert((2 * NPOS * 4) % 16 == 0 && offsetof(WaveLds, D) % 16 == 0, "D and Db are zeroed as 16-byte words");
  for (int j = lane; j < 2 * NPOS / 4; j += 64) reinterpret_cast<uint4*>(w.D)[j] = make_uint4(0u, 0u, 0u, 0u);      // D and Db
  if (lane < REDO_WORDS) w.Xb[REDO0 + lane] = 0u;
  reinterpret_cast<uint32_t*>(s_bb)[lane] = bbw;
  {
    const uint32_t mx = (1u << (8 * ((x0 ? n00 : n01) & 3))) - 1u;
    if (x0) tw0 = (twx & mx) | (tw0 & ~mx);
    if (x1) tw1 = (twx & mx) | (tw1 & ~mx);
    if (h0 && i0 + 4 > dl) tw0 &= (1u << (8 * (dl - i0))) - 1u;
    if (h1 && i1 + 4 > dl) tw1 &= (1u << (8 * (dl - i1))) - 1u;
    reinterpret_cast<uint32_t*>(w.text)[lane] = tw0;
    if (i1 < TEXT_LEN) reinterpret_cast<uint32_t*>(w.text)[lane + 64] = tw1;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  PH(0)

  // ---- step A: descriptors for every position the segment can look at -----------------------------
  // What bounds this kernel is the number of divergent gathers (every lane of a probe touches its own cache line; the
  // vector memory pipeline retires about one line per clock per CU), so step A1 is built to issue as few of them as
  // possible: a lane owns a RUN of consecutive positions, and once the walk at p has ended on trie node n it does not
  // start over at p+1 but follows the suffix link of n (tm_tables.h) — the state of the walk of text[p+1:] after the
  // bytes already known to match — and only probes for what may come after them.  ~3.1 gathers per position instead of
  // ~4.9 (two-byte map + one probe per further byte).  (pansearch LongestSubstring, call sites go/tokenmonster.go:1049..)
  PH_COUNT(12, 1)
  const int ntask = TM_DBG_ON(dbg & 1) ? 0 : (share ? SEG : min(NPOS, dl));       // positions >= dl keep descriptor 0 (nothing there); a shared halo is the neighbour's work
  // the walks of steps A1 and A3: a lane's state is its key — KEY_SET (A1: the gather is a link-format entry), KEY_IDLE (nothing to
  // do; the gather is the always-empty entry behind the double array), anything else = the node whose child is being probed (the
  // check word the entry must carry)
  constexpr uint32_t KEY_SET = 0xFFFFFFFEu;        // neither is a node id, the x of a link-format entry (depths <= 63 in its top bits: tm_tables.h) or kNone
  static_assert(KEY_IDLE != KEY_SET && KEY_IDLE != kNone && KEY_SET != kNone && (KEY_IDLE >> 26) == 63u && (KEY_SET >> 26) == 63u, "walk states");
  typedef unsigned long long M64;
  const char* __restrict__ tabb = reinterpret_cast<const char*>(T.tab);
  // the walks of a wavefront that go one lane each - the forward-delete probes of step A3, the chain walks behind step A1 - until the last of
  // them has ended: probe rounds (a double-array entry per lane and round) and, rarely, a round for the walks that stand at the head of a
  // one-child chain (tm_tables.h)
  int rw_rounds = 0;                     // (rounds of the walker, for the phase profile of tools/: dead in the product build)
  auto run_walks = [&](Walk& k) {
    while (__any(!walk_idle(k) || k.tw != 0u)) {
      rw_rounds++;
      if (__any(k.tw != 0u)) {
        // a round for the walks that stand at the head of a one-child chain (the others wait it out: rare)
        const bool on = k.tw != 0u;
        uint4 h;
        const bool ok = tail_compare(tabb, idle_off, T.last_rec, on, k.tw, TM_LDS_ADDR(w.text) + (uint32_t)(k.tbase + k.depth), k.limit - k.depth, &h);
        if (on) {
          k.tw = 0u;
          if (ok) {
            k.depth += (int)tail_len(h.x);
            if (h.y != 0u) { k.bestv = h.y; k.bestlen = k.depth; }
            const uint32_t c2 = w.text[k.tbase + k.depth];
            if (k.depth < k.limit && child_possible32(h.z, c2)) {
              if (is_tail_word(h.w)) k.tw = h.w; else { k.key = h.x & kLinkNodeMask; k.hoff = (h.w + c2) << 4; }
            }
          }
        }
        continue;
      }
      const uint4 e = *reinterpret_cast<const uint4*>(tabb + k.hoff);
      const uint32_t c = w.text[k.tbase + k.depth + 1];
      walk_consume(T, k, e, c);
      PH_INC(11)
    }
  };
  {
    // ---- A1: longest match at every position -> D[p] = len | nWords | flag5 (next-byte class added in A2), X[p] = node value
    // A run is in one of two states.  SET: the gather is a link-format entry (a suffix link, or the direct map on the
    // first two bytes when there is nothing to link from) that says where the walk stands — node, depth, best match so
    // far — and whether it can go on.  PROBE: the gather is an edge-hash slot for the next byte.  The round is written
    // as straight-line selects (one instruction costs about a third of a gather here, and branches cost more than the
    // work they skip); the LDS bytes a round may need — the next key byte, the first two bytes of the next position —
    // are read while the gather is in flight.
    // the last byte of a document can only match a one-byte token: no table walk, and it is left out of the runs
    const bool tail_here = !share && dl <= NPOS;                    // the document's last byte is one of this wavefront's positions
    const int nwalkpos = tail_here ? ntask - 1 : ntask;             // positions with at least two bytes of text left
    // Positions are carried as LDS byte addresses of their text byte (one add less per use, and the kernel is VALU bound).
    typedef TM_LDS_SPACE uint8_t lds_u8;
    typedef TM_LDS_SPACE_UNALIGNED uint16_t lds_u16u;
    typedef TM_LDS_SPACE uint32_t lds_u32;
    const uint32_t tb = TM_LDS_ADDR(w.text);                                        // address of text[0]
    const uint32_t xconst = TM_LDS_ADDR(w.X) - 4u * tb;                               // &X[i] == xconst + 4 * (tb + i), &D[i] 6 * 256 bytes behind
    // A lane owns `run` consecutive positions.  The loop is written for NRUN independent streams of consecutive positions per lane whose
    // rounds are interleaved (while the gather of one stream is in flight the lane works on the entry of the other) because round 5 wanted to
    // know whether a wavefront's life - a gather's latency plus ~45 dependent instructions per round, 32 wavefronts per CU - is waiting that a
    // second gather in flight per lane could fill.  It is not: NRUN 2 +14 % / +8 % / +21 % (32 000 / 100 256 / 4 096 ids), NRUN 3 +46 %
    // (profiles/r05_k1_tails.txt (6)): twice the instructions per round and fewer positions that start from a suffix link cost more than the
    // rounds saved - the kernel is bound by what it issues, not by what it waits for.  NRUN stays 1.
#ifndef TM_K1_RUNS
#define TM_K1_RUNS 1
#endif
    constexpr int NRUN = TM_K1_RUNS;
    struct Run { uint32_t posa, pfa, off, key, bestv, node, lasta, c, nn; int depth, limit, bestlen; uint4 e; };
    Run R[NRUN];
    M64 setm[NRUN];
    const int run = (max(nwalkpos, 0) + 63) >> 6;
    const uint32_t dla = tb + (uint32_t)dl;
    {
      const int lo = min(lane * run, max(nwalkpos, 0)), hi = min(lane * run + run, max(nwalkpos, 0));
#pragma unroll
      for (int q = 0; q < NRUN; q++) {
        // stream q: positions [a, b) of the lane's [lo, hi)
        const int a = lo + ((hi - lo) * q + NRUN - 1) / NRUN, b = lo + ((hi - lo) * (q + 1) + NRUN - 1) / NRUN;
        Run& r = R[q];
        r.posa = tb + (uint32_t)a; r.lasta = tb + (uint32_t)b - 1u;
        r.depth = 0; r.limit = 0; r.bestlen = 0; r.pfa = tb; r.off = idle_off; r.key = 0u; r.bestv = 0u; r.node = 0u;
        const bool setting = a < b;
        if (setting) {
          r.limit = min((int)(dla - r.posa), Lmax);
          r.off = T.direct_off + ((uint32_t)*TM_LDS_PTR(lds_u16u, r.posa) << 4);
          r.pfa = r.posa + 2u;
        } else {
          // a stream without positions stores its (0, 0) every round like the others: into Db[lane] and, 6 * 256 bytes behind, Xb[..], which are
          // all zero / not in use before step A3
          static_assert(offsetof(WaveLds, Db) + 4 * 63 + 6 * 256 + 4 <= offsetof(WaveLds, xch) && offsetof(WaveLds, Db) + 6 * 256 >= offsetof(WaveLds, Xb), "dump words");
          r.posa = tb + (uint32_t)((offsetof(WaveLds, Db) - offsetof(WaveLds, X)) / 4) + (uint32_t)lane;
        }
        setm[q] = __builtin_amdgcn_ballot_w64(setting);
      }
    }
    const bool nowalk = TM_DBG_ON((dbg & 4) != 0);
    // The round with its control state as explicit 64-bit lane masks (ballots) and v_cndmask selects on them.  Written this way because
    // the scalar unit, not the vector unit, is the busier issue port of this loop (profiles/r03_k1_issue_ports.txt: one more scalar
    // instruction per round costs 1.6 x one more vector instruction): the structured control flow the compiler builds from `if`s on
    // per-lane booleans — save / restore of exec around every block, mask algebra for every && and || — was ~60 scalar instructions
    // per round, the mask operations below are what the state machine needs.  A stream is SETTING (its gather is a link-format entry: the
    // mask `setm`, carried from round to round), PROBING (a double-array entry, valid if its check word is `key`) or idle (it gathers
    // the always-empty entry, which is nobody's child).
    uint32_t v_link = T.link_off, v_direct = T.direct_off, v_idle = idle_off;
    TM_KEEP_IN_VGPRS2(v_link, v_direct);
    TM_KEEP_IN_VGPRS2(v_idle, v_link);            // operands of the selects: registers for the whole loop, not moves per round
    // (walks that leave the loop go to the task list at Db[TAIL_TASK0], chain heads that find it full to the bitmap at Xb[REDO0]: above the kernel)
    // A walk that is DEFER bytes deep and wants to go on is handed to the task list as well: the deep end of a walk is what a lane's whole run
    // of positions waits for, and behind the loop the deep walks of a wavefront run side by side.  Measured (profiles/r05_k1_tails.txt, K1 per
    // 256 MiB, 32 000 / 100 256 ids): chains only 4.92 / 6.21 ms, DEFER 16: 4.90, 12: 4.85 / 6.14, 10: 4.87 / 6.18, 8: 5.14 / 6.71, 6: 5.31.
#ifndef TM_K1_DEFER_DEPTH
#define TM_K1_DEFER_DEPTH 12
#endif
    constexpr int DEFER = TM_K1_DEFER_DEPTH;
    int ntask_tail = 0;
    bool redo_any = false;                       // (wave-uniform)
    // the gather of a stream's next round and the LDS bytes that round may need - the next key byte, the first two bytes of the next position
    auto issue = [&](Run& r) {
      r.e = *reinterpret_cast<const uint4*>(tabb + r.off);
#ifdef TM_DEVEL
      // (pricing experiments, tools/ builds only: what a second 16-byte load per round costs when it lies in the same 32 bytes / on another line)
      if (dbg & 0x60000) { const uint4 e2 = *reinterpret_cast<const uint4*>(tabb + (r.off ^ ((dbg & 0x20000) ? 16u : 0x1000u))); asm volatile("" :: "v"(e2.x), "v"(e2.y), "v"(e2.z), "v"(e2.w)); }
#endif
      r.c = *TM_LDS_PTR(lds_u8, r.pfa);
      r.nn = *TM_LDS_PTR(lds_u16u, r.posa + 1u);
    };
    auto rounds = [&](auto tail_tag) {
      constexpr bool TAIL = decltype(tail_tag)::value;
      // (The loop exists twice: when the document goes on for at least Lmax bytes behind the last position of the segment, no walk is
      // cut short by the end of the text and `limit` is the constant Lmax.)
      // one round of one stream: its entry has arrived
      auto step = [&](Run& r, M64& setm_r) {
        const M64 busy = __builtin_amdgcn_ballot_w64(r.off != idle_off);
        const uint4 e = r.e;
        const uint32_t c = r.c, nn = r.nn;
        // a double-array entry is the child being probed for iff its check word is the parent (tm_tables.h); a link-format entry always "hits"
        const M64 hit = __builtin_amdgcn_ballot_w64(e.x == r.key) & ~setm_r;
        const M64 adv = hit | setm_r;
        const uint32_t nid = sel_mask(setm_r, e.x, e.y) & kLinkNodeMask;
        r.node = sel_mask(adv, nid, r.node);
        r.depth = (int)sel_mask(setm_r, link_depth(e.x), add_mask_bit((uint32_t)r.depth, hit));
        const M64 acc = hit & __builtin_amdgcn_ballot_w64(nid < T.n_info);
        r.bestv = sel_mask(setm_r | acc, e.y, r.bestv);
        r.bestlen = (int)sel_mask(setm_r, link_bestlen(e.x), sel_mask(acc, (uint32_t)r.depth, (uint32_t)r.bestlen));
        // probe only for a byte the node can continue with: bit (c & 31) of its child filter (0 behind a link that cannot go on)
        M64 go = adv & __builtin_amdgcn_ballot_w64(bit_of(e.z, c) != 0u) & __builtin_amdgcn_ballot_w64(r.depth < (TAIL ? r.limit : Lmax));
        if (nowalk) go = 0ull;
        // one-child chains (tm_tables.h): a walk about to go on from a node with a chain word ENDS here as far as this loop is concerned - the
        // position keeps the best match up to that node, the next position starts from the node's suffix link (valid, if shallower than the
        // link of the node the chain would have led to) - and leaves a task: {chain word, node, position | depth << 16}.  The tasks of a wavefront
        // are walked together behind the loop, one lane each (chain compare, then on as far as the trie goes).  Taking the chains inside the
        // round instead was timed: +11 % (a wavefront then runs the compare in every round in which ANY lane meets a chain).
        const M64 tl = go & __builtin_amdgcn_ballot_w64(is_tail_word(e.w));
        const M64 dm = DEFER > 0 ? (tl | (go & __builtin_amdgcn_ballot_w64(r.depth >= DEFER))) : tl;      // walks that leave this loop for the task list
        if (dm != 0ull) {
          const int nt = __builtin_popcountll(dm);
          if (ntask_tail + nt <= TAIL_TASKS) {
            if ((dm >> lane) & 1ull) {
              const uint32_t slot = mbcnt64(dm, (uint32_t)ntask_tail);
              w.Db[TAIL_TASK0 + 3 * slot] = e.w;
              w.Db[TAIL_TASK0 + 3 * slot + 1] = nid;
              w.Db[TAIL_TASK0 + 3 * slot + 2] = (r.posa - tb) | ((uint32_t)r.depth << 16);
            }
            ntask_tail += nt;
            go &= ~dm;
          } else if (tl != 0ull) {
            // (no room in the list: a walk that is merely deep goes on in the loop; one at the head of a chain cannot - its base word is the
            // chain's record - and marks its position for the walks behind the tasks)
            if ((tl >> lane) & 1ull) atomicOr(&w.Xb[REDO0 + ((r.posa - tb) >> 5)], 1u << ((r.posa - tb) & 31u));
            redo_any = true;
            go &= ~tl;
          }
        }
        const M64 fin = busy & ~go;
        // the best match so far at the stream's position, every round (the last store of a position is its result; a stream that has run out
        // of positions stays on its last one and stores the same values again): no select of a store address, and ONE store for both
        // words (WaveLds: D[p] lies 6 * 256 bytes behind X[p]).  No match: bestlen == 0 and the link formats give bestv == 0.
        {
          TM_LDS_SPACE uint32_t* xp = TM_LDS_PTR(lds_u32, xconst + 4u * r.posa);
          xp[0] = r.bestv;                                                                                      // X[pos]
          xp[6 * 64] = (uint32_t)r.bestlen;                                                                      // D[pos]
        }
        // ... and move on: through the suffix link if the walk got deep enough, else from the direct map
        const M64 more = __builtin_amdgcn_ballot_w64(r.posa < r.lasta), deep = __builtin_amdgcn_ballot_w64(r.depth >= 3);      // (the next position is posa + 1)
        const uint32_t off_f = sel_mask(more, sel_mask(deep, v_link, v_direct) + (sel_mask(deep, r.node, nn) << 4), v_idle);
        // a walk that goes on probes entry base + byte for the byte behind the one just read (also behind a link: it stands for the bytes
        // up to there); the first byte a new position reads: posn + depth - 1 behind a suffix link, posn + 2 behind the direct map
        r.key = sel_mask(go, nid, r.key);
        r.off = sel_mask(go, (e.w + c) << 4, off_f);                             // (an idle stream has no more positions: off_f is the idle entry)
        r.pfa = sel_mask(go, r.pfa + 1u, r.posa + (uint32_t)max(r.depth, 3));
        if (TAIL) r.limit = (int)sel_mask(fin, (uint32_t)min((int)(dla - r.posa) - 1, Lmax), (uint32_t)r.limit);
        setm_r = fin & more;
        r.posa = add_mask_bit(r.posa, setm_r);
        issue(r);
      };
#pragma unroll
      for (int q = 0; q < NRUN; q++) issue(R[q]);
      for (;;) {
        bool any_busy = false;
#pragma unroll
        for (int q = 0; q < NRUN; q++) any_busy |= R[q].off != idle_off;
        if (__builtin_amdgcn_ballot_w64(any_busy) == 0ull) break;
#pragma unroll
        for (int q = 0; q < NRUN; q++) step(R[q], setm[q]);
        PH_INC(8)
      }
    };
    if (dl >= NPOS + Lmax) rounds(std::false_type{}); else rounds(std::true_type{});
    // ---- the chains the walks above stopped at: one lane per task - the chain's string against the text in one round, then on as far as the
    // trie goes (most chains end in a leaf) -, and the position's match replaced if this one is longer
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
    for (int tbase0 = 0; tbase0 < ntask_tail; tbase0 += 64) {
      Walk k = Walk{0, 0, 0, 0, 0, idle_off, KEY_IDLE, 0u, 0u};
      const bool mine = tbase0 + lane < ntask_tail;
      if (mine) {
        const uint32_t bw0 = w.Db[TAIL_TASK0 + 3 * (tbase0 + lane)], nd0 = w.Db[TAIL_TASK0 + 3 * (tbase0 + lane) + 1], pd = w.Db[TAIL_TASK0 + 3 * (tbase0 + lane) + 2];
        k.pos = (int)(pd & 0xFFFFu); k.tbase = k.pos; k.depth = (int)(pd >> 16); k.limit = min(dl - k.pos, Lmax);
        k.bestlen = (int)w.D[k.pos]; k.bestv = w.X[k.pos];
        if (is_tail_word(bw0)) k.tw = bw0;
        else { k.key = nd0; k.hoff = (bw0 + (uint32_t)w.text[k.pos + k.depth]) << 4; }      // (a walk handed over for its depth: it goes on probing)
      }
      run_walks(k);
      if (mine && k.bestlen > (int)w.D[k.pos]) { w.X[k.pos] = k.bestv; w.D[k.pos] = (uint32_t)k.bestlen; }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
    for (int j = lane; j < 3 * ntask_tail; j += 64) w.Db[TAIL_TASK0 + j] = 0u;
    __builtin_amdgcn_wave_barrier();
    PH_COUNT(9, ntask_tail)
    PH_COUNT(10, rw_rounds)
    if (redo_any) {
      // (rare: more chain heads under one wavefront than the task list holds) the marked positions once more, from their first byte: the
      // direct map says where the walk stands after two bytes, the walker does the rest
      __builtin_amdgcn_s_waitcnt(0);
      for (int it = 0; it < NPOS_PAD / 64; it++) {
        const int p0 = it * 64 + lane;
        const bool marked = p0 < NPOS && ((w.Xb[REDO0 + (p0 >> 5)] >> (p0 & 31)) & 1u) != 0u;
        Walk k = Walk{0, 0, 0, 0, 0, idle_off, KEY_IDLE, 0u, 0u};
        if (marked) {
          const uint4 e = *reinterpret_cast<const uint4*>(tabb + T.direct_off + ((uint32_t)*TM_LDS_PTR(lds_u16u, tb + (uint32_t)p0) << 4));
          k.pos = p0; k.tbase = p0; k.depth = (int)link_depth(e.x); k.limit = min(dl - p0, Lmax);
          k.bestlen = (int)link_bestlen(e.x); k.bestv = e.y;
          const uint32_t c0 = w.text[p0 + k.depth];
          if (k.depth < k.limit && child_possible32(e.z, c0)) {
            if (is_tail_word(e.w)) k.tw = e.w; else { k.key = link_node(e.x); k.hoff = (e.w + c0) << 4; }
          }
        }
        if (__any(marked)) {
          run_walks(k);
          if (marked) { w.X[p0] = k.bestv; w.D[p0] = (uint32_t)k.bestlen; }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    // the last byte of a document can only match a one-byte token: no table walk, and it is left out of the runs
    if (lane == 0 && tail_here && ntask > 0) {
      const uint32_t r = T.root[w.text[dl - 1]];
      if (r != kNone && node_id(r) < T.n_info) { w.D[dl - 1] = 1u; w.X[dl - 1] = r; }
    }
    PH(2)
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  // ---- A2: class of the byte after each match; which positions need the forward-delete probe (go :1088) ----------
  // second token begins with a letter, has no word boundary and the byte after it is letter-class
  unsigned long long elig[NPOS_PAD / 64];
  {
    const int off = (int)T.off;
    const bool can_b = T.has_delete && T.bstart != kNone && !TM_DBG_ON(dbg & 8);
#pragma unroll
    for (int it = 0; it < NPOS_PAD / 64; it++) {
      const int p = it * 64 + lane;
      const uint32_t d = (p < NPOS && !(share && p >= SEG)) ? w.D[p] : 0u;      // length of the longest match (step A1)
      bool el = false;
      if (d != 0) {
        const uint32_t v = w.X[p];
        const uint32_t nb = s_bb[w.text[p + d]];
        el = can_b && ((v >> 28) & 1u) && (((v >> 29) & 1u) | (T.spl_hint ^ 1u)) && nb == 1 && node_nwords(v) == 0 && min(dl - p, Lmax - off) > 0;
        w.D[p] = make_sdesc(d, v, nb, false, T.spl_hint);
      }
      elig[it] = __ballot(el);
    }
  }
  PH(4)
  {
    // ---- A3: longest match of ' '+text[p:] at the eligible positions -> Db[p], Xb[p] (accepted only if longer, go :1092)
    // Eligible positions are few, so they are first compacted into a dense list (64 at a time) and every lane runs one
    // walk.  The space-prefix link of the plain match (one gather) stands for the first mainlen+off bytes of that walk,
    // so only the walks that can still grow enter the probe loop.
    const int off = (int)T.off;
    int n_el = 0;
#pragma unroll
    for (int it = 0; it < NPOS_PAD / 64; it++) n_el += __popcll(elig[it]);
    for (int base = 0; base < n_el; base += 64) {
      int run = 0;
#pragma unroll
      for (int it = 0; it < NPOS_PAD / 64; it++) {
        const int dst = (int)mbcnt64(elig[it], (uint32_t)run) - base;                 // (run + the eligible positions below this lane: two v_mbcnt)
        if (((elig[it] >> lane) & 1ull) && dst >= 0 && dst < 64) w.xch[dst] = (uint16_t)(it * 64 + lane);
        run += __popcll(elig[it]);
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0);
      Walk k = Walk{0, 0, 0, 0, 0, idle_off, KEY_IDLE, 0u, 0u};
      int mainlen = 0;
      if (base + lane < n_el) {
        const int p = (int)w.xch[lane];
        const uint32_t ml = desc_len(w.D[p]);
        const uint4 e = T.spl[node_id(w.X[p])];
        const int limit = min(dl - p, Lmax - off) + off;
        const int depth = (int)ml + off;
        const int bl = (int)((e.x >> 22) & 63u);
        const uint32_t c0 = w.text[p + ml];
        // the probe is only walked if the node of ' '+match can go on over the next text byte at all (its child filter): most cannot
        if (e.x != kNone && ((e.x >> 21) & 1u) && depth < limit && child_possible32(e.z, c0)) {
          k.pos = p; k.tbase = p - off; k.bestlen = bl; k.bestv = e.y; k.depth = depth; k.limit = limit;
          mainlen = (int)ml;
          if (is_tail_word(e.w)) k.tw = e.w;                         // (the node of ' '+match begins a one-child chain)
          else { k.key = e.x & kNodeMask; k.hoff = (e.w + c0) << 4; }
        } else if (e.x != kNone && bl > (int)ml + 1) {               // (only possible with the two-byte UTF-16 prefix)
          const int lb = bl - off;
          w.Db[p] = make_sdesc((uint32_t)lb, e.y, s_bb[w.text[p + lb]], true, T.spl_hint);
          w.D[p] |= D_HAS_B;
          if (p < SEG) w.Xb[p] = e.y;
        }
      }
      run_walks(k);
      // a lane walks ONE task per batch: what it found is stored once, after the loop (not in the round in which its walk happens to end)
      if (k.bestlen > mainlen + 1) {
        const int lb = k.bestlen - off;                              // go :1093
        w.Db[k.pos] = make_sdesc((uint32_t)lb, k.bestv, s_bb[w.text[k.pos + lb]], true, T.spl_hint);
        w.D[k.pos] |= D_HAS_B;
        if (k.pos < SEG) w.Xb[k.pos] = k.bestv;
      }
      __builtin_amdgcn_wave_barrier();
    }
    PH_COUNT(14, n_el)
  }
  PH(5)
  __builtin_amdgcn_wave_barrier();
  // the row gathers of step B need only what step A1 has left (X[p]; step A2 has folded the flags into D[p], which stays non-zero where it
  // was): issued here, they are under way while the wavefront waits for its neighbours at the barrier.  (Round 4 issued them before step A3 - 16
  // registers held across it, -2 % on the 100 256-id shape only; with the chain rounds of round 5 in A3 that spilled a row to scratch.)
  Row row0[SEG / 64];
#pragma unroll
  for (int it = 0; it < SEG / 64; it++) {
    const int p = it * 64 + lane;
    row0[it] = Row{0u, 0u, 0u, 0u};
    if (p < seglen && w.D[p] != 0) row0[it] = T.rows[TM_DBG_ON(dbg & 0x10000) ? (node_id(w.X[p]) & 63u) : node_id(w.X[p])];      // (devel bit 16: every row gather hits the same 1 KiB)
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);                    // lgkmcnt(0) only: the LDS stores of this wavefront are done; its row gathers stay in flight
  __syncthreads();                                       // every wavefront of the workgroup has its descriptors
  PH(3)
  if (share && lane < NPOS - SEG) {
    const WaveLds& nx = s_wave[wvi + 1];
    w.D[SEG + lane] = nx.D[lane];
    w.Db[SEG + lane] = nx.Db[lane];
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);

  // ---- step B: T(p,0) and T(p,1) for every position of the segment --------------------------------
  // The kernel is VALU-issue bound (profiles/r01_v3_pmc_k1.txt) and the six-branch scoring is its largest block of
  // straight-line code, so it must not run on mostly idle lanes: T(p,0) is evaluated for all positions (row gathers
  // issued first), but the few (p,1) states (forward-delete matches) are first compacted into a dense list — through
  // the task list of step A3, free by now — and evaluated in as few full-width passes as possible.
  uint32_t r0[SEG / 64], r1[SEG / 64];
  {
    uint32_t d0[SEG / 64];
    unsigned long long m1[SEG / 64];
    int n1 = 0;
#pragma unroll
    for (int it = 0; it < SEG / 64; it++) {
      const int p = it * 64 + lane;
      d0[it] = w.D[p];
      m1[it] = __ballot(p < seglen && w.Db[p] != 0);
      n1 += __popcll(m1[it]);
    }
#pragma unroll
    for (int it = 0; it < SEG / 64; it++) {
      const int p = it * 64 + lane;
      r0[it] = R_INVALID;
      if (p < seglen) r0[it] = TM_DBG_ON(dbg & 0x800000) ? ((row0[it].x & kRowIdMask) | (max(desc_len(d0[it]), 1u) << 24)) : transition<0>(T, w, s_bb, p, dl, d0[it], row0[it]);      // (devel bit 23: greedy, what step B's scoring costs)
    }
    PH(1)
    const bool side_ok = n1 < SIDE_STRIDE && !(dbg & 64);          // (dbg & 64: tests force the dense path)
    for (int base = 0; base < n1; base += 64) {
      int run = 0;
#pragma unroll
      for (int it = 0; it < SEG / 64; it++) {
        const int dst = (int)mbcnt64(m1[it], (uint32_t)run) - base;
        if (((m1[it] >> lane) & 1ull) && dst >= 0 && dst < 64) w.xch[dst] = (uint16_t)(it * 64 + lane);
        run += __popcll(m1[it]);
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0);
      if (base + lane < n1) {
        const int q = (int)w.xch[lane];
        const uint32_t dB = w.Db[q];
        const Row row1 = T.rows[node_id(w.Xb[q])];
        const uint32_t t1 = transition<1>(T, w, s_bb, q, dl, dB, row1);
        w.Xb[q] = t1;                                              // Xb[q] is only ever read by this lane: reuse it for the result
        if (side_ok) side[g * SIDE_STRIDE + 1 + lane] = make_uint2((uint32_t)q, t1);      // (an ordinary store: a few 8-byte entries per segment, not whole lines)
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0);
    }
#pragma unroll
    for (int it = 0; it < SEG / 64; it++) {
      const int p = it * 64 + lane;
      r1[it] = ((m1[it] >> lane) & 1ull) ? w.Xb[p] : R_INVALID;
      if (p < seglen) {
        // rows per SEGMENT (not per text position): every store is whole aligned lines.  With at most 65 536 ids a row is two planes, ids
        // (u16) and advance | fd' | missing (u8): 768 instead of 1 024 bytes of the largest stream this kernel writes (r0_narrow_* below)
        if (narrow == 1) {
          TM_STREAM_STORE(reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(R0) + g * R0_NARROW) + p, (uint16_t)r0[it]);
          TM_STREAM_STORE(reinterpret_cast<uint8_t*>(R0) + g * R0_NARROW + 2 * SEG + p, (uint8_t)(((r0[it] >> 24) & 63u) | ((r0[it] >> 30) << 6)));
        } else if (narrow == 2) {
          TM_STREAM_STORE(reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(R0) + g * R0_WIDE) + p, r0[it] & ID_NONE);
          TM_STREAM_STORE(reinterpret_cast<uint8_t*>(R0) + g * R0_WIDE + 4 * SEG + p, (uint8_t)(((r0[it] >> 24) & 63u) | ((r0[it] >> 30) << 6)));
        } else TM_STREAM_STORE(&R0[g * SEG + p], r0[it]);
        if (!side_ok) TM_STREAM_STORE(&R1[g * SEG + p], r1[it]);   // (rare) too many forward-delete states for the side list
      }
    }
    if (lane == 0) side[g * SIDE_STRIDE] = make_uint2(side_ok ? (uint32_t)n1 : SIDE_DENSE, 0u);
    PH_COUNT(15, n1)
  }
  PH(6)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);                    // lgkmcnt(0) only: step C needs this wavefront's LDS stores, not its stores of R0 / R1 / side

  if (TM_DBG_ON(dbg & 16)) { for (int e = lane; e < ENT; e += 64) exit16[g * ENT + e] = 0u; return; }   // (timing experiments only)
  // ---- step C: exit map of the segment by pointer doubling over the 256 plain states, in registers ----------
  // An entry {#tokens emitted on the way, where the path ends} summarises the path from a state to where it currently points; composing
  // an entry with that of its target doubles the path.  The (p,1) states are few (a forward-delete match) and are contracted out first:
  // each gets the hop that leads through its (.,1) successors to a plain state or out of the segment, and a plain state whose first hop
  // leads into (q,1) takes that contracted hop with it.  What is left are the 256 plain states, state (it * 64 + lane, 0) in ja[it]:
  // a pointer into its own block of 64 positions is a lane index, followed with ds_bpermute, no LDS store.  Every hop consumes at least
  // one byte (only a (p,1) state can stand still, and that is a dead end below), so targets lie strictly ahead: a block first doubles
  // within itself (<= 6 rounds for <= 63 hops), then blocks 2, 1, 0 resolve against the (finished) blocks behind them.
  // (Rounds 2-6 doubled over all 2 x 256 states through a table in LDS, 4 reads + 4 writes and a full wait per round: K1 3.3 % slower.)
  {
    // entry: #tokens [0..JF-1] | field [JF..30] | left-the-segment [31]; the field is the target state (p + SEG * fd) while the path is
    // inside the segment, the entry state of the next segment once it has left it (JNONE: the state is unreachable)
    constexpr uint32_t JF = 12, JCNT = (1u << JF) - 1u, JNONE = (1u << (31 - JF)) - 1u, JOUT = 0x80000000u;
    static_assert(2 * SEG + 2 < 4096, "id count of a segment must fit 12 bits");
    constexpr int N0 = SEG / 64;
    // (in select form: as early returns, the eight calls were branches and exec-mask juggling around every state)
    auto first_hop = [&](uint32_t r, int p, uint32_t fd) -> uint32_t {
      // at/after the end of the segment: nothing is emitted here.  At the end of the text that is the terminal state; in a byte
      // range that is followed by more text, a token of the range before may cover this whole (short, last) segment: pass through
      auto out = [&](uint32_t q, uint32_t f) { return JOUT | ((more_text ? (q - (uint32_t)seglen) * 2u + f : 0u) << JF); };
      const uint32_t pn = (uint32_t)p + ((r >> 24) & 63u), fdn = (r >> 30) & 1u;
      const uint32_t nt = ((r & ID_NONE) != ID_NONE ? 1u : 0u) + fdn;          // ids this step emits: the token (unless it is "none") + the delete token
      const uint32_t xo = out(pn, fdn), xi = (fdn * (uint32_t)SEG + pn) << JF, mo = 0u - (uint32_t)(pn >= (uint32_t)seglen);
      const uint32_t x = ((xo & mo) | (xi & ~mo)) | nt;
      // a state that is its own successor (no byte consumed, same forward-delete flag: a UTF-16 vocabulary with one-byte keys beside the
      // delete token can make one) would never leave the segment: a dead end here; K4, which walks the one chain that is real, reports
      // the text (TM_E_INPUT)
      const bool dead = r == R_INVALID || (fd == 1u && pn == (uint32_t)p && fdn == 1u);
      return p >= seglen ? out((uint32_t)p, fd) : dead ? JOUT | (JNONE << JF) : x;
    };
    auto pend = [](uint32_t x) { return (int)x >= 0; };
    auto bperm = [](uint32_t x, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((x >> JF) & 63u) << 2), (int)v); };     // v at x's target lane
    // 1. the (p,1) states: first hops to LDS (J1 overlays D, dead after step B), then (.,1) -> (.,1) hops composed away in place (rare: a
    // delete token behind a delete token; every entry always describes a valid prefix of its state's chain, so reads and writes of a
    // round may interleave).  Positions strictly increase along such a chain: <= 8 rounds for 256 states.
    uint32_t* J1 = reinterpret_cast<uint32_t*>(w.D) + J_SKIP + J_PLANE;
    static_assert(J_SKIP + J_PLANE + SEG <= 2 * NPOS, "J1 overlay does not fit");
    uint32_t jb[N0], ja[N0];
#pragma unroll
    for (int it = 0; it < N0; it++) {
      const int p = it * 64 + lane;
      jb[it] = TM_DBG_ON(dbg & 0x400000) ? JOUT | (JNONE << JF) : first_hop(r1[it], p, 1u);      // (devel bit 22: no forward-delete states in step C)
      J1[p] = jb[it];
      ja[it] = first_hop(r0[it], p, 0u);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0) only
    for (int round = 0; round < 8; round++) {
      bool any1 = false;
#pragma unroll
      for (int k = 0; k < N0; k++) any1 |= pend(jb[k]) && (jb[k] >> JF) >= (uint32_t)SEG;
      if (__builtin_amdgcn_ballot_w64(any1) == 0ull) break;
#pragma unroll
      for (int k = 0; k < N0; k++)
        if (pend(jb[k]) && (jb[k] >> JF) >= (uint32_t)SEG) { jb[k] = (jb[k] & JCNT) + J1[(jb[k] >> JF) - SEG]; J1[k * 64 + lane] = jb[k]; }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0) only
      PH_INC(13)
    }
    // 2. a plain state whose first hop leads into (q,1) takes q's contracted hop: one LDS read
#pragma unroll
    for (int k = 0; k < N0; k++)
      if (pend(ja[k]) && (ja[k] >> JF) >= (uint32_t)SEG) ja[k] = (ja[k] & JCNT) + J1[(ja[k] >> JF) - SEG];
    // 3. doubling within each block of 64 positions, all four at once, until no state points into its own block (a pending plain entry
    // is < 2^20: its block is x >> (JF + 6))
    for (int round = 0; round < 6; round++) {
      bool anyb = false;
#pragma unroll
      for (int k = 0; k < N0; k++) anyb |= pend(ja[k]) && (ja[k] >> (JF + 6)) == (uint32_t)k;
      if (__builtin_amdgcn_ballot_w64(anyb) == 0ull) break;
#pragma unroll
      for (int k = 0; k < N0; k++) {
        const uint32_t b = bperm(ja[k], ja[k]);
        ja[k] = pend(ja[k]) && (ja[k] >> (JF + 6)) == (uint32_t)k ? (ja[k] & JCNT) + b : ja[k];
      }
      PH_INC(13)
    }
    // 4. blocks 2, 1, 0 against the blocks behind them, which are finished by then (6 ds_bpermute)
#pragma unroll
    for (int k = N0 - 2; k >= 0; k--) {
      uint32_t b = 0u;
#pragma unroll
      for (int j = k + 1; j < N0; j++) {
        const uint32_t bj = bperm(ja[k], ja[j]);
        b = (ja[k] >> (JF + 6)) == (uint32_t)j ? bj : b;
      }
      ja[k] = pend(ja[k]) ? (ja[k] & JCNT) + b : ja[k];
    }
    // 5. the entry states (o, 1), o < 40, that lead into a plain state: contracted hop + that state's resolved entry
    uint32_t e1 = jb[0];
    if (__builtin_amdgcn_ballot_w64(lane < ENT / 2 && pend(e1)) != 0ull) {
      uint32_t b = 0u;
#pragma unroll
      for (int j = 0; j < N0; j++) {
        const uint32_t bj = bperm(e1, ja[j]);
        b = (e1 >> (JF + 6)) == (uint32_t)j ? bj : b;
      }
      e1 = pend(e1) ? (e1 & JCNT) + b : e1;
    }
    // exit map entry (exit_entry below): next entry state [0..6] | #ids << 7 in 16 bits, 0xFFFF: the entry state cannot occur; a count that
    // does not fit 9 bits (more than 510 ids from one 256-byte segment: one-byte tokens with delete tokens) is written as 511 and the
    // segment's map goes to the wide array as well (next entry state [0..7] | #ids << 8, 0xFFFFFFFF).  Lane o writes entries 2o (fd 0), 2o + 1.
    // Test hook 5 (dbg & 32) sends every segment's map that way, as if every count had run over: no text the tests can build from UTF-8
    // reaches 511 ids in a segment, and the resolve kernels must read the wide entries the same.
    const bool all_wide = (dbg & 32) != 0;
    auto ok_of = [](uint32_t a) { return (a >> 31) != 0 && ((a >> JF) & JNONE) != JNONE; };
    auto e16 = [&](uint32_t a) -> uint32_t { return ok_of(a) ? (((a >> JF) & JNONE) | ((all_wide ? 511u : min(a & JCNT, 511u)) << 7)) : 0xFFFFu; };
    // (an ordinary store: a map is 160 bytes, not whole lines, and k_resolve reads it next - measured against the non-temporal store: the
    // kernel writes 0.36 GB less per GiB, k_resolve 0.19 -> 0.14 ms per 256 MiB)
    if (lane < ENT / 2) *reinterpret_cast<uint32_t*>(exit16 + g * ENT + 2 * lane) = e16(ja[0]) | (e16(e1) << 16);
    const bool wide = all_wide || (lane < ENT / 2 && ((ok_of(ja[0]) && (ja[0] & JCNT) >= 511u) || (ok_of(e1) && (e1 & JCNT) >= 511u)));
    if (__any(wide) && lane < ENT / 2) {
      exitmap[g * ENT + 2 * lane] = ok_of(ja[0]) ? ((ja[0] >> JF) & JNONE) | ((ja[0] & JCNT) << 8) : R_INVALID;
      exitmap[g * ENT + 2 * lane + 1] = ok_of(e1) ? ((e1 >> JF) & JNONE) | ((e1 & JCNT) << 8) : R_INVALID;
    }
  }
  PH(7)
  PH_FLUSH
}

// exit map entry (uint32): next entry state [0..7] | #ids emitted << 8 (delete tokens included).  0xFFFFFFFF: entry unreachable.
// Count() (= ids without the delete tokens, quirk Q2) and the missing characters of a document are counted by K4.

// ------------------------------------------------------------------------------------------------
// K3: resolve — per document, chain the exit maps
// ------------------------------------------------------------------------------------------------
// doc_entry (may be null = all 0): the entry state of a document's first segment.  It is 0 for a document; a byte range of a
// dataset that continues the whole-buffer walk of the range before it enters in the state that walk left (tm_score_begin/finish).
__global__ void k_resolve(const uint32_t* __restrict__ exitmap, const uint16_t* __restrict__ exit16, const uint64_t* __restrict__ doc_seg_start, uint32_t ndocs,
                          const uint8_t* __restrict__ doc_entry, uint8_t* __restrict__ seg_entry, uint32_t* __restrict__ seg_tokbase,
                          uint32_t* __restrict__ doc_ntok, uint32_t* __restrict__ error_flag, uint32_t long_segs, uint32_t* __restrict__ doc_fd,
                          uint32_t* __restrict__ doc_missing, const uint64_t* __restrict__ ctl = nullptr) {
  uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (ctl && d < ndocs && ctl[1] == 0) { doc_ntok[d] = 0u; return; }          // (a chunk the ring does not take: no ids)
  if (d >= ndocs) return;
  doc_fd[d] = 0u; doc_missing[d] = 0u;          // (what K4 counts per document starts at zero: no memset commands of their own)
  uint64_t g0 = doc_seg_start[d], g1 = doc_seg_start[d + 1];
  if (g1 - g0 > long_segs) return;               // long documents: k_group_compose / k_long_top / k_group_expand
  uint32_t e = doc_entry ? doc_entry[d] : 0u, ntok = 0;
  for (uint64_t g = g0; g < g1; g++) {
    seg_entry[g] = (uint8_t)e;
    seg_tokbase[g] = ntok;
    const uint32_t x = exit_entry(exit16, exitmap, g * ENT + e);
    if (x == R_INVALID) { atomicOr(error_flag, 1u); break; }
    e = x & 0xFFu;
    ntok += x >> 8;
  }
  doc_ntok[d] = ntok;
}

// Long documents (more than LONG_SEGS segments: a multi-megabyte document, or a strip of the trainvocab dataset) would make
// k_resolve a serial chain of millions of dependent loads.  Their segments hang under a TREE of groups with fan-out GROUP_FAN
// (table built on the host at upload): level-1 groups hold segments, level-k groups hold level-(k-1) groups, until a document has
// at most GROUP_FAN groups at the top.  k_group_compose composes the maps of a group's children for all 80 entry states at once (one
// lane per entry state), level by level; k_long_top chains a document's few top groups; k_group_expand replays every group from its
// now known entry state, top level first.  Every serial chain is GROUP_FAN steps long: a 1 GiB strip (4.5 M segments, 4 levels)
// resolves in well under a millisecond.  Exit-map composition is associative, so the result is the same as the serial chain.
// group map entry (uint2): x = next entry state, y = #ids; x == R_INVALID: unreachable

template <bool LEAF>     // LEAF: the children are segments (exit maps, uint32); otherwise groups of the level below (group maps, uint2)
__global__ __launch_bounds__(128) void k_group_compose(const uint32_t* __restrict__ exitmap, const uint16_t* __restrict__ exit16, const uint2* __restrict__ gmap_in, const Group* __restrict__ groups,
                                                       uint32_t first_group, uint2* __restrict__ gmap) {
  const uint32_t gi = first_group + blockIdx.x;
  const Group gr = groups[gi];
  const uint32_t e0 = threadIdx.x;
  if (e0 >= ENT) return;
  uint32_t e = e0, ntok = 0;
  bool ok = true;
  for (uint32_t k = 0; k < gr.nchildren; k++) {
    if (LEAF) {
      const uint32_t x = exit_entry(exit16, exitmap, (uint64_t)(gr.first_child + k) * ENT + e);
      if (x == R_INVALID) { ok = false; break; }
      e = x & 0xFFu;
      ntok += x >> 8;
    } else {
      const uint2 x = gmap_in[(uint64_t)(gr.first_child + k) * ENT + e];
      if (x.x == R_INVALID) { ok = false; break; }
      e = x.x;
      ntok += x.y;
    }
  }
  gmap[(uint64_t)gi * ENT + e0] = ok ? make_uint2(e, ntok) : make_uint2(R_INVALID, 0u);
}

__global__ void k_long_top(const uint2* __restrict__ gmap, const LongDoc* __restrict__ longs, uint32_t nlong, const uint8_t* __restrict__ doc_entry,
                           uint8_t* __restrict__ group_entry, uint32_t* __restrict__ group_base, uint32_t* __restrict__ doc_ntok,
                           uint32_t* __restrict__ error_flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nlong) return;
  const LongDoc ld = longs[i];
  uint32_t e = doc_entry ? doc_entry[ld.doc] : 0u, ntok = 0;
  for (uint32_t k = 0; k < ld.ngroups; k++) {
    const uint32_t gi = ld.first_group + k;
    group_entry[gi] = (uint8_t)e;
    group_base[gi] = ntok;
    const uint2 x = gmap[(uint64_t)gi * ENT + e];
    if (x.x == R_INVALID) { atomicOr(error_flag, 1u); break; }
    e = x.x;
    ntok += x.y;
  }
  doc_ntok[ld.doc] = ntok;
}

template <bool LEAF>     // one thread per group of the level: hands its entry state and token base down to its children
__global__ void k_group_expand(const uint32_t* __restrict__ exitmap, const uint16_t* __restrict__ exit16, const uint2* __restrict__ gmap, const Group* __restrict__ groups, uint32_t first_group,
                               uint32_t ngroups, uint8_t* __restrict__ group_entry, uint32_t* __restrict__ group_base,
                               uint8_t* __restrict__ seg_entry, uint32_t* __restrict__ seg_tokbase, uint32_t* __restrict__ error_flag) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ngroups) return;
  const uint32_t gi = first_group + t;
  const Group gr = groups[gi];
  uint32_t e = group_entry[gi], ntok = group_base[gi];
  for (uint32_t k = 0; k < gr.nchildren; k++) {
    const uint64_t c = (uint64_t)gr.first_child + k;
    if (LEAF) {
      seg_entry[c] = (uint8_t)e;
      seg_tokbase[c] = ntok;
      const uint32_t x = exit_entry(exit16, exitmap, c * ENT + e);
      if (x == R_INVALID) { atomicOr(error_flag, 1u); break; }
      e = x & 0xFFu;
      ntok += x >> 8;
    } else {
      group_entry[c] = (uint8_t)e;
      group_base[c] = ntok;
      const uint2 x = gmap[c * ENT + e];
      if (x.x == R_INVALID) { atomicOr(error_flag, 1u); break; }
      e = x.x;
      ntok += x.y;
    }
  }
}

// Exit state of a document for EVERY entry state (one thread per entry state): what a rank hands to its neighbours when a dataset is
// scored as byte ranges of ONE whole-buffer walk.  Short documents chain their segments' exit maps, long ones their top groups' maps
// (k_group_compose has composed those for all 80 entry states already).  0xFF: the entry state cannot occur.
__global__ __launch_bounds__(128) void k_doc_exits(const uint32_t* __restrict__ exitmap, const uint16_t* __restrict__ exit16, const uint64_t* __restrict__ doc_seg_start, const uint2* __restrict__ gmap,
                                                   const LongDoc* __restrict__ longs, uint32_t nlong, uint8_t* __restrict__ exits, uint32_t long_segs) {
  const uint32_t d = blockIdx.x, e0 = threadIdx.x;
  if (e0 >= ENT) return;
  const uint64_t g0 = doc_seg_start[d], g1 = doc_seg_start[d + 1];
  uint32_t e = e0;
  bool ok = true;
  if (g1 - g0 > long_segs) {
    uint32_t li = 0;
    while (li < nlong && longs[li].doc != d) li++;
    if (li == nlong) ok = false;
    else {
      const LongDoc ld = longs[li];
      for (uint32_t k = 0; k < ld.ngroups && ok; k++) {
        const uint2 x = gmap[(uint64_t)(ld.first_group + k) * ENT + e];
        if (x.x == R_INVALID) ok = false; else e = x.x;
      }
    }
  } else {
    for (uint64_t g = g0; g < g1 && ok; g++) {
      const uint32_t x = exit_entry(exit16, exitmap, g * ENT + e);
      if (x == R_INVALID) ok = false; else e = x & 0xFFu;
    }
  }
  exits[(uint64_t)d * ENT + e0] = ok ? (uint8_t)e : (uint8_t)0xFF;
}

// The streaming encoder (tm_encoder.hip) between two passes over ONE document that arrives in pieces, on the device: the pass that has
// just run owned the bytes [0, own) of the encoder's text buffer and could look at all `have` of them.
//   entry[0]    <- exits[entry[0]]: the state the walk left the range in is the one the next pass enters in (k_doc_exits' map; `exits` is null
//                  behind the last pass of a document: the next one starts a new document in state 0).  A state that has no exit cannot be
//                  reached by a walk that K3 resolved: K3 has set the error word then, the state goes back to 0.
//   acc[0]      += the characters without a token the pass counted (K4: doc_missing), acc[1] = the state as a word
//   text[0 ..)  <- text[own .. have): the look-ahead of this pass is the beginning of the next one's text.  The ranges overlap when the
//                  pass was a short one, so every thread holds its byte before any is stored (keep <= the workgroup's size).
__global__ __launch_bounds__(256) void k_enc_carry(const uint8_t* __restrict__ exits, uint8_t* __restrict__ entry, const uint32_t* __restrict__ doc_missing,
                                                   uint32_t* __restrict__ acc, uint8_t* __restrict__ text, uint64_t own, uint32_t keep) {
  const uint32_t t = threadIdx.x;
  const uint8_t byte = t < keep ? text[own + t] : (uint8_t)0;
  __syncthreads();
  if (t < keep) text[t] = byte;
  if (t == 0) {
    uint32_t e = 0u;
    if (exits) { e = exits[entry[0]]; if (e >= (uint32_t)ENT) e = 0u; }
    entry[0] = (uint8_t)e;
    acc[0] += doc_missing[0];
    acc[1] = e;
  }
}

// tm_tokenize_document (tm_document.hip): the same step between two pieces of ONE document that lie in DIFFERENT workspaces (slots), so that
// the match kernel of piece k + 1 can run while piece k resolves, emits and downloads.  The document's state lives in one cell of the call:
//   cell[0] = entry state of the next piece, cell[2] = error word (sticky)
// One wavefront, behind this piece's k_match_branch + k_doc_exits and behind the chain kernel of the piece before:
//   entry[0]  <- cell[0]: where this slot's k_resolve looks (tm_batch::d_doc_entry)
//   cell[0]   <- exits[cell[0]] (`exits` null: a piece that owns nothing, the state passes through).  A state without an exit is the walk's
//                dead end (k_resolve would set bit 0 of the error word): it goes into cell[2] and into this slot's error word here, and
//   ctl       <- the slot's control words for the kernels behind (k_resolve .. K4, tm_batch::d_ctl): {nseg, 1 document}, or all zero once
//                cell[2] is set - neither this piece nor any later one emits
//   next_text[0 .. keep) <- text[from .. from + keep): raw input, whose look-ahead cannot be uploaded twice - the last bytes of this slot's
//                normalized text are the first of the next slot's (different buffers: no overlap to mind)
__global__ __launch_bounds__(64) void k_doc_chain(uint32_t* __restrict__ cell, const uint8_t* __restrict__ exits, uint8_t* __restrict__ entry, uint32_t* __restrict__ slot_error,
                                                  uint64_t* __restrict__ ctl, uint64_t nseg, const uint8_t* __restrict__ text, uint64_t from, uint32_t keep,
                                                  uint8_t* __restrict__ next_text) {
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < keep; i += 64u) next_text[i] = text[from + i];
  if (t != 0) return;
  uint32_t e = cell[0], err = cell[2];
  if (e >= (uint32_t)ENT) { e = 0u; err |= 2u; }
  uint32_t x = e;
  if (exits && !err) { x = exits[e]; if (x >= (uint32_t)ENT) { x = 0u; err |= 1u; } }
  entry[0] = (uint8_t)e;
  cell[0] = x;
  cell[2] = err;
  if (err) *slot_error = *slot_error | err;
  ctl[0] = err ? 0ull : nseg;
  ctl[1] = err ? 0ull : 1ull;
  ctl[2] = 0ull;
  ctl[3] = err ? (uint64_t)RING_ERROR : 0ull;
  ctl[4] = 0ull;
  ctl[5] = 0ull;
}

// Count() of a document = its ids without the delete tokens (go/tokenmonster.go:1281, quirk Q2): K3 knows the ids, K4 the delete tokens
__global__ void k_doc_events(const uint32_t* __restrict__ doc_ntok, const uint32_t* __restrict__ doc_fd, uint32_t ndocs, uint32_t* __restrict__ doc_events) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < ndocs) doc_events[d] = doc_ntok[d] - doc_fd[d];
}

// ------------------------------------------------------------------------------------------------
// K4: emit ids (or, HIST, accumulate the trainvocab histogram, training/trainvocab.go:1105-1174)
// ------------------------------------------------------------------------------------------------
// hist layout (all uint32, so that one RCCL all-reduce(sum) merges ranks): scores[n_ids] | tokens_in_text as
// four 16-bit limbs | missing[256] (per-byte counters, > 0 = that byte had no token)
// The scoring variant keeps most of the histogram traffic in LDS: persistent workgroups (one per CU) own a two-way
// set-associative table of HSLOTS counters {id << 32 | bytes}.  An id that finds itself in its set adds in LDS; one that does
// not takes the way with the smaller count if that count is still below HSTICKY (the evicted counter is flushed with one global
// atomic) and otherwise falls through to a global atomic itself: hot ids become sticky after a few occurrences, whichever id
// came first, and only the cold ids of a set — spread over many addresses — go to the L2.  (A direct-mapped first-come table
// left 4.2 of the kernel's 8.2 ms in global atomics on a 65 536-id vocabulary: eight ids per slot, the hottest not always the
// owner, and atomics on one address serialise in the L2.)  Counters are flushed when the workgroup retires.
constexpr int HSLOTS = 8192;
constexpr uint32_t HSTICKY = 512;
constexpr unsigned long long HEMPTY = 0xFFFFFFFF00000000ull;
__device__ __forceinline__ void hist_add(unsigned long long* s_w, uint32_t* __restrict__ scores, uint32_t id, uint32_t adv) {
  unsigned long long* set = s_w + 2u * ((id * 0x9E3779B1u) >> (32 - 12));
  static_assert(HSLOTS == 2 << 12, "set index is 12 bits");
  for (;;) {
    const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(set);
    const uint32_t t0 = (uint32_t)(w.x >> 32), t1 = (uint32_t)(w.y >> 32), c0 = (uint32_t)w.x, c1 = (uint32_t)w.y;
    if (t0 == id || t1 == id) {
      const int way = t0 == id ? 0 : 1;
      const unsigned long long old = way ? w.y : w.x;
      // a sticky counter can no longer change hands: plain add (same-address adds of a wavefront are serialised by the LDS, no retries)
      if ((uint32_t)old >= HSTICKY) { atomicAdd(&set[way], (unsigned long long)adv); return; }
      if (atomicCAS(&set[way], old, old + adv) == old) return;
      continue;
    }
    const int way = c1 < c0 ? 1 : 0;
    const unsigned long long old = way ? w.y : w.x;
    if ((uint32_t)old >= HSTICKY) { atomicAdd(&scores[id], adv); return; }          // both ways are hot ids
    if (atomicCAS(&set[way], old, ((unsigned long long)id << 32) | adv) == old) {
      if ((uint32_t)old != 0) atomicAdd(&scores[(uint32_t)(old >> 32)], (uint32_t)old);
      return;
    }
  }
}

// The same for ids below 65 536 (k_score_list: the two-plane rows), twice as many counters in the same 64 KB and four ways to a set: a counter
// is ONE word - the id's top four bits | 28 bits of count - in the set its low twelve bits name, so a set is 16 bytes, read with one load, and
// holds four of the sixteen ids that share it.  (With two ways of {id, count} pairs four ids in ten found no counter: a hot id keeps its way for
// the whole pass, and 8 192 ids do not fall evenly into 4 096 sets of two - and every miss is a transaction of its own on the way to HBM,
// 1.9 of the 2.7 ms the histogram cost per GiB: profiles/r06_k4.txt.)  A count cannot run over: 28 bits hold every byte a CU sees in a pass.
constexpr int H16_SETS = 4096;
constexpr uint32_t H16_CNT = 0x0FFFFFFFu;
__device__ __forceinline__ void hist16_add(uint32_t* s_h, uint32_t* __restrict__ scores, uint32_t id, uint32_t adv) {
  uint32_t* set = s_h + 4u * (id & (uint32_t)(H16_SETS - 1));
  const uint32_t tag = id >> 12, base_id = id & (uint32_t)(H16_SETS - 1);
  for (;;) {
    const uint4 w = *reinterpret_cast<const uint4*>(set);
    const uint32_t e[4] = {w.x, w.y, w.z, w.w};
    int way = -1, victim = 0;
    uint32_t vc = e[0] & H16_CNT;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t c = e[k] & H16_CNT;
      if (c != 0u && (e[k] >> 28) == tag) way = k;
      if (c < vc) { vc = c; victim = k; }
    }
    if (way >= 0) {
      const uint32_t old = e[way];
      // a sticky counter can no longer change hands: plain add (same-address adds of a wavefront are serialised by the LDS, no retries)
      if ((old & H16_CNT) >= HSTICKY) { atomicAdd(&set[way], adv); return; }
      if (atomicCAS(&set[way], old, old + adv) == old) return;
      continue;
    }
    if (vc >= HSTICKY) { atomicAdd(&scores[id], adv); return; }          // all four ways are hot ids
    const uint32_t old = e[victim];
    if (atomicCAS(&set[victim], old, (tag << 28) | adv) == old) {
      if (vc != 0u) atomicAdd(&scores[((old >> 28) << 12) | base_id], vc);
      return;
    }
  }
}

// K4 as a chain walk through LDS tiles (a parallel list ranking of all 512 states of a segment, of which ~60 are on the chain,
// was measured at 5.5 ms per GiB against 3.3 for this walk and has been removed).  A wavefront takes TS consecutive segments: their T(p,0) words are streamed into LDS
// with full-width 16-byte loads, then lane s simply follows the chain of segment s through its row (one dependent LDS read and
// ~15 instructions per token, for 16 segments at once).  The ids are staged in the part of the row the walk has already left
// and leave in coalesced stores.  The kernel is bound by the latency of the walk, i.e. by how many rows fit the LDS of a CU.
// (p,1) states are rare: their words are looked up in the segment's side list (or the dense array) when one is entered.
// (Letting every lane walk its segment straight from HBM — no tiles — was measured at 8.5 ms per GiB: ~0.6 G scattered 4-byte
// accesses cost ~8 cycles each per CU.)
constexpr int TS = 8;                       // segments per wavefront (8: 18 wavefronts per CU; 16 was 8 % slower, the phases of a tile overlap less)
constexpr int TSLACK = 2;               // position p of a row is word TSLACK + p: the two ids of a first token fit in front of it
constexpr int TROW = SEG + 8;           // words per tile row (16-byte multiple; the odd multiple of 8 spreads the rows over the LDS banks)

// k_seg_params: everything K4 needs to know about a segment in one 16-byte record, so that a tile starts with ONE round of loads
// instead of a chain of three (segment -> document -> offsets):
//   x = begin[0..31]   y = begin[32..39] | seglen << 8 (12 bits) | entry state << 20 (7 bits)   z, w = first output index (64 bit)
// Record nseg holds the end of the output stream.
__global__ void k_seg_params(const uint64_t* __restrict__ doc_begin, const uint64_t* __restrict__ doc_end, const uint32_t* __restrict__ seg_doc,
                             const uint64_t* __restrict__ doc_seg_start, uint64_t nseg, uint32_t ndocs, const uint8_t* __restrict__ seg_entry,
                             const uint32_t* __restrict__ seg_tokbase, const uint64_t* __restrict__ tok_offsets, uint4* __restrict__ par,
                             const uint64_t* __restrict__ ctl = nullptr) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ctl) nseg = ctl[0];
  if (g > nseg) return;
  if (g == nseg) { const uint64_t total = tok_offsets[ndocs]; par[g] = make_uint4(0u, 0u, (uint32_t)total, (uint32_t)(total >> 32)); return; }
  const uint32_t doc = seg_doc[g];
  const uint64_t begin = doc_begin[doc] + (g - doc_seg_start[doc]) * SEG;
  const uint64_t rem = doc_end[doc] - begin;
  const uint32_t seglen = rem > (uint64_t)SEG ? (uint32_t)SEG : (uint32_t)rem;
  const uint64_t base = tok_offsets[doc] + seg_tokbase[g];
  par[g] = make_uint4((uint32_t)begin, (uint32_t)((begin >> 32) & 0xFFu) | (seglen << 8) | ((uint32_t)seg_entry[g] << 20), (uint32_t)base, (uint32_t)(base >> 32));
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32);
}
// stream the T(p,0) words of the tile's segments into LDS, position p of segment s at tile[s][TSLACK + p]: lane l fetches words
// 4l..4l+3 of a row with one aligned 16-byte load (segment g owns words [g * SEG, (g + 1) * SEG) of R0, so a tile is one contiguous
// block).  All loads are issued before the first LDS write, so a tile costs one HBM latency, not sixteen.
// narrow != 0: the rows are in the two-plane form (R0_NARROW bytes per segment); `no_id` is the id a missing character gets (the unk token, or none)
__device__ __forceinline__ void tile_load(uint32_t (*tile)[TROW], const TileSeg& t, uint64_t g0, int nv, int lane, const uint32_t* __restrict__ R0, int narrow, uint32_t no_id) {
  if (narrow) {
    static_assert(SEG == 256, "one 8-byte + one 4-byte load per lane fetch a narrow row");
    uint2 va[TS];
    uint32_t vb[TS];
#pragma unroll
    for (int s = 0; s < TS; s++) {
      const int ss = s < nv ? s : nv - 1;
      const uint8_t* row = reinterpret_cast<const uint8_t*>(R0) + (g0 + (uint64_t)ss) * R0_NARROW;
      const uint32_t len = s < nv ? (uint32_t)__shfl((int)t.seglen, ss) : 0u;
      va[s] = make_uint2(0u, 0u); vb[s] = 0u;
      if (4u * (uint32_t)lane < len) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 q = TM_STREAM_LOAD(reinterpret_cast<const u32x2*>(row) + lane);
        va[s] = make_uint2(q.x, q.y);
        vb[s] = TM_STREAM_LOAD(reinterpret_cast<const uint32_t*>(row + 2 * SEG) + lane);
      }
    }
#pragma unroll
    for (int s = 0; s < TS; s++) {
      uint32_t w4[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t id16 = ((q < 2 ? va[s].x : va[s].y) >> (16 * (q & 1))) & 0xFFFFu, m8 = (vb[s] >> (8 * q)) & 0xFFu;
        const uint32_t id = (m8 >> 7) ? no_id : id16;              // (a character without a token carries the unk id, or none)
        w4[q] = id | ((m8 & 63u) << 24) | ((m8 >> 6) << 30);
      }
      uint2* dst = reinterpret_cast<uint2*>(&tile[s][TSLACK + 4 * lane]);
      dst[0] = make_uint2(w4[0], w4[1]);
      dst[1] = make_uint2(w4[2], w4[3]);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
    return;
  }
  constexpr int PARTS = SEG / 256;                                       // a row is fetched 256 words (one 16-byte load per lane) at a time
  static_assert(SEG % 256 == 0, "tile_load fetches rows in units of 256 words");
  uint4 v[TS][PARTS];
  const uint32_t* src[TS];
  uint32_t len[TS];
#pragma unroll
  for (int s = 0; s < TS; s++) {
    const int ss = s < nv ? s : nv - 1;                                // rows beyond the last segment: nothing is fetched
    src[s] = R0 + (g0 + (uint64_t)ss) * SEG + 4 * lane;
    len[s] = s < nv ? (uint32_t)__shfl((int)t.seglen, ss) : 0u;
  }
#pragma unroll
  for (int s = 0; s < TS; s++)
#pragma unroll
    for (int h = 0; h < PARTS; h++) {
      v[s][h] = make_uint4(0u, 0u, 0u, 0u);
      if (4u * (uint32_t)lane + 256u * h < len[s]) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 q = TM_STREAM_LOAD(reinterpret_cast<const u32x4*>(src[s] + 256 * h));
        v[s][h] = make_uint4(q.x, q.y, q.z, q.w);
      }
    }
#pragma unroll
  for (int s = 0; s < TS; s++)
#pragma unroll
    for (int h = 0; h < PARTS; h++) {                                    // TSLACK = 2: the row is 8-byte, not 16-byte, aligned
      uint2* dst = reinterpret_cast<uint2*>(&tile[s][TSLACK + 4 * lane + 256 * h]);
      dst[0] = make_uint2(v[s][h].x, v[s][h].y);
      dst[1] = make_uint2(v[s][h].z, v[s][h].w);
    }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
}

// NARROW: the rows are in the two-plane form (k_match_branch: u16 ids, u8 advance | fd' | missing) and stay that way in LDS - 6 instead of
// 8 KB per tile, a third more walking lanes per CU, and no words to rebuild; an id is staged as 16 bits and widened on the way out.
constexpr int TSLACK_N = 4, TROW_N = SEG + 16;        // narrow tile row: position p at index TSLACK_N + p of both planes
template <bool NARROW>
__global__ __launch_bounds__(64) void k_emit_tiles(const uint32_t* __restrict__ R0, const uint2* __restrict__ side,
                                                   const uint32_t* __restrict__ R1, const uint4* __restrict__ par, uint64_t nseg,
                                                   uint32_t delete_id, uint64_t out_cap, uint32_t* __restrict__ out,
                                                   uint32_t* __restrict__ error_flag, uint32_t stage_after, const uint32_t* __restrict__ seg_doc,
                                                   uint32_t* __restrict__ doc_fd, uint32_t* __restrict__ doc_missing, uint32_t no_id,
                                                   const uint64_t* __restrict__ ctl = nullptr) {
  alignas(16) __shared__ uint32_t s_tile[NARROW ? 1 : TS][NARROW ? 4 : TROW];
  alignas(16) __shared__ uint16_t s_a[NARROW ? TS : 1][NARROW ? TROW_N : 8];
  alignas(16) __shared__ uint8_t s_m[NARROW ? TS : 1][NARROW ? TROW_N : 16];
  const int lane = threadIdx.x;
  const uint64_t g0 = (uint64_t)blockIdx.x * TS;
  if (ctl) { nseg = ctl[0]; if (g0 >= nseg) return; }
  const int nv = (int)(nseg - g0 < (uint64_t)TS ? nseg - g0 : (uint64_t)TS);
  const TileSeg t = tile_segment(par, g0 + lane, lane < TS, nseg);
  constexpr uint32_t SLACK = NARROW ? TSLACK_N : TSLACK;
  if constexpr (NARROW) {
    // lane l fetches positions 4l .. 4l+3 of every row: 8 bytes of ids, 4 bytes of advance / flags; all loads before the first LDS write
    uint2 va[TS];
    uint32_t vb[TS];
#pragma unroll
    for (int s = 0; s < TS; s++) {
      const int ss = s < nv ? s : nv - 1;
      const uint8_t* rowg = reinterpret_cast<const uint8_t*>(R0) + (g0 + (uint64_t)ss) * R0_NARROW;
      const uint32_t len = s < nv ? (uint32_t)__shfl((int)t.seglen, ss) : 0u;
      va[s] = make_uint2(0u, 0u); vb[s] = 0u;
      if (4u * (uint32_t)lane < len) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 q = TM_STREAM_LOAD(reinterpret_cast<const u32x2*>(rowg) + lane);
        va[s] = make_uint2(q.x, q.y);
        vb[s] = TM_STREAM_LOAD(reinterpret_cast<const uint32_t*>(rowg + 2 * SEG) + lane);
      }
    }
#pragma unroll
    for (int s = 0; s < TS; s++) {
      *reinterpret_cast<uint2*>(&s_a[s][TSLACK_N + 4 * lane]) = va[s];
      *reinterpret_cast<uint32_t*>(&s_m[s][TSLACK_N + 4 * lane]) = vb[s];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
  } else {
    tile_load(s_tile, t, g0, nv, lane, R0, 0, no_id);
  }
  // Walk.  Id number E of the segment is staged in slot E of its own row while that slot lies before the position being read
  // (E < SLACK + p: true unless the text averages more than one id per byte); from the first id that does not fit, the rest of
  // the segment's ids go straight to HBM.  (stage_after = 0; the tests pass 512 so that nothing is staged: debug bit 10.)
  // The walk is ONE loop of the wavefront with two kinds of step.  The common one — a (p, 0) state whose ids still fit in front of the word
  // being read — is straight-line code under a single lane mask: both staging stores are unconditional (slot E, then slot E + has-an-id;
  // both lie before the position being read, and a slot that was not meant is overwritten by the next id or lies behind the count).
  // Everything else — a forward-delete state (T(p,1) comes from the side list in HBM), a segment whose ids have caught up with its
  // words, the test hook — takes the general step, which the wavefront only enters when one of its lanes needs it.  (As nested per-lane
  // loops with a branch per store this was ~100 instructions per step, 60 of them scalar: the walk is bound by instruction issue, 8 lanes at a time.)
  uint32_t staged = 0;
  {
    const int rl = lane & (TS - 1);                                      // (lanes >= TS have no segment; they only need valid pointers)
    uint32_t* row = s_tile[NARROW ? 0 : rl];
    uint16_t* rowa = s_a[NARROW ? rl : 0];
    const uint8_t* rowm = s_m[NARROW ? rl : 0];
    const uint2* __restrict__ sl = side + (g0 + rl) * SIDE_STRIDE;
    uint32_t nfd = 0, nmiss = 0;                                       // delete tokens emitted / characters without a token (go :1274)
    // the word of state (p, fd): T(p,0) from the tile, T(p,1) from the segment's side list
    auto word = [&](uint32_t pp, uint32_t f) -> uint32_t {
      if (f != 0) return side_word(sl, R1, g0 + rl, pp);
      if (!NARROW) return row[SLACK + pp];
      const uint32_t m8 = rowm[SLACK + pp], i16 = rowa[SLACK + pp];
      return ((m8 >> 7) ? no_id : i16) | ((m8 & 63u) << 24) | ((m8 >> 6) << 30);
    };
    // lane state, all in 32-bit registers (no per-lane booleans carried around the loop: the compiler keeps those as lane masks and spends
    // a dozen scalar instructions per round re-deriving them): p >= seglen = the chain has left the segment (or the lane has none);
    // room = slots free in front of the word being read, minus the two a step may need (< 0: general step); direct = 1 once the ids go to HBM
    const uint32_t seglen = t.have ? t.seglen : 0u;
    uint32_t p = t.entry >> 1, fd = t.entry & 1u, E = 0, direct = 0, hop = 0;
    // gate >= 0 <=> the lane may take the straight-line step: (p, 0) state, staging, and the two slots a step may need are free in front
    // of the word being read (gate = free slots - 2 - (fd | direct) << 16); GATE_DEAD: the chain has left the segment (or the lane has none).
    // ONE register says which of the three a lane is.
    constexpr int GATE_DEAD = -(1 << 24);
    const int slack0 = (int)SLACK - 2 - (int)stage_after;
    int gate = p < seglen ? slack0 + (int)p - (int)(fd << 16) : GATE_DEAD;
    const uint32_t nounk = no_id == ID_NONE ? 1u : 0u;
    // the straight-line step of one lane
    auto fast_step = [&]() __attribute__((always_inline)) {
      uint32_t id, fdn, miss, adv;
      if (NARROW) {
        const uint32_t m8 = rowm[SLACK + p];
        id = rowa[SLACK + p];                                          // (a character without a token carries the unk id in the id plane, if there is one)
        miss = m8 >> 7; fdn = (m8 >> 6) & 1u; adv = m8 & 63u;
      } else {
        const uint32_t w = row[SLACK + p];
        if (w == R_INVALID) atomicOr(error_flag, 2u);                  // (never on a chain K1 / K3 produced: T(p,0) exists for every p < seglen; the walk ends, adv = 63)
        miss = w >> 31; fdn = (w >> 30) & 1u; adv = (w >> 24) & 63u;
        id = w & ID_NONE;
      }
      const uint32_t has = 1u - (miss & nounk);
      if (NARROW) { rowa[E] = (uint16_t)id; E += has; rowa[E] = (uint16_t)delete_id; }
      else { row[E] = id; E += has; row[E] = delete_id; }
      E += fdn;
      gate += (int)adv - (int)(fdn * 0x10001u + has);                    // one slot per id, and out of the straight-line steps while fd' is set
      nfd += fdn;
      nmiss += miss;
      fd = fdn;
      p += max(adv, 1u);                                               // (a (p, 0) state always advances — also on a row that is not one: the walk ends)
      gate = p < seglen ? gate : GATE_DEAD;
    };
    for (;;) {
      // The straight-line rounds are a loop of their own, entered by the lanes that can take them and left when the first of THEM cannot any
      // more (its chain has left the segment, or it needs the general step: gate < 0 either way): inside, a round is the step, one compare and
      // one branch - no lane mask to set and restore, no second question.  A wavefront leaves this loop a dozen times in its life.  (With the
      // masks inside the loop a round was 11 scalar instructions beside its 27 vector ones; what that bought, and what it did not, is in
      // profiles/r05_issue_model.txt.)
#ifndef TM_EMU
      if (gate >= 0) {
        do fast_step(); while (__builtin_amdgcn_ballot_w64(gate < 0) == 0ull);       // (a ballot of the lanes in the loop)
      }
#else
      // (tools/emu: wave-level operations are meeting points of ALL lanes of a wavefront, so the lanes that stay outside go round too)
      if (__builtin_amdgcn_ballot_w64(gate >= 0) != 0ull) {
        const bool in = gate >= 0;
        do { if (in) fast_step(); } while (__builtin_amdgcn_ballot_w64(in && gate < 0) == 0ull);
      }
#endif
      const bool general = (uint32_t)gate > (uint32_t)GATE_DEAD;      // GATE_DEAD < gate < 0 (as unsigned numbers these lie above everything else)
      if (__builtin_amdgcn_ballot_w64(general) != 0ull) {
        if (general) {
          const uint32_t w = word(p, fd);
          if (w == R_INVALID || hop > 2u * SEG) { atomicOr(error_flag, 2u); p = seglen; gate = GATE_DEAD; }      // cannot happen on a chain K1/K3 produced (a chain visits a state at most once)
          else {
            const uint32_t id = w & ID_NONE;
            const bool fits = direct == 0u && slack0 + (int)p - (int)E >= 0;
            if (!fits && direct == 0u) { direct = 1u; staged = E; }      // from here on the segment's ids go straight to HBM
            fd = (w >> 30) & 1u;
            nfd += fd;
            nmiss += w >> 31;
            if (fits) {
              if (NARROW) { if (id != ID_NONE) rowa[E++] = (uint16_t)id; if (fd) rowa[E++] = (uint16_t)delete_id; }
              else { if (id != ID_NONE) row[E++] = id; if (fd) row[E++] = delete_id; }
            } else {
              if (id != ID_NONE) { if (t.base + E < out_cap) TM_STREAM_STORE(&out[t.base + E], id); E++; }
              if (fd) { if (t.base + E < out_cap) TM_STREAM_STORE(&out[t.base + E], delete_id); E++; }
            }
            p += (w >> 24) & 63u;                                          // (0 is possible: a one-byte alternative of a forward-delete state)
            hop++;
            gate = p < seglen ? slack0 + (int)p - (int)E - (int)((fd | direct) << 16) : GATE_DEAD;
          }
        }
      } else if (__builtin_amdgcn_ballot_w64(gate >= 0) == 0ull) break;                 // no lane can step: every chain has left its segment
    }
    if (direct == 0u) staged = E;
    // what the document's Count() and `missing` need beyond the id count of K3 (rare: the document is only looked up when there is something to add)
    if (nfd | nmiss) {
      const uint32_t doc = seg_doc[g0 + lane];
      if (nfd) atomicAdd(&doc_fd[doc], nfd);
      if (nmiss) atomicAdd(&doc_missing[doc], nmiss);
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
#pragma unroll 4
  for (int s = 0; s < nv; s++) {
    const uint32_t n = (uint32_t)__shfl((int)staged, s);
    const uint64_t base = shfl_u64(t.base, s);
    for (uint32_t j = (uint32_t)lane; j < n; j += 64u) if (base + j < out_cap) TM_STREAM_STORE(&out[base + j], NARROW ? (uint32_t)s_a[NARROW ? s : 0][j] : s_tile[NARROW ? 0 : s][j]);
  }
}

// K4 for the two-plane rows, second form: POSITIONS are staged, not ids.  The walk only needs the advance / flag byte of a position, so only
// that plane of a segment's row is in LDS (272 bytes instead of 816), and what the walk leaves behind - in the bytes it has passed, as the id
// form does - is the position of every id; a second phase of the whole wavefront then fetches the ids of the listed positions from the id plane
// where it lies in HBM and writes them out.  K4's time follows the number of chains a CU walks side by side (profiles/r05_issue_model.txt (3)):
// 16 segments per wavefront and 32 wavefronts per CU = 512 instead of 192.
//   list entry (one byte): the position the id of this output slot comes from; the SAME position twice in a row: the second slot is the delete
//   token behind the token of the first.  A slot whose id comes from a forward-delete state (the side list, not the row) is written by the walk
//   itself and has its bit set in a 256-bit map of the segment: the second phase leaves it alone.  Positions of consecutive ids differ (a step that consumes no byte - a forward-delete state may - and everything
//   behind it is written straight to HBM, like ids that do not fit in front of the byte being read), and a word without an id carries no
//   forward-delete flag (tm_kernels.hip: the only producer of "missing" is T's first line), so the rule has no second reading.
// WIDE: the ids of the row are u32 (vocabularies of more than 65 536 ids), else u16
// OUT16: the ids go out as 16 bits each - `out` is the serialized form of go/tokenmonster.go:1545 itself (a chunk of the host-to-host ring with
// two-byte ids: no serializing pass behind K4, 1.6 GB less traffic per GiB of text)
template <bool WIDE, bool OUT16 = false>
__global__ __launch_bounds__(64) void k_emit_list(const uint32_t* __restrict__ R0, const uint2* __restrict__ side,
                                                  const uint32_t* __restrict__ R1, const uint4* __restrict__ par, uint64_t nseg,
                                                  uint32_t delete_id, uint64_t out_cap, uint32_t* __restrict__ out,
                                                  uint32_t* __restrict__ error_flag, uint32_t stage_after, const uint32_t* __restrict__ seg_doc,
                                                  uint32_t* __restrict__ doc_fd, uint32_t* __restrict__ doc_missing, uint32_t no_id,
                                                  const uint64_t* __restrict__ ctl = nullptr) {
  alignas(16) __shared__ uint8_t s_m[TSL][TROW_L];
  __shared__ uint32_t s_side[TSL][9];                 // (a word of slack: slot numbers up to TROW_L - 1 are looked up)
  __shared__ uint32_t s_n[TSL];
  __shared__ uint64_t s_base[TSL];
  const int lane = threadIdx.x;
  const uint64_t g0 = (uint64_t)blockIdx.x * TSL;
  if (ctl) { nseg = ctl[0]; if (g0 >= nseg) return; }
  const int nv = (int)(nseg - g0 < (uint64_t)TSL ? nseg - g0 : (uint64_t)TSL);
  const TileSeg t = tile_segment(par, g0 + lane, lane < TSL, nseg);
  constexpr uint32_t SLACK = TSLACK_L;
  const uint8_t* rows_g = reinterpret_cast<const uint8_t*>(R0);
  typedef typename std::conditional<WIDE, uint32_t, uint16_t>::type idt;
  typedef typename std::conditional<OUT16, uint16_t, uint32_t>::type outt;
  outt* const outp = reinterpret_cast<outt*>(out);
  constexpr uint64_t RS = WIDE ? R0_WIDE : R0_NARROW, FO = WIDE ? 4 * SEG : 2 * SEG;      // bytes per row, where its flag plane begins
  {
    // lane l fetches the flag bytes of positions 4l .. 4l+3 of every row; all loads before the first LDS write
    uint32_t vb[TSL];
#pragma unroll
    for (int s = 0; s < TSL; s++) {
      const int ss = s < nv ? s : nv - 1;
      const uint32_t len = s < nv ? (uint32_t)__shfl((int)t.seglen, ss) : 0u;
      vb[s] = 0u;
      if (4u * (uint32_t)lane < len) vb[s] = TM_STREAM_LOAD(reinterpret_cast<const uint32_t*>(rows_g + (g0 + (uint64_t)ss) * RS + FO) + lane);
    }
#pragma unroll
    for (int s = 0; s < TSL; s++) *reinterpret_cast<uint32_t*>(&s_m[s][TSLACK_L + 4 * lane]) = vb[s];
#pragma unroll
    for (int i = lane; i < TSL * 9; i += 64) reinterpret_cast<uint32_t*>(s_side)[i] = 0u;
    static_assert((TSL & (TSL - 1)) == 0 && TSL >= 8 && TSL <= 64, "a lane per segment, lane & (TSL - 1); the second phase takes eight at a time");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
  }
  uint32_t staged = 0;
  {
    const int rl = lane & (TSL - 1);                                     // (lanes >= TSL have no segment; they only need valid pointers)
    uint8_t* rowm = s_m[rl];
    uint32_t* smap = s_side[rl];
    const uint2* __restrict__ sl = side + (g0 + rl) * SIDE_STRIDE;
    const idt* __restrict__ ids_g = reinterpret_cast<const idt*>(rows_g + (g0 + (uint64_t)(rl < nv ? rl : 0)) * RS);
    uint32_t nfd = 0, nmiss = 0;                                       // delete tokens emitted / characters without a token (go :1274)
    // the word of state (p, fd): T(p,1) from the segment's side list, T(p,0) from the flag byte in LDS and the id where it lies (general step only)
    auto word = [&](uint32_t pp, uint32_t f) -> uint32_t {
      if (f != 0) return side_word(sl, R1, g0 + rl, pp);
      const uint32_t m8 = rowm[SLACK + pp];
      return ((m8 >> 7) ? no_id : (uint32_t)ids_g[pp]) | ((m8 & 63u) << 24) | ((m8 >> 6) << 30);
    };
    const uint32_t seglen = t.have ? t.seglen : 0u;
    uint32_t p = t.entry >> 1, fd = t.entry & 1u, E = 0, direct = 0, hop = 0;
    // gate: as in k_emit_tiles (>= 0: straight-line step; GATE_DEAD < gate < 0: general step; GATE_DEAD: the chain has left the segment)
    constexpr int GATE_DEAD = -(1 << 24);
    const int slack0 = (int)SLACK - 2 - (int)stage_after;
    int gate = p < seglen ? slack0 + (int)p - (int)(fd << 16) : GATE_DEAD;
    const uint32_t nounk = no_id == ID_NONE ? 1u : 0u;
    auto fast_step = [&]() __attribute__((always_inline)) {
      const uint32_t m8 = rowm[SLACK + p];
      const uint32_t miss = m8 >> 7, fdn = (m8 >> 6) & 1u, adv = m8 & 63u;
      const uint32_t has = 1u - (miss & nounk);
      rowm[E] = (uint8_t)p; E += has; rowm[E] = (uint8_t)p;              // the id's slot, then (same position again) the delete token's
      E += fdn;
      gate += (int)adv - (int)(fdn * 0x10001u + has);
      nfd += fdn;
      nmiss += miss;
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
          const uint32_t w = word(p, fd);
          if (w == R_INVALID || hop > 2u * SEG) { atomicOr(error_flag, 2u); p = seglen; gate = GATE_DEAD; }      // cannot happen on a chain K1/K3 produced
          else {
            const uint32_t id = w & ID_NONE, adv = (w >> 24) & 63u, fdn = (w >> 30) & 1u;
            // staged only while the list can say it: room in front of the byte being read, a byte consumed (positions of consecutive ids differ),
            // and no delete token without a token in front of it
            const bool fits = direct == 0u && slack0 + (int)p - (int)E >= 0 && adv != 0u && !(id == ID_NONE && fdn != 0u);
            if (!fits && direct == 0u) { direct = 1u; staged = E; }      // from here on the segment's ids go straight to HBM
            nfd += fdn;
            nmiss += w >> 31;
            if (fits) {
              if (id != ID_NONE) {
                // (the id of a forward-delete state is not in the row: it goes out here, and the slot is marked as written)
                if (fd) { smap[E >> 5] |= 1u << (E & 31u); if (t.base + E < out_cap) TM_STREAM_STORE(&outp[t.base + E], (outt)id); }
                rowm[E++] = (uint8_t)p;
              }
              if (fdn) rowm[E++] = (uint8_t)p;
            } else {
              if (id != ID_NONE) { if (t.base + E < out_cap) TM_STREAM_STORE(&outp[t.base + E], (outt)id); E++; }
              if (fdn) { if (t.base + E < out_cap) TM_STREAM_STORE(&outp[t.base + E], (outt)delete_id); E++; }
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
    if (nfd | nmiss) {
      const uint32_t doc = seg_doc[g0 + lane];
      if (nfd) atomicAdd(&doc_fd[doc], nfd);
      if (nmiss) atomicAdd(&doc_missing[doc], nmiss);
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  // second phase: the ids of the listed positions.  A round takes 64 slots of EVERY segment of the tile: the fetches of a round are issued back to
  // back (one trip to HBM per round, not per segment), then its stores; a segment has more than 64 slots about every other time, 512 at most.
  // Nothing branches before the stores: a lane without a slot reads the last byte of the row and fetches some id of the row.
  if (out_cap == 0) return;
  if (lane < TSL) { s_n[lane] = lane < nv ? staged : 0u; s_base[lane] = t.base; }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  uint32_t nmax = 0;
#pragma unroll
  for (int s = 0; s < TSL; s++) nmax = max(nmax, s_n[s]);
  nmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)nmax);
  for (uint32_t j0 = 0; j0 < nmax; j0 += 64u) {
    const uint32_t j = j0 + (uint32_t)lane, jj = min(j, (uint32_t)TROW_L - 1u), jp = max(jj, 1u) - 1u;
    // (eight segments at a time: sixteen fetches in flight cost the registers of half the wavefronts a CU holds)
#pragma unroll 1
    for (int s0 = 0; s0 < TSL; s0 += 8) {
      uint32_t idv[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int s = s0 + k, ss = s < nv ? s : nv - 1;
        const uint32_t pp = s_m[s][jj], prev = s_m[s][jp];
        const uint32_t fetched = reinterpret_cast<const idt*>(rows_g + (g0 + (uint64_t)ss) * RS)[pp];
        idv[k] = (pp == prev && j != 0u) ? delete_id : fetched;
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int s = s0 + k;
        const uint64_t base = s_base[s];
        const bool written = ((s_side[s][jj >> 5] >> (jj & 31u)) & 1u) != 0u;
        if (j < s_n[s] && !written && base + j < out_cap) TM_STREAM_STORE(&outp[base + j], (outt)idv[k]);
      }
    }
  }
}

// K4, scoring variant of the tile walk (training/trainvocab.go:1105-1174): persistent workgroups (the LDS-privatised histogram is
// what keeps the hot ids off the L2 atomics), every wavefront walks tiles of TS segments.
template <int WV>
__global__ __launch_bounds__(WV * 64) void k_score_tiles(const uint32_t* __restrict__ R0, const uint2* __restrict__ side,
                                                        const uint32_t* __restrict__ R1, const uint8_t* __restrict__ text,
                                                        const uint4* __restrict__ par, uint64_t nseg, uint32_t delete_id,
                                                        uint32_t* __restrict__ scores, unsigned long long* __restrict__ tokens,
                                                        uint32_t* __restrict__ missing_bits, uint32_t* __restrict__ error_flag, int narrow, uint32_t no_id) {
  alignas(16) __shared__ uint32_t s_tile[WV][TS][TROW];
  alignas(16) __shared__ unsigned long long s_w[HSLOTS];
  __shared__ unsigned long long s_ntok;
  __shared__ uint32_t s_ndel;
  for (int j = threadIdx.x; j < HSLOTS; j += WV * 64) s_w[j] = HEMPTY;
  if (threadIdx.x == 0) { s_ntok = 0; s_ndel = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t ntok = 0, ndel = 0;
  for (uint64_t g0 = ((uint64_t)blockIdx.x * WV + wv) * TS; g0 < nseg; g0 += (uint64_t)gridDim.x * WV * TS) {
    const int nv = (int)(nseg - g0 < (uint64_t)TS ? nseg - g0 : (uint64_t)TS);
    const TileSeg t = tile_segment(par, g0 + lane, lane < TS, nseg);
    tile_load(s_tile[wv], t, g0, nv, lane, R0, narrow, no_id);
    // Walk (TS lanes, a chain each): the words of the chain are only collected — word number h of a segment's chain goes to word h
    // of its own row while that lies in front of the position being read ...
    // (one loop of the wavefront, as in k_emit_tiles: a straight-line step for the (p, 0) states, the general one only when a lane is in a
    // forward-delete state or has no room: a forward-delete state may advance by 0 bytes, so a chain that alternates between the two kinds
    // of state byte after byte collects words faster than it reads them — two per byte — and TSLACK does not cover that.  A word that would
    // reach the words still to be read is counted at once instead of being staged.  (Until round 3 it was staged regardless: the chain then
    // read its own staged words as transitions — found by tools/emu/fuzz.py, seed 1100002.)
    uint32_t staged = 0;
    {
      const int rl = lane & (TS - 1);                                   // (lanes >= TS have no segment; they only need a valid pointer)
      uint32_t* row = s_tile[wv][rl];
      const uint32_t seglen = t.have ? t.seglen : 0u;
      uint32_t p = t.entry >> 1, fd = t.entry & 1u, hop = 0;
      const uint2* __restrict__ sl = side + (g0 + rl) * SIDE_STRIDE;
      for (;;) {
        const bool alive = p < seglen;
        if (!__any(alive)) break;
        const bool slow = alive && (fd != 0u || staged >= TSLACK + p);
        if (__any(slow)) {
          if (slow) {
            const uint32_t w = fd != 0u ? side_word(sl, R1, g0 + rl, p) : row[TSLACK + p];
            if (w == R_INVALID || hop > 2u * SEG) { atomicOr(error_flag, 2u); p = seglen; }      // cannot happen on a chain K1/K3 produced
            else {
              fd = (w >> 30) & 1u;
              if (w >> 31) {                                       // trainvocab.go:1166-1173: no token for this byte
                const uint32_t byte = text[t.begin + p];
                atomicOr(&missing_bits[byte >> 5], 1u << (byte & 31));
              } else if (staged < TSLACK + p) row[staged++] = w;
              else atomicAdd(&scores[w & ID_NONE], (w >> 24) & 63u);     // no room in front of the words still to be read: counted here
              ntok += 1 + fd;                                      // tokensInText++ (also for a missing byte, :1169) / += 2
              ndel += fd;                                          // scores[deleteToken]++ (:1134,1143,1152)
              p += (w >> 24) & 63u;
              hop++;
            }
          }
        }
        if (alive && !slow) {
          const uint32_t w = row[TSLACK + p];
          if (w == R_INVALID) atomicOr(error_flag, 2u);            // (never on a chain K1 / K3 produced: T(p,0) exists for every p < seglen; the walk ends, adv = 63)
          const uint32_t miss = w >> 31;
          fd = (w >> 30) & 1u;
          row[staged] = w;                                         // (staged < TSLACK + p; unconditional: a word that does not count is overwritten by the next one or lies behind the count)
          staged += 1u - miss;
          if (miss) {                                              // trainvocab.go:1166-1173: no token for this byte
            const uint32_t byte = text[t.begin + p];
            atomicOr(&missing_bits[byte >> 5], 1u << (byte & 31));
          }
          ntok += 1 + fd;
          ndel += fd;
          p += max((w >> 24) & 63u, 1u);                           // (a (p, 0) state always advances — also on a row that is not one: the walk ends)
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
    // ... and counted by all 64 lanes: scores[id] += bytes covered (:1109..1162), through the workgroup's LDS histogram
    for (int sg = 0; sg < nv; sg++) {
      const uint32_t n = (uint32_t)__shfl((int)staged, sg);
      for (uint32_t j = (uint32_t)lane; j < n; j += 64u) {
        const uint32_t w = s_tile[wv][sg][j];
        const uint32_t id = w & ID_NONE, adv = (w >> 24) & 63u;
        hist_add(s_w, scores, id, adv);
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
  }
  for (int o = 32; o > 0; o >>= 1) { ntok += __shfl_xor(ntok, o); ndel += __shfl_xor(ndel, o); }
  if (lane == 0) {
    if (ndel) atomicAdd(&s_ndel, ndel);
    if (ntok) atomicAdd(&s_ntok, (unsigned long long)ntok);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < HSLOTS; j += WV * 64)
    if ((uint32_t)s_w[j] != 0) atomicAdd(&scores[(uint32_t)(s_w[j] >> 32)], (uint32_t)s_w[j]);
  if (threadIdx.x == 0) {
    if (s_ndel) atomicAdd(&scores[delete_id], s_ndel);
    if (s_ntok) atomicAdd(tokens, s_ntok);
  }
}

// K4 of the scoring pass for the two-plane rows (round 6): k_emit_list's position staging instead of k_score_tiles' word staging - only the flag
// plane of a row is in LDS (272 bytes per segment instead of 1 056), so a workgroup walks 16 wavefronts x 16 chains beside its histogram instead
// of 11 x 8, and K4's time follows the number of chains a CU walks side by side (profiles/r05_issue_model.txt (3)).
//   The list has one entry per STEP of the chain: the position the step began at.  The bytes a token covers (trainvocab.go:1109-1162:
//   scores[id] += length) are the distance to the next entry (to where the chain left the segment, or stopped being staged, for the last one).
//   A step without a token to fetch from the id plane - a character without a token (:1166-1173), or a forward-delete state, whose token
//   comes from the side list and is counted by the walk itself - is entered TWICE: equal neighbours say "skip".  Steps that consume no byte
//   (a forward-delete state may) cannot be listed: from the first of them, as from the first step that finds no room in front of the byte being
//   read, the chain's tokens are counted by the walk itself.
template <int WV>
__global__ __launch_bounds__(WV * 64) void k_score_list(const uint32_t* __restrict__ R0, const uint2* __restrict__ side,
                                                       const uint32_t* __restrict__ R1, const uint8_t* __restrict__ text,
                                                       const uint4* __restrict__ par, uint64_t nseg, uint32_t delete_id,
                                                       uint32_t* __restrict__ scores, unsigned long long* __restrict__ tokens,
                                                       uint32_t* __restrict__ missing_bits, uint32_t* __restrict__ error_flag, uint32_t stage_after) {
  alignas(16) __shared__ uint8_t s_m[WV][TSL][TROW_L];
  alignas(16) __shared__ uint32_t s_w[4 * H16_SETS];
  __shared__ uint32_t s_n[WV][TSL], s_pend[WV][TSL];
  __shared__ unsigned long long s_ntok;
  __shared__ uint32_t s_ndel;
  for (int j = threadIdx.x; j < 4 * H16_SETS; j += WV * 64) s_w[j] = 0u;
  if (threadIdx.x == 0) { s_ntok = 0; s_ndel = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint8_t* rows_g = reinterpret_cast<const uint8_t*>(R0);
  constexpr uint32_t SLACK = TSLACK_L;
  uint32_t ntok = 0, ndel = 0;
  for (uint64_t g0 = ((uint64_t)blockIdx.x * WV + wv) * TSL; g0 < nseg; g0 += (uint64_t)gridDim.x * WV * TSL) {
    const int nv = (int)(nseg - g0 < (uint64_t)TSL ? nseg - g0 : (uint64_t)TSL);
    const TileSeg t = tile_segment(par, g0 + lane, lane < TSL, nseg);
    {
      uint32_t vb[TSL];
#pragma unroll
      for (int s = 0; s < TSL; s++) {
        const int ss = s < nv ? s : nv - 1;
        const uint32_t len = s < nv ? (uint32_t)__shfl((int)t.seglen, ss) : 0u;
        vb[s] = 0u;
        if (4u * (uint32_t)lane < len) vb[s] = TM_STREAM_LOAD(reinterpret_cast<const uint32_t*>(rows_g + (g0 + (uint64_t)ss) * R0_NARROW + 2 * SEG) + lane);
      }
#pragma unroll
      for (int s = 0; s < TSL; s++) *reinterpret_cast<uint32_t*>(&s_m[wv][s][TSLACK_L + 4 * lane]) = vb[s];
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0);
    }
    uint32_t staged = 0, pend = 0;
    {
      const int rl = lane & (TSL - 1);
      uint8_t* rowm = s_m[wv][rl];
      const uint2* __restrict__ sl = side + (g0 + rl) * SIDE_STRIDE;
      const uint16_t* __restrict__ ids_g = reinterpret_cast<const uint16_t*>(rows_g + (g0 + (uint64_t)(rl < nv ? rl : 0)) * R0_NARROW);
      const uint32_t seglen = t.have ? t.seglen : 0u;
      uint32_t p = t.entry >> 1, fd = t.entry & 1u, E = 0, direct = 0, hop = 0;
      constexpr int GATE_DEAD = -(1 << 24);
      const int slack0 = (int)SLACK - 2 - (int)stage_after;
      int gate = p < seglen ? slack0 + (int)p - (int)(fd << 16) : GATE_DEAD;      // as in k_emit_list: >= 0 straight-line step, GATE_DEAD < gate < 0 general step
      auto note_missing = [&](uint32_t pp) {                               // trainvocab.go:1166-1173: no token for this byte
        const uint32_t byte = text[t.begin + pp];
        atomicOr(&missing_bits[byte >> 5], 1u << (byte & 31));
      };
      auto fast_step = [&]() __attribute__((always_inline)) {
        const uint32_t m8 = rowm[SLACK + p];
        const uint32_t miss = m8 >> 7, fdn = (m8 >> 6) & 1u, adv = m8 & 63u;
        rowm[E] = (uint8_t)p; rowm[E + 1u] = (uint8_t)p;                   // the step's entry; a second one for a character without a token
        E += 1u + miss;
        if (miss) note_missing(p);
        gate += (int)adv - (int)(fdn << 16) - (int)(1u + miss);
        ntok += 1u + fdn;                                                  // tokensInText++ (also for a missing byte, :1169) / += 2
        ndel += fdn;                                                       // scores[deleteToken]++ (:1134,1143,1152)
        fd = fdn;
        p += max(adv, 1u);
        gate = p < seglen ? gate : GATE_DEAD;
      };
      for (;;) {
#ifndef TM_EMU
        if (gate >= 0) {
          do fast_step(); while (__builtin_amdgcn_ballot_w64(gate < 0) == 0ull);
        }
#else
        if (__builtin_amdgcn_ballot_w64(gate >= 0) != 0ull) {
          const bool in = gate >= 0;
          do { if (in) fast_step(); } while (__builtin_amdgcn_ballot_w64(in && gate < 0) == 0ull);
        }
#endif
        const bool general = (uint32_t)gate > (uint32_t)GATE_DEAD;
        if (__builtin_amdgcn_ballot_w64(general) != 0ull) {
          if (general) {
            uint32_t w;
            if (fd != 0u) w = side_word(sl, R1, g0 + rl, p);
            else { const uint32_t m8 = rowm[SLACK + p]; w = (uint32_t)ids_g[p] | ((m8 & 63u) << 24) | ((m8 >> 6) << 30); }      // (only read while its flag byte is intact: E <= p + SLACK - 2 or direct)
            if (w == R_INVALID || hop > 2u * SEG) { atomicOr(error_flag, 2u); if (direct == 0u) { direct = 1u; staged = E; pend = p; } p = seglen; gate = GATE_DEAD; }
            else {
              const uint32_t id = w & ID_NONE, adv = (w >> 24) & 63u, fdn = (w >> 30) & 1u, miss = w >> 31;
              const bool fits = direct == 0u && slack0 + (int)p - (int)E >= 0 && adv != 0u;
              if (!fits && direct == 0u) { direct = 1u; staged = E; pend = p; }      // from here on the chain's tokens are counted here
              ntok += 1u + fdn;
              ndel += fdn;
              if (miss) note_missing(p);
              else if (!fits || fd != 0u) hist16_add(s_w, scores, id, adv);       // a forward-delete state's token is not in the row
              if (fits) {
                rowm[E++] = (uint8_t)p;
                if (fd != 0u || miss) rowm[E++] = (uint8_t)p;                  // "skip": counted above, or nothing to count
              }
              fd = fdn;
              p += adv;
              hop++;
              gate = p < seglen ? slack0 + (int)p - (int)E - (int)((fd | direct) << 16) : GATE_DEAD;
            }
          }
        } else if (__builtin_amdgcn_ballot_w64(gate >= 0) == 0ull) break;
      }
      if (direct == 0u) { staged = E; pend = p; }
    }
    if (lane < TSL) { s_n[wv][lane] = lane < nv ? staged : 0u; s_pend[wv][lane] = pend; }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
    // second phase, all 64 lanes: the ids of the listed positions from the id plane, scores[id] += bytes covered through the workgroup's histogram
    uint32_t nmax = 0;
#pragma unroll
    for (int s = 0; s < TSL; s++) nmax = max(nmax, s_n[wv][s]);
    nmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)nmax);
    for (uint32_t j0 = 0; j0 < nmax; j0 += 64u) {
      const uint32_t j = j0 + (uint32_t)lane, jj = min(j, (uint32_t)TROW_L - 2u), jp = max(jj, 1u) - 1u;
#pragma unroll 1
      for (int s0 = 0; s0 < TSL; s0 += 8) {
        uint32_t idv[8], advv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int s = s0 + k, ss = s < nv ? s : nv - 1;
          const uint32_t n = s_n[wv][s];
          const uint32_t pp = s_m[wv][s][jj], prev = s_m[wv][s][jp], nxt = j + 1u < n ? (uint32_t)s_m[wv][s][jj + 1u] : s_pend[wv][s];
          const bool skip = j >= n || (pp == prev && j != 0u) || (j + 1u < n && pp == nxt);
          idv[k] = reinterpret_cast<const uint16_t*>(rows_g + (g0 + (uint64_t)ss) * R0_NARROW)[pp];
          advv[k] = skip ? 0u : nxt - pp;
        }
#pragma unroll
#ifndef TM_SCORE_NOHIST      // (tools/variant_ab.sh: what the walk alone costs - results are WRONG)
        for (int k = 0; k < 8; k++) if (advv[k] != 0u) hist16_add(s_w, scores, idv[k], advv[k]);
#else
        for (int k = 0; k < 8; k++) if (advv[k] == 77u && idv[k] == 0x1234u) atomicAdd(&scores[0], 1u);
#endif
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
  }
  for (int o = 32; o > 0; o >>= 1) { ntok += __shfl_xor(ntok, o); ndel += __shfl_xor(ndel, o); }
  if (lane == 0) {
    if (ndel) atomicAdd(&s_ndel, ndel);
    if (ntok) atomicAdd(&s_ntok, (unsigned long long)ntok);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 4 * H16_SETS; j += WV * 64)
    if ((s_w[j] & H16_CNT) != 0u) atomicAdd(&scores[((s_w[j] >> 28) << 12) | (uint32_t)(j >> 2)], s_w[j] & H16_CNT);
  if (threadIdx.x == 0) {
    if (s_ndel) atomicAdd(&scores[delete_id], s_ndel);
    if (s_ntok) atomicAdd(tokens, s_ntok);
  }
}

__global__ void k_hist_finish(const unsigned long long* __restrict__ tokens, const uint32_t* __restrict__ missing_bits,
                              uint32_t* __restrict__ tail) {
  uint32_t t = threadIdx.x;
  if (t < 4) tail[t] = (uint32_t)((*tokens >> (16 * t)) & 0xFFFFull);
  if (t < 256) tail[4 + t] = (missing_bits[t >> 5] >> (t & 31)) & 1u;
}

// pack u32 ids to 2/3/4 little-endian bytes (go/tokenmonster.go:1545, :1817, :2089)
__global__ void k_serialize(const uint32_t* __restrict__ ids, uint64_t n, uint32_t enc, uint8_t* __restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t v = ids[i];
  uint8_t* o = out + i * enc;
  o[0] = (uint8_t)v;
  o[1] = (uint8_t)(v >> 8);
  if (enc >= 3) o[2] = (uint8_t)(v >> 16);
  if (enc == 4) o[3] = 0;                     // go :2089 writes a zero high byte
}

// The same, eight ids per work-item and 16-byte stores, for the two widths a stream is normally written in (2 bytes: up to 65 536 ids; 4:
// the server's wide form): `out` may be page-locked HOST memory (tm_tokenize_pipeline writes the ids of a chunk straight into the caller's
// pinned buffer: no device staging, no copy command behind the kernel), where only full-width stores of neighbouring lanes make sensible
// PCIe writes.  ids [0, head) and the last few are left to k_serialize (the vector part starts at the first 16-byte boundary of `out`).
template <int ENC>
__global__ __launch_bounds__(256) void k_serialize_wide(const uint32_t* __restrict__ ids, uint64_t head, uint64_t nvec, uint8_t* __restrict__ out) {
  constexpr int PER = 16 / ENC;                       // ids per 16 bytes of output
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nvec) return;
  const uint32_t* src = ids + head + t * PER;
  uint32_t v[PER];
#pragma unroll
  for (int k = 0; k < PER; k++) v[k] = src[k];
  uint4 o;
  if (ENC == 2) o = make_uint4((v[0] & 0xFFFFu) | (v[1] << 16), (v[2] & 0xFFFFu) | (v[3] << 16), (v[4] & 0xFFFFu) | (v[5] << 16), (v[6] & 0xFFFFu) | (v[7] << 16));
  else o = make_uint4(v[0] & 0xFFFFFFu, v[1] & 0xFFFFFFu, v[2] & 0xFFFFFFu, v[3 % PER] & 0xFFFFFFu);
  *reinterpret_cast<uint4*>(out + (head + t * PER) * ENC) = o;
}

// ---- a chunk of the host-to-host ring: the counts stay on the device --------------------------------------------------------------------
// k_chunk_ctl, behind the normalizer pass: ninfo = what tm_batch_normalize reads back ([0] documents for the host normalizer, [1] long
// documents, [2] segments, [3] undecided pieces, [4] pieces that outgrew their slab, [5] normalized bytes, [6] short pieces inside a document).
// A chunk with any of those (or beyond the bounds its kernels were launched over) is NOT taken: ctl[0] = ctl[1] = 0 turn the kernels behind
// this one into no-ops, the status word tells the host, which runs the chunk through the exact path (tm_host.hip).
__global__ void k_chunk_ctl(const unsigned long long* __restrict__ ninfo, uint32_t ndocs, uint64_t max_bytes, uint64_t seg_bound, uint64_t* __restrict__ ctl) {
  if (threadIdx.x != 0) return;
  uint64_t st = 0;
  if (ninfo[0]) st |= RING_HOST_DOCS;
  if (ninfo[1]) st |= RING_LONG_DOCS;
  if (ninfo[3]) st |= RING_UNDECIDED;
  if (ninfo[4]) st |= RING_SLAB;
  if (ninfo[6]) st |= RING_SHORT_PIECE;
  if (ninfo[5] > max_bytes) st |= RING_BYTES;
  if (ninfo[2] > seg_bound) st |= RING_SEGS;
  ctl[0] = st ? 0ull : ninfo[2];
  ctl[1] = st ? 0ull : (uint64_t)ndocs;
  ctl[2] = 0ull;
  ctl[3] = st;
  ctl[4] = ninfo[5];
  ctl[5] = ninfo[0];
}
// the verdict of a chunk whose ids K4 has packed itself (no k_serialize_ctl behind it)
__global__ void k_chunk_done(const uint64_t* __restrict__ ctl, const uint64_t* __restrict__ totals, const uint32_t* __restrict__ error_flag, uint64_t out_cap,
                             uint64_t* __restrict__ h_status) {
  if (threadIdx.x != 0) return;
  uint64_t st = ctl[3];
  const uint64_t ntok = st ? 0ull : totals[1];
  const uint32_t err = *error_flag;
  if (!st && err) st |= RING_ERROR;
  if (!st && ntok > out_cap) st |= RING_OUT_CAP;
  h_status[1] = ntok; h_status[2] = ctl[4]; h_status[3] = ctl[0]; h_status[4] = err; h_status[5] = ctl[5];
  __threadfence_system();                      // (the host polls the status word: what it says must be there first)
  h_status[0] = st;
}
// the verdict of a piece of tm_tokenize_document (k_doc_chain has written the piece's control words): as k_chunk_done, and the piece's characters
// without a token beside the count of its ids
__global__ void k_doc_done(const uint64_t* __restrict__ ctl, const uint64_t* __restrict__ totals, const uint32_t* __restrict__ error_flag, const uint32_t* __restrict__ doc_missing,
                           uint64_t out_cap, uint64_t* __restrict__ h_status) {
  if (threadIdx.x != 0) return;
  uint64_t st = ctl[3];
  const uint64_t ntok = st ? 0ull : totals[1];
  const uint32_t err = *error_flag;
  if (!st && err) st |= RING_ERROR;
  if (!st && ntok > out_cap) st |= RING_OUT_CAP;
  h_status[1] = ntok; h_status[2] = st ? 0ull : (uint64_t)doc_missing[0]; h_status[3] = ctl[0]; h_status[4] = err;
  __threadfence_system();                      // (the host watches the status word: what it says must be there first)
  h_status[0] = st;
}
// ids -> enc bytes each, the count worked out on the device (the status word of k_chunk_ctl the id total, the error word); sixteen ids per work-item, 16-byte stores (`out` 16-byte aligned)
// ... and k_chunk_done's part with it (one launch less behind K4): every work-item works the count out for itself, the first one tells the host
template <int ENC>
__global__ __launch_bounds__(256) void k_serialize_ctl(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ ctl, uint8_t* __restrict__ out,
                                                       const uint64_t* __restrict__ totals, const uint32_t* __restrict__ error_flag, uint64_t out_cap, uint64_t* __restrict__ h_status) {
  uint64_t st = ctl[3];
  const uint64_t ntok = st ? 0ull : totals[1];
  const uint32_t err = *error_flag;
  if (!st && err) st |= RING_ERROR;
  if (!st && ntok > out_cap) st |= RING_OUT_CAP;
  const uint64_t n = st ? 0ull : ntok;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    h_status[1] = ntok; h_status[2] = ctl[4]; h_status[3] = ctl[0]; h_status[4] = err; h_status[5] = ctl[5];
    __threadfence_system();
    h_status[0] = st;
  }
  const uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16u;
  if (i0 >= n) return;
  if (i0 + 16u <= n) {
    uint32_t v[16];
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint4 q = reinterpret_cast<const uint4*>(ids + i0)[k]; v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w; }
    uint4* o = reinterpret_cast<uint4*>(out + i0 * ENC);
    if (ENC == 2) {
#pragma unroll
      for (int k = 0; k < 2; k++)
        o[k] = make_uint4((v[8 * k] & 0xFFFFu) | (v[8 * k + 1] << 16), (v[8 * k + 2] & 0xFFFFu) | (v[8 * k + 3] << 16), (v[8 * k + 4] & 0xFFFFu) | (v[8 * k + 5] << 16),
                          (v[8 * k + 6] & 0xFFFFu) | (v[8 * k + 7] << 16));
    } else if (ENC == 4) {
#pragma unroll
      for (int k = 0; k < 4; k++) o[k] = make_uint4(v[4 * k] & 0xFFFFFFu, v[4 * k + 1] & 0xFFFFFFu, v[4 * k + 2] & 0xFFFFFFu, v[4 * k + 3] & 0xFFFFFFu);
    } else {
      // 3 bytes each: four ids make three words
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t a = v[4 * k] & 0xFFFFFFu, b = v[4 * k + 1] & 0xFFFFFFu, c = v[4 * k + 2] & 0xFFFFFFu, d = v[4 * k + 3] & 0xFFFFFFu;
        reinterpret_cast<uint32_t*>(o)[3 * k] = a | (b << 24);
        reinterpret_cast<uint32_t*>(o)[3 * k + 1] = (b >> 8) | (c << 16);
        reinterpret_cast<uint32_t*>(o)[3 * k + 2] = (c >> 16) | (d << 8);
      }
    }
  } else {
    for (uint64_t i = i0; i < n; i++) {
      const uint32_t v = ids[i];
      uint8_t* o = out + i * ENC;
      o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8);
      if (ENC >= 3) o[2] = (uint8_t)(v >> 16);
      if (ENC == 4) o[3] = 0;
    }
  }
}

}  // namespace tmh

using namespace tmh;

// ------------------------------------------------------------------------------------------------
// tm_batch
// ------------------------------------------------------------------------------------------------

namespace tmh {

// Test hooks (tm_debug_flags): bits that force a rarely taken fallback path of the product so that the tests can cover it, with the
// same results: 5 = the wide exit map for every segment (K1 step C), 6 = dense T(p,1) array for every segment, 8 = per-lane normalizer kernel, 10 = K4 tile walk that stores every id
// directly, 11 = the device normalizer packs its text instead of leaving it in the slabs for K1, 12 = group tree of long documents with fan-out 4
// from 9 segments on (a deep tree on a small document), 13 = a 64 KiB
// mailbox for the small host <-> device transfers (wraps within a test), 14 = the last member of tm_score_multi gives up after the first
// meeting of the members (an ERROR path: every member must return), 15 = K4's id-staging walk for two-plane rows too, 16 = nothing any more (it split k_seg_fill into
// two launches for a chunk of the host-to-host ring while the batch path had them apart; every caller has the one launch now), 24 = one chunk of a
// tm_tokenize_pipeline call fails at a place of the host code named in TM_TEST_FAIL (an ERROR path, tm_host.hip: PipeCall::hook_arm; the bits 17 - 23
// between belong to the -DTM_DEVEL build, and the match kernel reads 17 and 18 in every build).  Nothing else is
// reachable in the default build.  With -DTM_DEVEL (tools/ only: results are WRONG) further bits switch
// phases of K1 off for profiling — 0 no walks at all, 2 no hash probes, 3 no forward-delete probes, 4 no exit maps — bit 9 adds 4 KB
// of dummy LDS per K1 workgroup, and TM_DBG in the environment sets the initial value.
#ifndef TM_DEVEL
constexpr int kDebugMask = 32 | 64 | 256 | 1024 | 2048 | 4096 | 8192 | 16384 | 32768 | 65536 | 16777216;
#define TM_K1_EXTRA_LDS 0
#define TM_DBG_INITIAL 0
#endif
int g_debug_flags = -1;
// The hooks are armed only in a process that was started with TM_TEST_HOOKS in its environment (the test suite's conftest, bench.py
// --also-flags): in any other process tm_debug_flags() is inert, so that no caller of a server can change the code path under the others.
bool hooks_armed() { static const bool armed = getenv("TM_TEST_HOOKS") != nullptr; return armed; }
int debug_flags() {
  if (g_debug_flags < 0) g_debug_flags = TM_DBG_INITIAL;
  return g_debug_flags;
}

// T(p,0) rows in the narrow form (u16 id + u8 advance / flags per position) whenever the ids fit
static bool r0_narrow(const tm_batch* b) { return b->vocab->host.n_ids <= 65536u; }
// ... k_match_branch's `narrow`: two planes (1: u16 ids, 2: u32 ids) for K4's position-staging walk; one plane of u32 words for the id-staging
// walks - the scoring pass of a vocabulary of more than 65 536 ids, and test hook 15 on such a vocabulary
static int r0_mode(const tm_batch* b, bool for_score) { return r0_narrow(b) ? 1 : (for_score || (debug_flags() & 32768)) ? 0 : 2; }
static uint32_t r0_no_id(const tm_batch* b) { return b->vocab->tables.unk_id != TM_NONE ? b->vocab->tables.unk_id : ID_NONE; }      // what a character without a token emits (go :1269-1276)

uint32_t long_segs() { return (debug_flags() & 4096) ? 8u : LONG_SEGS; }

static const char* kKernelNames[TM_NUM_KERNELS] = {"segments", "match_branch", "resolve", "scan", "emit"};

static hipError_t batch_alloc_bytes(tm_batch* b, void** p, uint64_t bytes) {
  hipError_t e = hipMalloc(p, bytes ? bytes : 16);
  if (e == hipSuccess) b->device_bytes += bytes;
  return e;
}
template <typename T>
static hipError_t dalloc(tm_batch* b, T** p, uint64_t count) { return batch_alloc_bytes(b, (void**)p, count * sizeof(T)); }

void launch_doc_units(const uint64_t* doc_begin, const uint64_t* doc_end, uint32_t ndocs, uint32_t unit, uint32_t* doc_nunits, hipStream_t st) {
  if (ndocs) TM_LAUNCH(k_doc_nseg, (ndocs + 255) / 256, 256, 0, st, doc_begin, doc_end, ndocs, doc_nunits, unit);
}
void launch_unit_owner(const uint64_t* doc_unit_start, uint32_t ndocs, uint64_t nunits, uint32_t* unit_doc, hipStream_t st, const uint64_t* count_dev) {
  if (nunits) TM_LAUNCH(k_segments, (uint32_t)((nunits + 255) / 256), 256, 0, st, doc_unit_start, ndocs, nunits, unit_doc, count_dev);
}
static void launch_seg_params(tm_batch* b, hipStream_t st);
void launch_chain_hist(tm_batch* b, uint32_t delete_id, int n_cu, uint32_t* d_hist, unsigned long long* d_tokens, uint32_t* d_missing_bits,
                       uint32_t n_ids, hipStream_t st) {
  const uint64_t nseg = b->nseg;
  pack_text(b, st);                    // (k_score_tiles looks at the text)
  if (nseg > 0) {
    launch_seg_params(b, st);
    constexpr int WV = SEG <= 256 ? 11 : 5;      // wavefronts of a scoring workgroup: as many tiles as fit the LDS beside the histogram
    constexpr int WVL = 16;                      // ... of the position-staging form: 16 x 16 chains, 68 KB of flag bytes beside the 64 KB histogram
    if (r0_narrow(b) && !(debug_flags() & 32768))      // (test hook 15: the word-staging walk for the two-plane rows too)
      TM_LAUNCH(k_score_list<WVL>, (uint32_t)std::min<uint64_t>((nseg + WVL * TSL - 1) / (WVL * TSL), (uint64_t)n_cu), WVL * 64, 0, st,
          b->d_R0, b->d_side, b->d_R1, b->d_text, b->d_seg_par, nseg, delete_id, d_hist, d_tokens, d_missing_bits, b->d_error, (debug_flags() & 1024) ? 512u : 0u);
    else
    TM_LAUNCH(k_score_tiles<WV>, (uint32_t)std::min<uint64_t>((nseg + WV * TS - 1) / (WV * TS), (uint64_t)n_cu), WV * 64, 0, st, 
        b->d_R0, b->d_side, b->d_R1, b->d_text, b->d_seg_par, nseg, delete_id, d_hist, d_tokens, d_missing_bits, b->d_error, r0_narrow(b) ? 1 : 0, r0_no_id(b));
  }
  TM_LAUNCH(k_hist_finish, 1, 256, 0, st, d_tokens, d_missing_bits, d_hist + n_ids);
}

// the per-segment records of k_seg_params (after the token-offset scan)
static void launch_seg_params(tm_batch* b, hipStream_t st) {
  TM_LAUNCH(k_seg_params, (uint32_t)((b->nseg + 1 + 255) / 256), 256, 0, st, b->d_doc_begin, b->d_doc_end, b->d_seg_doc, b->d_doc_seg_start, b->nseg, b->ndocs, b->d_seg_entry,
                                                                      b->d_seg_tokbase, b->d_tok_offsets, b->d_seg_par, b->d_ctl);
}
// K4 for the id-emitting entry points: the tile walk (test hook bit 10: every id stored directly, the overflow path of the staging)
// store == false (Count): the same walk with an output capacity of 0 — it is there for the delete tokens and missing characters it counts
// rezero: the per-document counters have been added to since k_resolve cleared them (the emit stage is being repeated)
static void launch_emit(tm_batch* b, hipStream_t st, bool store, bool rezero = false) {
  const uint64_t nseg = b->nseg;
  const uint32_t nd = b->ndocs;
  if (rezero) {
    (void)hipMemsetAsync(b->d_doc_fd, 0, (size_t)nd * 4, st);
    (void)hipMemsetAsync(b->d_doc_missing, 0, (size_t)nd * 4, st);
  }
  if (nseg > 0) {
    launch_seg_params(b, st);
    const uint32_t stage_after = (debug_flags() & 1024) ? 512u : 0u;
    if (!(debug_flags() & 32768) && !r0_narrow(b))             // (test hook 15: the id-staging form of the walk instead - for the larger vocabularies over one-plane rows)
      TM_LAUNCH(k_emit_list<true>, (uint32_t)((nseg + TSL - 1) / TSL), 64, 0, st, b->d_R0, b->d_side, b->d_R1, b->d_seg_par, nseg, b->vocab->tables.delete_id, store ? b->out_cap : 0, b->d_out,
                                                                   b->d_error, stage_after, b->d_seg_doc, b->d_doc_fd, b->d_doc_missing, r0_no_id(b), b->d_ctl);
    else if (!(debug_flags() & 32768) && store && b->d_out16)      // (a chunk of the ring with two-byte ids: K4 writes the serialized form itself)
      TM_LAUNCH((k_emit_list<false, true>), (uint32_t)((nseg + TSL - 1) / TSL), 64, 0, st, b->d_R0, b->d_side, b->d_R1, b->d_seg_par, nseg, b->vocab->tables.delete_id, b->out16_cap,
                                                                           reinterpret_cast<uint32_t*>(b->d_out16), b->d_error, stage_after, b->d_seg_doc, b->d_doc_fd, b->d_doc_missing, r0_no_id(b), b->d_ctl);
    else if (!(debug_flags() & 32768))
      TM_LAUNCH(k_emit_list<false>, (uint32_t)((nseg + TSL - 1) / TSL), 64, 0, st, b->d_R0, b->d_side, b->d_R1, b->d_seg_par, nseg, b->vocab->tables.delete_id, store ? b->out_cap : 0, b->d_out,
                                                                   b->d_error, stage_after, b->d_seg_doc, b->d_doc_fd, b->d_doc_missing, r0_no_id(b), b->d_ctl);
    else if (r0_narrow(b))
      TM_LAUNCH(k_emit_tiles<true>, (uint32_t)((nseg + TS - 1) / TS), 64, 0, st, b->d_R0, b->d_side, b->d_R1, b->d_seg_par, nseg, b->vocab->tables.delete_id, store ? b->out_cap : 0, b->d_out,
                                                                         b->d_error, stage_after, b->d_seg_doc, b->d_doc_fd, b->d_doc_missing, r0_no_id(b), b->d_ctl);
    else
      TM_LAUNCH(k_emit_tiles<false>, (uint32_t)((nseg + TS - 1) / TS), 64, 0, st, b->d_R0, b->d_side, b->d_R1, b->d_seg_par, nseg, b->vocab->tables.delete_id, store ? b->out_cap : 0, b->d_out,
                                                                          b->d_error, stage_after, b->d_seg_doc, b->d_doc_fd, b->d_doc_missing, r0_no_id(b), b->d_ctl);
  }
  if (nd && !store) TM_LAUNCH(k_doc_events, (nd + 255) / 256, 256, 0, st, b->d_doc_ntok, b->d_doc_fd, nd, b->d_doc_events);      // (Count() is the only reader)
}

// the same scan for up to SCAN1_MAX elements in ONE launch of one workgroup (a run of elements per thread): a server batch or a chunk of the
// host-to-host pipeline or a server batch scans a few thousand documents / pieces / segments several times, and there the two launches
// saved per scan are worth more than the parallelism lost
constexpr uint64_t SCAN1_MAX = 1u << 14;     // (a single workgroup over 2^17 elements took longer than the two launches it saved)
template <int SCAN1_T>
__global__ __launch_bounds__(SCAN1_T) void k_scan_single(const uint32_t* __restrict__ in, uint32_t n, uint64_t* __restrict__ total, uint64_t* __restrict__ out) {
  __shared__ uint64_t s[SCAN1_T];
  const uint32_t per = (n + SCAN1_T) / SCAN1_T;                       // (covers index n, the total slot)
  const uint32_t b = threadIdx.x * per, e = b + per < n ? b + per : (b < n ? n : b);
  uint64_t acc = 0;
  for (uint32_t i = b; i < e; i++) acc += in[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 1; st < SCAN1_T; st <<= 1) {
    const uint64_t t = (int)threadIdx.x >= st ? s[threadIdx.x - st] : 0;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  uint64_t run = s[threadIdx.x] - acc;
  for (uint32_t i = b; i < e; i++) { out[i] = run; run += in[i]; }
  if (b <= n && n < b + per) out[n] = run;                              // one-past-the-end = grand total
  if (threadIdx.x == SCAN1_T - 1) *total = s[SCAN1_T - 1];
}

void scan_u32(const uint32_t* in, uint64_t n, uint64_t* block_sums, uint64_t* total, uint64_t* out, hipStream_t st) {
  static const int scan1 = [] { const char* e = getenv("TM_SCAN1"); return e ? atoi(e) : 1024; }();
  if (n <= SCAN1_MAX && scan1 == 1024) { TM_LAUNCH(k_scan_single<1024>, 1, 1024, 0, st, in, (uint32_t)n, total, out); return; }
  if (n <= SCAN1_MAX && scan1 == 256) { TM_LAUNCH(k_scan_single<256>, 1, 256, 0, st, in, (uint32_t)n, total, out); return; }
  uint32_t nblocks = (uint32_t)((n + 1 + SCAN_CH - 1) / SCAN_CH);   // covers index n (the total slot)
  TM_LAUNCH(k_scan_partial, nblocks, SCAN_T, 0, st, in, n, block_sums);
  TM_LAUNCH(k_scan_sums, 1, SCAN_T, 0, st, block_sums, nblocks, total);
  TM_LAUNCH(k_scan_final, nblocks, SCAN_T, 0, st, in, n, block_sums, out);
}

// room for the group tree of the long documents: ngroups groups, nlong documents, and their pinned staging.  make_workspace reserves what a
// batch of the workspace's size can need at most (a few MB): long documents are rare, and when each lane of the host-to-host pipeline met
// its first one in a different call, each of those calls stopped the whole device for ~8 ms (hipFree / hipMalloc / hipHostMalloc).
int reserve_groups(tm_batch* b, uint32_t ngroups, uint32_t nlong) {
  hipError_t e;
  if (ngroups > b->cap_groups) {
    if (b->cap_groups) trace_grow("segment groups", (uint64_t)ngroups * (sizeof(Group) + ENT * sizeof(uint2) + 5));
    (void)hipFree(b->d_groups); (void)hipFree(b->d_gmap); (void)hipFree(b->d_group_entry); (void)hipFree(b->d_group_base);
    b->d_groups = nullptr; b->d_gmap = nullptr; b->d_group_entry = nullptr; b->d_group_base = nullptr;
    b->cap_groups = ngroups + ngroups / 4 + 16;
    if ((e = hipMalloc((void**)&b->d_groups, (size_t)b->cap_groups * sizeof(Group))) != hipSuccess ||
        (e = hipMalloc((void**)&b->d_gmap, (size_t)b->cap_groups * ENT * sizeof(uint2))) != hipSuccess ||
        (e = hipMalloc((void**)&b->d_group_entry, b->cap_groups)) != hipSuccess ||
        (e = hipMalloc((void**)&b->d_group_base, (size_t)b->cap_groups * sizeof(uint32_t))) != hipSuccess)
      return hip_fail(e, "hipMalloc (segment groups)");
  }
  if (nlong > b->cap_long) {
    if (b->cap_long) trace_grow("long documents", (uint64_t)nlong * sizeof(LongDoc));
    (void)hipFree(b->d_longs);
    b->d_longs = nullptr;
    b->cap_long = nlong + nlong / 4 + 16;
    if ((e = hipMalloc((void**)&b->d_longs, (size_t)b->cap_long * sizeof(LongDoc))) != hipSuccess) return hip_fail(e, "hipMalloc (long documents)");
  }
  const size_t need = (((size_t)ngroups * sizeof(Group) + 255) & ~(size_t)255) + (size_t)nlong * sizeof(LongDoc);
  if (b->h_groups_cap < need) {
    if (b->h_groups_cap) trace_grow("segment groups (pinned staging)", need);
    (void)hipHostFree(b->h_groups);
    b->h_groups = nullptr;
    b->h_groups_cap = need + need / 4 + 4096;
    if ((e = hipHostMalloc((void**)&b->h_groups, b->h_groups_cap, hipHostMallocDefault)) != hipSuccess) { b->h_groups_cap = 0; return hip_fail(e, "hipHostMalloc (segment groups)"); }
  }
  return TM_OK;
}

// host: the group tree of the long documents.  doc d has lens[d] bytes; segments are numbered in document order.  groups[] holds
// level 1 first (children = segments), then level 2 (children = level-1 groups), ...; b->level_first[k] is where level k+1 begins.
int build_groups(tm_batch* b, const uint64_t* begin, const uint64_t* end, uint32_t ndocs, hipStream_t st) {
  std::vector<std::vector<Group>> levels;        // levels[k]: groups of level k+1, all long documents, in document order
  std::vector<LongDoc> longs;
  struct Top { uint32_t level, first, count; };  // a long document's top groups: index range within its top level
  std::vector<Top> tops;
  uint64_t seg = 0;
  const uint64_t FAN = (debug_flags() & 4096) ? 4u : GROUP_FAN;      // (test hook bit 12: a deep tree on a small document)
  const uint64_t LONG = long_segs();
  for (uint32_t d = 0; d < ndocs; d++) {
    const uint64_t S = (end[d] - begin[d] + SEG - 1) / SEG;
    if (S > LONG) {
      uint64_t first = seg, count = S;             // children of the level being built: segments, then groups of the level below
      for (uint32_t lvl = 0;; lvl++) {
        if (levels.size() <= lvl) levels.emplace_back();
        const uint32_t g0 = (uint32_t)levels[lvl].size();
        for (uint64_t k = 0; k < count; k += FAN)
          levels[lvl].push_back(Group{(uint32_t)(first + k), (uint32_t)std::min<uint64_t>(FAN, count - k), d, lvl});
        const uint32_t ng = (uint32_t)levels[lvl].size() - g0;
        if (ng <= FAN) { tops.push_back(Top{lvl, g0, ng}); longs.push_back(LongDoc{d, 0u, ng, 0u}); break; }
        first = g0; count = ng;                    // (indices within the level: rebased below once the level offsets are known)
      }
    }
    seg += S;
  }
  if (seg >= (1ull << 32)) return set_error(TM_E_LIMIT, "batch has more than 2^32 segments");
  std::vector<Group> groups;
  b->level_first.assign(1, 0u);
  for (auto& lv : levels) { groups.insert(groups.end(), lv.begin(), lv.end()); b->level_first.push_back((uint32_t)groups.size()); }
  for (size_t lvl = 1; lvl < levels.size(); lvl++)                       // children of a level >= 2 group are groups of the level below
    for (uint32_t g = b->level_first[lvl]; g < b->level_first[lvl + 1]; g++) groups[g].first_child += b->level_first[lvl - 1];
  for (size_t i = 0; i < longs.size(); i++) longs[i].first_group = b->level_first[tops[i].level] + tops[i].first;
  b->ngroups = (uint32_t)groups.size();
  b->nlong = (uint32_t)longs.size();
  if (b->ngroups == 0) return TM_OK;
  hipError_t e;
  { int rc = reserve_groups(b, b->ngroups, b->nlong); if (rc != TM_OK) return rc; }
  // (not hipMemcpy from the vectors: a pageable copy pins its pages per call and runs on the NULL stream — with other threads
  // loading vocabularies at the same time that cost 10 - 20 ms per scoring pass.  Through the batch's pinned staging instead.)
  const size_t gb = groups.size() * sizeof(Group), lb = longs.size() * sizeof(LongDoc), lat = (gb + 255) & ~(size_t)255;
  std::memcpy(b->h_groups, groups.data(), gb);
  std::memcpy(b->h_groups + lat, longs.data(), lb);
  if ((e = hipMemcpyAsync(b->d_groups, b->h_groups, gb, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(b->d_longs, b->h_groups + lat, lb, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)             // (the staging buffer is reused by the next batch)
    return hip_fail(e, "H2D segment groups");
  return TM_OK;
}

// The pipeline in two halves, so that the scoring pass can look at the exit maps (tm_score_begin) before the entry states of its byte
// ranges are known (tm_score_finish): pipeline_match = K0 + K1 (+ the group maps of long documents), pipeline_resolve = K3 + scan (+ K4).
int pipeline_match(tm_batch* b, hipStream_t st, hipEvent_t* ev, bool for_score) {
  const tm_vocab* v = b->vocab;
  { int rc = enter_device(v); if (rc != TM_OK) return rc; }
  b->last_stream = st;
  (void)hipGetLastError();               // (the check at the end is for the launches in between, not for what some earlier call of this thread has left behind)
  auto mark = [&](int k) { if (ev) (void)hipEventRecord(ev[k], st); };
  const uint32_t nd = b->ndocs;
  const uint64_t nseg = b->nseg;
  if (nd == 0) (void)hipMemsetAsync(b->d_error, 0, 4, st);
  mark(0);
  if (nd > 0) {
    TM_LAUNCH(k_doc_nseg, (nd + 255) / 256, 256, 0, st, b->d_doc_begin, b->d_doc_end, nd, b->d_doc_nseg, (uint32_t)SEG, b->d_error);
    scan_u32(b->d_doc_nseg, nd, b->d_scan_tmp, b->d_totals + 0, b->d_doc_seg_start, st);
    // the segments' documents and the records K1 starts from (in d_seg_par, which K4's parameters take over after K3), in one launch
    if (nseg > 0)
      TM_LAUNCH(k_seg_fill, (uint32_t)((nseg + 255) / 256), 256, 0, st, b->d_doc_seg_start, nd, b->d_doc_begin, b->d_doc_end, b->d_doc_vis ? b->d_doc_vis : b->d_doc_end,
                b->text_in_slabs ? b->d_doc_piece_start : nullptr, b->d_piece_off, nseg, b->d_seg_doc, b->d_seg_par, b->d_ctl);
  }
  mark(1);
  if (nseg > 0)
    TM_LAUNCH(k_match_branch, (uint32_t)((nseg + WAVES - 1) / WAVES), WAVES * 64, TM_K1_EXTRA_LDS, st, v->tables, b->d_text, nseg, b->d_R0, b->d_side, b->d_R1, b->d_exitmap,
              b->d_exit16, r0_mode(b, for_score), debug_flags(), b->text_in_slabs ? b->d_slab : nullptr, b->d_seg_par, b->d_ctl);
    note_table_use(v, st);
  mark(2);
  for (size_t lvl = 0; lvl + 1 < b->level_first.size() && b->ngroups > 0; lvl++) {     // bottom up: a level reads the maps of the one below
    const uint32_t g0 = b->level_first[lvl], ng = b->level_first[lvl + 1] - g0;
    if (lvl == 0) TM_LAUNCH(k_group_compose<true>, ng, 128, 0, st, b->d_exitmap, b->d_exit16, b->d_gmap, b->d_groups, g0, b->d_gmap);
    else TM_LAUNCH(k_group_compose<false>, ng, 128, 0, st, b->d_exitmap, b->d_exit16, b->d_gmap, b->d_groups, g0, b->d_gmap);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? TM_OK : hip_fail(e, "kernel launch");
}

// mode: 0 = resolve only (the scoring pass walks the chains itself), 1 = + K4 counting only (Count), 2 = + K4 writing the ids
int pipeline_resolve(tm_batch* b, hipStream_t st, hipEvent_t* ev, int mode) {
  (void)hipGetLastError();               // (as in pipeline_match)
  const uint32_t nd = b->ndocs;
  auto mark = [&](int k) { if (ev) (void)hipEventRecord(ev[k], st); };
  if (nd > 0)
    TM_LAUNCH(k_resolve, (nd + 255) / 256, 256, 0, st, b->d_exitmap, b->d_exit16, b->d_doc_seg_start, nd, b->d_doc_entry, b->d_seg_entry, b->d_seg_tokbase,
                                                b->d_doc_ntok, b->d_error, long_segs(), b->d_doc_fd, b->d_doc_missing, b->d_ctl);
  if (b->ngroups > 0) {
    TM_LAUNCH(k_long_top, (b->nlong + 63) / 64, 64, 0, st, b->d_gmap, b->d_longs, b->nlong, b->d_doc_entry, b->d_group_entry, b->d_group_base, b->d_doc_ntok, b->d_error);
    for (size_t lvl = b->level_first.size() - 1; lvl-- > 0;) {                           // top down
      const uint32_t g0 = b->level_first[lvl], ng = b->level_first[lvl + 1] - g0;
      if (lvl == 0) TM_LAUNCH(k_group_expand<true>, (ng + 63) / 64, 64, 0, st, b->d_exitmap, b->d_exit16, b->d_gmap, b->d_groups, g0, ng, b->d_group_entry, b->d_group_base,
                                                                         b->d_seg_entry, b->d_seg_tokbase, b->d_error);
      else TM_LAUNCH(k_group_expand<false>, (ng + 63) / 64, 64, 0, st, b->d_exitmap, b->d_exit16, b->d_gmap, b->d_groups, g0, ng, b->d_group_entry, b->d_group_base,
                                                                 b->d_seg_entry, b->d_seg_tokbase, b->d_error);
    }
  }
  mark(3);
  if (nd > 0) scan_u32(b->d_doc_ntok, nd, b->d_scan_tmp, b->d_totals + 1, b->d_tok_offsets, st);
  else (void)hipMemsetAsync(b->d_tok_offsets, 0, 8, st);
  mark(4);
  if (mode > 0) launch_emit(b, st, mode == 2);
  mark(5);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? TM_OK : hip_fail(e, "kernel launch");
}

// exit state of every document for every entry state -> exits[ndocs * ENT] (device); needs pipeline_match
void launch_doc_exits(tm_batch* b, uint8_t* d_exits, hipStream_t st) {
  if (b->ndocs) TM_LAUNCH(k_doc_exits, b->ndocs, 128, 0, st, b->d_exitmap, b->d_exit16, b->d_doc_seg_start, b->d_gmap, b->d_longs, b->nlong, d_exits, long_segs());
}

// behind a pass of the streaming encoder (k_enc_carry): d_exits null = the pass was the document's last
void launch_enc_carry(tm_batch* b, const uint8_t* d_exits, uint8_t* d_entry, uint32_t* d_acc, uint64_t own, uint32_t keep, hipStream_t st) {
  TM_LAUNCH(k_enc_carry, 1, 256, 0, st, d_exits, d_entry, b->d_doc_missing, d_acc, b->d_text, own, keep);
}

int run_pipeline(tm_batch* b, hipStream_t st, bool timed, float* ms, bool emit) {
  hipError_t e;
  if (timed && !b->have_events) {
    for (auto& ev : b->ev) if ((e = hipEventCreate(&ev)) != hipSuccess) return hip_fail(e, "hipEventCreate");
    b->have_events = true;
  }
  b->has_output = false;
  b->row_form = -1;
  int rc = pipeline_match(b, st, timed ? b->ev : nullptr);
  if (rc == TM_OK) rc = pipeline_resolve(b, st, timed ? b->ev : nullptr, emit ? 2 : 1);
  if (rc != TM_OK) return rc;
  b->has_output = emit;
  if (emit) b->row_form = r0_mode(b, false);      // (what pipeline_match has just handed to K1: the span pass reads the rows in this form)
  if (timed) {
    if ((e = hipEventSynchronize(b->ev[TM_NUM_KERNELS])) != hipSuccess) return hip_fail(e, "hipEventSynchronize");
    for (int k = 0; k < TM_NUM_KERNELS; k++) (void)hipEventElapsedTime(&ms[k], b->ev[k], b->ev[k + 1]);
  }
  return TM_OK;
}

// after a run: make sure the output buffer was large enough; if not, grow it and redo the emit stage
// ---- small transfers through the pinned mailbox -----------------------------------------------------------------
__global__ void k_copy_small(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t n, int words) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (words) { if (i < n / 8) reinterpret_cast<uint64_t*>(dst)[i] = reinterpret_cast<const uint64_t*>(src)[i]; }
  else if (i < n) dst[i] = src[i];
}
static void launch_copy_small(const void* src, void* dst, uint64_t n, hipStream_t st) {
  const int words = (((uintptr_t)src | (uintptr_t)dst | n) & 7u) == 0;
  const uint64_t items = words ? n / 8 : n;
  TM_LAUNCH(k_copy_small, (uint32_t)((items + 255) / 256), 256, 0, st, (const uint8_t*)src, (uint8_t*)dst, n, words);
}
// (test hook bit 13: a 64 KiB mailbox with transfers of at most 16 KiB, so that a small test wraps it and takes the copy-engine path too)
static uint64_t mail_bytes() { return (debug_flags() & 8192) ? (64u << 10) : MAIL_BYTES; }
static uint64_t mail_max() { return (debug_flags() & 8192) ? (16u << 10) : MAIL_MAX; }
static int mail_slot(tm_batch* b, uint64_t bytes, hipStream_t st, uint8_t** slot) {
  hipError_t e;
  if (!b->h_mail && (e = hipHostMalloc((void**)&b->h_mail, MAIL_BYTES, hipHostMallocDefault)) != hipSuccess) { b->h_mail = nullptr; return hip_fail(e, "hipHostMalloc (mailbox)"); }
  const uint64_t need = (bytes + 63) & ~63ull;
  if (b->mail_pos + need > mail_bytes()) {            // wrap: every copy kernel that reads or writes a slot handed out so far must be done
    const std::vector<hipStream_t> live = b->mail_streams;           // (small_sync takes the stream off the list)
    for (hipStream_t s2 : live) { int rc = small_sync(b, s2); if (rc != TM_OK) return rc; }
    if (!b->mail_pending.empty()) return set_error(TM_E_INVALID, "mailbox wrapped with transfers pending");
    b->mail_streams.clear();
    b->mail_pos = 0;
  }
  if (std::find(b->mail_streams.begin(), b->mail_streams.end(), st) == b->mail_streams.end()) b->mail_streams.push_back(st);
  *slot = b->h_mail + b->mail_pos;
  b->mail_pos += need;
  return TM_OK;
}
int small_d2h(tm_batch* b, void* host_dst, const void* dev_src, uint64_t bytes, hipStream_t st) {
  if (bytes == 0) return TM_OK;
  if (bytes > mail_max()) {
    hipError_t e = hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? TM_OK : hip_fail(e, "D2H");
  }
  uint8_t* slot = nullptr;
  int rc = mail_slot(b, bytes, st, &slot);
  if (rc != TM_OK) return rc;
  launch_copy_small(dev_src, slot, bytes, st);
  b->mail_pending.push_back({host_dst, slot, bytes, st});
  return TM_OK;
}
int small_h2d(tm_batch* b, void* dev_dst, const void* host_src, uint64_t bytes, hipStream_t st) {
  if (bytes == 0) return TM_OK;
  if (bytes > mail_max()) {
    hipError_t e = hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, st);   // (pageable sources are staged before this returns)
    return e == hipSuccess ? TM_OK : hip_fail(e, "H2D");
  }
  uint8_t* slot = nullptr;
  int rc = mail_slot(b, bytes, st, &slot);
  if (rc != TM_OK) return rc;
  std::memcpy(slot, host_src, bytes);
  launch_copy_small(slot, dev_dst, bytes, st);
  return TM_OK;
}
int small_sync(tm_batch* b, hipStream_t st) {
  const hipError_t e = hipStreamSynchronize(st);
  // The stream's transfers leave the list either way.  Behind a failed wait nothing is copied: the destinations are the caller's buffers or its
  // stack locals, and an entry left here would have the lane's NEXT small_sync write through them.
  size_t keep = 0;
  for (auto& m : b->mail_pending) {
    if (m.st != st) b->mail_pending[keep++] = m;
    else if (e == hipSuccess) std::memcpy(m.dst, m.slot, m.n);
  }
  b->mail_pending.resize(keep);
  // every copy kernel of this stream is done (or lost): the stream no longer has to be waited for when the mailbox wraps (and a caller's
  // stream that is destroyed later is not kept here)
  b->mail_streams.erase(std::remove(b->mail_streams.begin(), b->mail_streams.end(), st), b->mail_streams.end());
  return e == hipSuccess ? TM_OK : hip_fail(e, "hipStreamSynchronize");
}

// ---- grow-only buffers (tm_pipeline.h) ------------------------------------------------------------------------------------------------------
bool is_pinned(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeHost;
}
int grow_device(uint8_t** buf, uint64_t* cap, uint64_t need, uint64_t alloc, const char* what) {
  if (*cap >= need) return TM_OK;
  if (*cap) trace_grow(what, need);
  (void)hipFree(*buf);
  *buf = nullptr; *cap = 0;
  const hipError_t e = hipMalloc((void**)buf, alloc);
  if (e != hipSuccess) { *buf = nullptr; return hip_fail(e, what); }
  *cap = alloc;
  return TM_OK;
}
int batch_replace(tm_batch* b, void** p, uint64_t old_bytes, uint64_t need_bytes, uint64_t alloc_bytes, const char* what) {
  if (*p) trace_grow(what, need_bytes);
  (void)hipFree(*p);                                   // (waits for the device: no kernel is still reading or writing the old buffer)
  b->device_bytes -= old_bytes;
  *p = nullptr;
  const hipError_t e = batch_alloc_bytes(b, p, alloc_bytes);
  if (e != hipSuccess) { *p = nullptr; return hip_fail(e, what); }
  return TM_OK;
}
int grow_batch(tm_batch* b, void** p, uint64_t* cap, uint64_t need, uint64_t alloc, uint32_t elem_bytes, const char* what) {
  if (*cap >= need) return TM_OK;
  const uint64_t old_bytes = *cap * elem_bytes;
  *cap = 0;
  const int rc = batch_replace(b, p, old_bytes, need * elem_bytes, alloc * elem_bytes, what);
  if (rc == TM_OK) *cap = alloc;
  return rc;
}
int grow_pinned(uint8_t** buf, uint64_t* cap, uint64_t need, uint64_t alloc, const char* what) {
  if (*cap >= need) return TM_OK;
  if (*cap) trace_grow(what, need);
  (void)hipHostFree(*buf);
  *buf = nullptr; *cap = 0;
  const hipError_t e = hipHostMalloc((void**)buf, alloc, hipHostMallocDefault);
  if (e != hipSuccess) { *buf = nullptr; return hip_fail(e, what); }
  *cap = alloc;
  return TM_OK;
}
int grow_workspace(tm_batch** ws, const tm_vocab* v, uint64_t bytes, uint32_t docs, uint64_t alloc_bytes, const char* what) {
  tm_batch* const w = *ws;
  if (w && w->vocab == v && w->max_bytes >= bytes && w->max_docs >= docs) return TM_OK;
  const uint64_t want_b = std::max<uint64_t>(alloc_bytes, w ? w->max_bytes : 0);
  const uint64_t want_d = std::max<uint64_t>((uint64_t)docs + docs / 4 + 64, w ? w->max_docs : 0);
  if (w) trace_grow(what, want_b);
  tm_batch_free(w);
  *ws = nullptr;
  return tm_batch_create(v, want_b, (uint32_t)std::min<uint64_t>(want_d, 0xFFFFFFF0ull), ws);
}

int error_from_flag(uint32_t err) {
  if (err == 0) return TM_OK;
  if (err & 4u) return set_error(TM_E_INPUT, "a byte range of the whole-buffer walk cannot be entered in the state the walk reaches it in (tm_score_multi)");
  if ((err & 1u) == 0u) return set_error(TM_E_INTERNAL, "the emit stage met a transition the match stage never wrote (device error word %u): a fault of this library, not of the input", err);
  return set_error(TM_E_INPUT, "the walk does not advance on this text (a vocabulary / text combination the reference does not terminate on: e.g. one-byte keys beside the delete token in a UTF-16 vocabulary)");
}

int ensure_output(tm_batch* b) {
  { int rc = enter_device(b->vocab); if (rc != TM_OK) return rc; }
  hipError_t e;
  uint64_t* totals = b->last_totals;
  uint32_t err = 0;
  { uint64_t both[5] = {0, 0, 0, 0, 0};
    int rc = small_d2h(b, both, b->d_totals, sizeof both, b->last_stream);
    if (rc == TM_OK) rc = small_sync(b, b->last_stream);
    if (rc != TM_OK) return rc;
    totals[0] = both[0]; totals[1] = both[1]; totals[2] = both[2];
    err = (uint32_t)both[4]; }
  if (err != 0) return error_from_flag(err);
  uint64_t total = b->ndocs ? totals[1] : 0;
  if (total > b->out_cap) {
    const int rc = grow_batch(b, (void**)&b->d_out, &b->out_cap, total, total + total / 4 + 1024, 4, "ids");
    if (rc != TM_OK) return rc;
    hipStream_t st = b->last_stream;
    launch_emit(b, st, true, true);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "emit rerun");
  }
  return TM_OK;
}

}  // namespace tmh

extern "C" {

const char* tm_kernel_name(int k) { return k >= 0 && k < TM_NUM_KERNELS ? kKernelNames[k] : ""; }

int tm_debug_flags(int flags) {
  const int old = tmh::debug_flags();
  if (flags >= 0 && tmh::hooks_armed()) tmh::g_debug_flags = flags & tmh::kDebugMask;
  return old;
}

}  // extern "C"
namespace tmh {
int make_workspace(const tm_vocab* v, uint64_t max_bytes, uint32_t max_docs, bool own_text, bool with_output, tm_batch** out) {
  *out = nullptr;
  { int rc = enter_device(v); if (rc != TM_OK) return rc; }
  auto* b = new tm_batch();
  b->vocab = v;
  b->max_bytes = max_bytes;
  b->max_docs = max_docs;
  b->max_segs = max_bytes / SEG + max_docs + 1;
  b->out_cap = with_output ? max_bytes / 2 + 2ull * max_docs + 1024 : 0;   // grows on demand (worst case is 2 ids per byte)
  b->text_borrowed = !own_text;
  const uint64_t nd1 = (uint64_t)max_docs + 1;
  const uint64_t scan_blocks = (nd1 + max_bytes / 256 + 2 * SCAN_CH) / SCAN_CH + 64;   // scans run over documents, segments-per-doc and 1 KiB pieces
  hipError_t e = hipSuccess;
  if ((own_text && (e = dalloc(b, &b->d_text, max_bytes + 256)) != hipSuccess) || (e = dalloc(b, &b->d_offsets, 2 * nd1)) != hipSuccess ||
      (e = dalloc(b, &b->d_doc_nseg, nd1)) != hipSuccess || (e = dalloc(b, &b->d_doc_seg_start, nd1 + 1)) != hipSuccess ||
      (e = dalloc(b, &b->d_seg_doc, b->max_segs)) != hipSuccess || (e = dalloc(b, &b->d_R0, b->max_segs * (v->host.n_ids <= 65536u ? SEG : SEG + SEG / 4))) != hipSuccess || (e = dalloc(b, &b->d_R1, b->max_segs * SEG)) != hipSuccess ||
      (e = dalloc(b, &b->d_side, b->max_segs * SIDE_STRIDE)) != hipSuccess ||
      (e = dalloc(b, &b->d_exitmap, b->max_segs * ENT)) != hipSuccess || (e = dalloc(b, &b->d_exit16, b->max_segs * ENT)) != hipSuccess || (e = dalloc(b, &b->d_seg_entry, b->max_segs)) != hipSuccess ||
      (e = dalloc(b, &b->d_seg_tokbase, b->max_segs)) != hipSuccess || (e = dalloc(b, &b->d_seg_par, b->max_segs + 1)) != hipSuccess || (e = dalloc(b, &b->d_doc_ntok, nd1)) != hipSuccess ||
      (e = dalloc(b, &b->d_doc_events, nd1)) != hipSuccess || (e = dalloc(b, &b->d_doc_missing, nd1)) != hipSuccess || (e = dalloc(b, &b->d_doc_fd, nd1)) != hipSuccess ||
      (e = dalloc(b, &b->d_tok_offsets, nd1 + 1)) != hipSuccess || (e = dalloc(b, &b->d_scan_tmp, scan_blocks)) != hipSuccess ||
      (e = dalloc(b, &b->d_totals, 8)) != hipSuccess ||
      (e = dalloc(b, &b->d_out, b->out_cap)) != hipSuccess) {
    tm_batch_free(b);
    return hip_fail(e, "hipMalloc (batch workspace)");
  }
  {
    // the group tree of long documents at its largest for this workspace: a level of segments / GROUP_FAN groups, the levels above it, and
    // a partial group per level and long document
    const uint64_t nlong_max = b->max_segs / LONG_SEGS + 1, ngroups_max = b->max_segs / GROUP_FAN + b->max_segs / (GROUP_FAN * GROUP_FAN) + 3 * nlong_max + 64;
    int rc = reserve_groups(b, (uint32_t)std::min<uint64_t>(ngroups_max, 1u << 30), (uint32_t)std::min<uint64_t>(nlong_max, 1u << 30));
    if (rc != TM_OK) { tm_batch_free(b); return rc; }
  }
  (void)hipMemset(b->d_totals, 0, 64);
  b->d_error = reinterpret_cast<uint32_t*>(b->d_totals + 4);        // (the error word lies behind the totals: ensure_output fetches both with one copy)
  *out = b;
  return TM_OK;
}
// the normalizer's share of a workspace, for the raw pieces of the streaming encoder: the text buffer the normalizer packs into, the scans'
// block sums, the totals / error words.  One document; everything else stays null (tm_batch_free and the normalizer do not mind).
int make_piece_workspace(const tm_vocab* v, uint64_t max_bytes, hipStream_t st, tm_batch** out) {
  *out = nullptr;
  { int rc = enter_device(v); if (rc != TM_OK) return rc; }
  auto* b = new tm_batch();
  b->vocab = v;
  b->max_bytes = max_bytes;
  b->max_docs = 1;
  b->max_segs = max_bytes / SEG + 2;
  const uint64_t scan_blocks = (2 + max_bytes / 256 + 2 * SCAN_CH) / SCAN_CH + 64;
  hipError_t e = hipSuccess;
  if ((e = dalloc(b, &b->d_text, max_bytes + 256)) != hipSuccess || (e = dalloc(b, &b->d_scan_tmp, scan_blocks)) != hipSuccess || (e = dalloc(b, &b->d_totals, 8)) != hipSuccess ||
      (e = hipMemsetAsync(b->d_totals, 0, 64, st)) != hipSuccess) {
    tm_batch_free(b);
    return hip_fail(e, "hipMalloc (piece workspace)");
  }
  b->d_error = reinterpret_cast<uint32_t*>(b->d_totals + 4);
  *out = b;
  return TM_OK;
}
}  // namespace tmh
extern "C" {

int tm_batch_create(const tm_vocab* v, uint64_t max_bytes, uint32_t max_docs, tm_batch** out) {
  if (!v || !out) return set_error(TM_E_INVALID, "null argument");
  return make_workspace(v, max_bytes, max_docs, true, true, out);
}

void tm_batch_free(tm_batch* b) {
  if (!b) return;
  void* ptrs[] = {b->text_borrowed ? nullptr : (void*)b->d_text, b->d_offsets, b->d_doc_nseg, b->d_doc_seg_start, b->d_seg_doc, b->d_R0, b->d_R1, b->d_side, b->d_exitmap, b->d_exit16, b->d_seg_entry,
                  b->d_seg_tokbase, b->d_seg_par, b->d_doc_ntok, b->d_doc_events, b->d_doc_missing, b->d_doc_fd, b->d_tok_offsets, b->d_scan_tmp, b->d_totals,
                  b->d_out, b->d_groups, b->d_longs, b->d_gmap, b->d_group_entry, b->d_group_base,
                  b->d_ctl_store, b->d_dec_a, b->d_dec_b, b->d_spans, b->d_own, b->d_own_tmp, b->d_win, b->d_win_rows, b->d_units[0], b->d_units[1]};
  for (void* p : ptrs) (void)hipFree(p);
  tmh::raw_free(b);                                    // the normalizer's and the filter pass's device buffers (tm_norm.hip)
  if (b->have_events) for (auto& ev : b->ev) (void)hipEventDestroy(ev);
  if (b->aux_stream) (void)hipStreamDestroy(b->aux_stream);
  (void)hipHostFree(b->h_fb_raw); (void)hipHostFree(b->h_fb_norm); (void)hipHostFree(b->h_mail); (void)hipHostFree(b->h_groups);
  delete b;
}

int tm_batch_upload(tm_batch* b, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs) {
  int rc = tmh::batch_upload_on(b, text, offsets, ndocs, nullptr);
  if (rc == TM_OK) { hipError_t e = hipStreamSynchronize(nullptr); if (e != hipSuccess) rc = hip_fail(e, "H2D text"); }
  return rc;
}

}  // extern "C"
namespace tmh {
// H2D of packed text + offsets on `st` (asynchronous when the source is pinned); the batch is then ready for run_pipeline on `st`
int batch_upload_on(tm_batch* b, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, hipStream_t st) {
  if (!b || (ndocs && (!offsets))) return set_error(TM_E_INVALID, "null argument");
  { int rc = enter_device(b->vocab); if (rc != TM_OK) return rc; }
  if (ndocs > b->max_docs) return set_error(TM_E_LIMIT, "batch has %u documents, workspace sized for %u", ndocs, b->max_docs);
  uint64_t nbytes = ndocs ? offsets[ndocs] : 0;
  if (ndocs && offsets[0] != 0) return set_error(TM_E_INVALID, "offsets[0] must be 0");
  if (nbytes > b->max_bytes) return set_error(TM_E_LIMIT, "batch has %llu bytes, workspace sized for %llu", (unsigned long long)nbytes, (unsigned long long)b->max_bytes);
  uint64_t nseg = 0;
  for (uint32_t d = 0; d < ndocs; d++) {
    if (offsets[d + 1] < offsets[d]) return set_error(TM_E_INVALID, "offsets not monotone at document %u", d);
    nseg += (offsets[d + 1] - offsets[d] + SEG - 1) / SEG;
  }
  hipError_t e;
  // (a server-sized batch goes through the pinned mailbox: a pageable copy pins the caller's pages per call, and concurrent callers queue on that)
  if (nbytes && nbytes <= mail_max()) { int rc = small_h2d(b, b->d_text, text, nbytes, st); if (rc != TM_OK) return rc; }
  else if (nbytes && (e = hipMemcpyAsync(b->d_text, text, nbytes, hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e, "H2D text");
  if (ndocs) { int rc = small_h2d(b, b->d_offsets, offsets, ((uint64_t)ndocs + 1) * 8, st); if (rc != TM_OK) return rc; }
  b->ndocs = ndocs;
  b->has_output = false;
  units_forget(b, 3u);
  b->nbytes = nbytes;
  b->nseg = nseg;
  b->d_doc_begin = b->d_offsets;
  b->text_in_slabs = false;
  b->d_doc_end = b->d_offsets + 1;
  return build_groups(b, offsets, offsets + 1, ndocs, st);
}
void launch_serialize(const uint32_t* ids, uint64_t n, uint32_t enc, uint8_t* out, hipStream_t st) {
  if (!n) return;
  if ((enc == 2 || enc == 4) && n >= 4096) {
    // ids before the first 16-byte boundary of `out` and behind the last whole 16 bytes: the byte-wise kernel; everything between: 16-byte stores
    const uint64_t per = 16 / enc, mis = (uint64_t)(reinterpret_cast<uintptr_t>(out) & 15u);
    const uint64_t head = mis ? (16 - mis) / enc : 0;          // (`out` is a multiple of enc bytes into a 16-byte aligned buffer in every caller; an odd address falls through below)
    if (mis % enc == 0) {
      const uint64_t nvec = (n - head) / per, tail0 = head + nvec * per;
      if (head) TM_LAUNCH(k_serialize, 1, 256, 0, st, ids, head, enc, out);
      if (enc == 2) TM_LAUNCH(k_serialize_wide<2>, (uint32_t)((nvec + 255) / 256), 256, 0, st, ids, head, nvec, out);
      else TM_LAUNCH(k_serialize_wide<4>, (uint32_t)((nvec + 255) / 256), 256, 0, st, ids, head, nvec, out);
      if (tail0 < n) TM_LAUNCH(k_serialize, 1, 256, 0, st, ids + tail0, n - tail0, enc, out + tail0 * enc);
      return;
    }
  }
  TM_LAUNCH(k_serialize, (uint32_t)((n + 255) / 256), 256, 0, st, ids, n, enc, out);
}

// ---- the host-to-host ring (tm_host.hip): a chunk's kernels without a host round trip ----------------------------------------------------
void launch_chunk_ctl(tm_batch* b, uint64_t seg_bound, hipStream_t st) {
  TM_LAUNCH(k_chunk_ctl, 1, 64, 0, st, (const unsigned long long*)b->d_ninfo, b->ndocs, b->max_bytes, seg_bound, b->d_ctl_store);
}
int ring_enqueue_tokenize(tm_batch* b, hipStream_t st, uint32_t enc, uint8_t* d_bytes, uint64_t d_bytes_cap, uint64_t* h_status, const uint8_t** ids_at) {
  if (!b->d_ctl) return set_error(TM_E_INTERNAL, "ring_enqueue_tokenize: the workspace has no control words");
  // (the ids that fit d_bytes: what K4 may store is bounded by out_cap, and the chunk is not taken when it needed more)
  const uint64_t cap_ids = std::min<uint64_t>(b->out_cap, d_bytes_cap / enc);
  // Where the packed ids of the chunk end up.  Two bytes each from a vocabulary of at most 65 536 ids: K4 writes them that way itself
  // (k_emit_list<false, true>).  Four bytes each: K4's uint32 ids ARE the packed form (an id has 24 bits, go :2089 writes a zero high byte).
  // Otherwise (three bytes; two bytes cut from wider ids; the id-staging walk of test hook 15) a pass behind K4 packs them.
  const bool direct16 = enc == 2 && r0_narrow(b) && !(debug_flags() & 32768);
  const bool direct32 = enc == 4;
  b->d_out16 = direct16 ? reinterpret_cast<uint16_t*>(d_bytes) : nullptr;
  b->out16_cap = cap_ids;
  int rc = pipeline_match(b, st, nullptr);
  if (rc == TM_OK) rc = pipeline_resolve(b, st, nullptr, 2);
  b->d_out16 = nullptr;
  if (rc != TM_OK) return rc;
  *ids_at = direct32 ? reinterpret_cast<const uint8_t*>(b->d_out) : d_bytes;
  if (direct16 || direct32) TM_LAUNCH(k_chunk_done, 1, 64, 0, st, b->d_ctl, b->d_totals, b->d_error, cap_ids, h_status);
  else {
    const uint32_t grid = (uint32_t)((cap_ids / 16 + 1 + 255) / 256);
    if (enc == 2) TM_LAUNCH(k_serialize_ctl<2>, grid, 256, 0, st, b->d_out, b->d_ctl, d_bytes, b->d_totals, b->d_error, cap_ids, h_status);
    else if (enc == 3) TM_LAUNCH(k_serialize_ctl<3>, grid, 256, 0, st, b->d_out, b->d_ctl, d_bytes, b->d_totals, b->d_error, cap_ids, h_status);
    else TM_LAUNCH(k_serialize_ctl<4>, grid, 256, 0, st, b->d_out, b->d_ctl, d_bytes, b->d_totals, b->d_error, cap_ids, h_status);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? TM_OK : hip_fail(e, "kernel launch");
}

// ---- tm_tokenize_document (tm_document.hip): the second half of a piece, behind pipeline_match + launch_doc_exits ---------------------------
void launch_doc_chain(tm_batch* b, uint32_t* d_cell, const uint8_t* d_exits, uint8_t* d_entry, uint64_t* d_ctl, uint64_t nseg, uint64_t from, uint32_t keep,
                      uint8_t* next_text, hipStream_t st) {
  TM_LAUNCH(k_doc_chain, 1, 64, 0, st, d_cell, d_exits, d_entry, b->d_error, d_ctl, nseg, b->d_text, from, keep, next_text);
}
// K3 .. K4 under the control words k_doc_chain has written, the ids packed to `enc` bytes, the verdict to h_status (page-locked: status bits, ids,
// characters without a token, segments, device error word).  h_scratch: eight page-locked words nobody reads (k_serialize_ctl's own verdict)
int doc_enqueue_resolve(tm_batch* b, hipStream_t st, uint32_t enc, uint64_t* d_ctl, uint8_t* d_bytes, uint64_t d_bytes_cap, uint64_t* h_status, uint64_t* h_scratch,
                        const uint8_t** ids_at) {
  const uint64_t cap_ids = enc == 4 ? b->out_cap : std::min<uint64_t>(b->out_cap, d_bytes_cap / enc);
  const bool direct16 = enc == 2 && r0_narrow(b) && !(debug_flags() & 32768);      // (as ring_enqueue_tokenize: K4 writes two-byte ids itself)
  b->d_ctl = d_ctl;
  b->d_out16 = direct16 ? reinterpret_cast<uint16_t*>(d_bytes) : nullptr;
  b->out16_cap = cap_ids;
  const int rc = pipeline_resolve(b, st, nullptr, 2);
  b->d_out16 = nullptr;
  b->d_ctl = nullptr;
  if (rc != TM_OK) return rc;
  *ids_at = enc == 4 ? reinterpret_cast<const uint8_t*>(b->d_out) : d_bytes;
  if (!direct16 && enc != 4) {
    const uint32_t grid = (uint32_t)((cap_ids / 16 + 1 + 255) / 256);
    if (enc == 2) TM_LAUNCH(k_serialize_ctl<2>, grid, 256, 0, st, b->d_out, d_ctl, d_bytes, b->d_totals, b->d_error, cap_ids, h_scratch);
    else TM_LAUNCH(k_serialize_ctl<3>, grid, 256, 0, st, b->d_out, d_ctl, d_bytes, b->d_totals, b->d_error, cap_ids, h_scratch);
  }
  TM_LAUNCH(k_doc_done, 1, 64, 0, st, d_ctl, b->d_totals, b->d_error, b->d_doc_missing, cap_ids, h_status);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? TM_OK : hip_fail(e, "kernel launch");
}
// a piece whose ids outgrew the slot's buffers (RING_OUT_CAP): the emit stage again into a larger id buffer (ensure_output), with the stream waited for
int doc_redo_emit(tm_batch* b, hipStream_t st, uint64_t* d_ctl) {
  b->d_ctl = d_ctl;
  b->last_stream = st;
  const int rc = ensure_output(b);
  b->d_ctl = nullptr;
  return rc;
}
}  // namespace tmh
extern "C" {

int tm_batch_run(tm_batch* b, void* stream) {
  if (!b) return set_error(TM_E_INVALID, "null argument");
  return run_pipeline(b, (hipStream_t)stream, false, nullptr, true);
}

int tm_batch_run_timed(tm_batch* b, void* stream, float* ms) {
  if (!b || !ms) return set_error(TM_E_INVALID, "null argument");
  return run_pipeline(b, (hipStream_t)stream, true, ms, true);
}

int tm_batch_totals(tm_batch* b, uint64_t* total_tokens, uint64_t* total_missing) {
  if (!b) return set_error(TM_E_INVALID, "null argument");
  int rc = ensure_output(b);
  if (rc != TM_OK) return rc;
  hipError_t e;
  uint64_t totals[3] = {0, 0, 0};
  if ((e = hipMemcpy(totals, b->d_totals, sizeof totals, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "hipMemcpy totals");
  if (total_tokens) *total_tokens = b->ndocs ? totals[1] : 0;
  if (total_missing) {
    std::vector<uint32_t> miss(b->ndocs);
    if (b->ndocs && (e = hipMemcpy(miss.data(), b->d_doc_missing, (size_t)b->ndocs * 4, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "hipMemcpy missing");
    uint64_t m = 0;
    for (auto x : miss) m += x;
    *total_missing = m;
  }
  return TM_OK;
}

int tm_batch_download(tm_batch* b, uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* tok_offsets, uint32_t* missing) {
  if (!b) return set_error(TM_E_INVALID, "null argument");
  int rc = ensure_output(b);
  if (rc != TM_OK) return rc;
  hipError_t e;
  std::vector<uint64_t> offs((size_t)b->ndocs + 1, 0);
  if (b->ndocs && (e = hipMemcpy(offs.data(), b->d_tok_offsets, offs.size() * 8, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "D2H tok_offsets");
  if (tok_offsets) std::memcpy(tok_offsets, offs.data(), offs.size() * 8);
  if (missing && b->ndocs && (e = hipMemcpy(missing, b->d_doc_missing, (size_t)b->ndocs * 4, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "D2H missing");
  uint64_t total = offs[b->ndocs];
  if (total > tokens_cap) return set_error(TM_E_NOSPACE, "tokens_cap %llu < %llu required", (unsigned long long)tokens_cap, (unsigned long long)total);
  if (total && (e = hipMemcpy(tokens_out, b->d_out, total * 4, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "D2H tokens");
  return TM_OK;
}

const uint32_t* tm_batch_device_tokens(const tm_batch* b) { return b->d_out; }
const uint64_t* tm_batch_device_tok_offsets(const tm_batch* b) { return b->d_tok_offsets; }
uint64_t tm_batch_device_bytes(const tm_batch* b) { return b->device_bytes; }

#ifdef TM_PHASE_TIMERS
TM_DEVEL_PHASES_ENTRY
#endif

}  // extern "C"

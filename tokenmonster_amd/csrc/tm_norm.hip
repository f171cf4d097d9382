// tm_norm.hip — GPU normalizer behind tm_batch_upload_raw / tm_batch_normalize (include/tokenmonster_hip.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "tm_pipeline.h"
#include "tm_build.h"
#include "tm_norm_masks.h"

using namespace tmh;

// ================================================================================================
// GPU normalizer: the pre-step of Tokenize (go/tokenmonster.go:242-253: norm.Normalize then capcode.Encode)
// ================================================================================================
// Handles, entirely on the device, documents made of ASCII plus the NFD-stable General Punctuation block
// (U+2010..U+2027, U+2030..U+205E: curly quotes, dashes, ellipsis ...; U+2019 counts as an apostrophe exactly as in
// javascript/tokenmonster.js:878).  For these NFD is the identity (tokenmonster.cpp:190-198) and capcode level 2
// (javascript/tokenmonster.js:900-1005) becomes a LOCAL function of each character once three facts about its
// "capital run" are known.  A run is what the encoder's inWord state covers: it starts at the first capital of a
// maximal block of {capital, digit, apostrophe} characters and extends to the end of that block.  Needed per char:
//   ub   capitals before it in its block (0 = it is the run's first letter; >= 1 = inside the run)
//   ua   capitals after it in its block       (every later capital of a run is inside a run of several capitals)
//   tL   the character right after the block is a lowercase letter ('C' mode: "Hello"; otherwise 'W' mode: "HELLO")
// Documents are cut into 1 KiB pieces, one wavefront each (text staged in LDS):
//   pass 1  k_norm_summary  per piece: leading / trailing block-run summary, unsupported-byte flag
//   pass 2  k_norm_carry    per document: carries ub / ua / tL across piece boundaries (a few bits per piece)
//   pass 3  k_norm_emit<0>  per piece: output length            -> scan -> where every piece goes
//   pass 4  k_norm_emit<1>  per piece: the normalized bytes
// Any other document (other non-ASCII bytes: needs ICU for NFD / Unicode case) is normalized by the host normalizer
// (tm_normalize.cpp) and appended after the device-normalized documents; documents are (begin, end) ranges, so the
// layout of the device part never waits for the host.
namespace tmh {

constexpr int PIECE = 1024, PMARGIN = 68, PLDS = PIECE + 2 * PMARGIN;      // 64 bytes of margin either side (k_norm_emit2<false> takes its carries from them) + 4: the classifier looks three bytes either way
// character classes NC_* and flag bits NF_*: tm_norm_masks.h
// piece summary bits
constexpr uint32_t PS_WHOLE = 1u, PS_LEADU_SHIFT = 1, PS_LEADTL = 8u, PS_TRAILU_SHIFT = 5, PS_FIRSTBLOCK = 128u, PS_FIRSTL = 256u, PS_BAD = 512u;

__device__ __forceinline__ uint32_t ncls_ascii(uint32_t c, bool lower_all) {
  if (c - 'a' < 26u) return NC_L;
  if (c - 'A' < 26u) return lower_all ? NC_L : NC_U;
  if (c - '0' < 10u) return NC_N;
  if (c == '\'') return NC_AP;
  if (c == ' ') return NC_SP;
  return NC_O;
}
__device__ __forceinline__ bool nblock(uint32_t cls) { return (cls & NF_BLOCK) != 0; }       // capital, digit, apostrophe, combining mark

// (chg[c]: chunk c of the piece has a byte of a character that the pass CHANGES - a two-byte character, which takes its bytes from the table, or one
// NFD splits; set by norm_load_piece, looked at by k_norm_emit2, which leaves emit_high_byte alone for a chunk of nothing but inert characters)
struct PieceLds { alignas(16) uint8_t raw[PLDS]; alignas(4) uint8_t f[PLDS]; uint8_t chg[32]; };
// The normalizer's tables in ONE device buffer (tm_norm_masks.h): NmTwo[NM_TWO_SIZE] | block codes [NM_BLK_WORDS] | code-point codes
// [NM_CP_WORDS] | block codes of the four-byte characters [NM_BLK4_WORDS] | one word of switches (NM_MISC_*; 16 bytes with its padding).  The 256 work-items of a workgroup stage the entries of U+0080..U+017F (2 KB) and the block codes (256 bytes) in LDS.
constexpr size_t NM_TABLE_BYTES = NM_TWO_SIZE * sizeof(NmTwo) + (NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS + 4) * sizeof(uint32_t) + NM_LEA_SIZE * sizeof(NmLea) + NM_KANA_SIZE * sizeof(uint16_t) + NM_CCC_SIZE + (NM_DEC3_SIZE + NM_DEC3_THIRDS) * sizeof(uint32_t);      // (... | the characters of Latin Extended Additional, read where they lie)
struct TabLds { NmTwo two[NM_TWO_FAST]; uint32_t blk[NM_BLK_WORDS]; uint32_t misc; };
__device__ __forceinline__ NmTabs stage_tabs(TabLds& s, const NmTwo* __restrict__ two) {
  static_assert(NM_TWO_FAST == 256 && NM_BLK_WORDS <= 256, "one entry per work-item");
  const uint32_t* blk = reinterpret_cast<const uint32_t*>(two + NM_TWO_SIZE);
  s.two[threadIdx.x] = two[threadIdx.x];
  if (threadIdx.x < NM_BLK_WORDS) s.blk[threadIdx.x] = blk[threadIdx.x];
  const uint32_t misc = (uint32_t)__builtin_amdgcn_readfirstlane((int)blk[NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS]);
  if (threadIdx.x == 0) s.misc = misc;
  return NmTabs{s.two, two, s.blk, blk + NM_BLK_WORDS, blk + NM_BLK_WORDS + NM_CP_WORDS, misc,
                reinterpret_cast<const NmLea*>(blk + NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS + 4)};
}
// The out-of-line functions below get the tables as TWO POINTERS - the staged part in LDS, the whole in global memory - and put the NmTabs
// together themselves: as a 56-byte argument by value it went through scratch memory (a copy per call and lane), and on the device - not on
// the emulated one - a kernel whose out-of-line callee took a few bytes more of arguments faulted at address 0.
__device__ __forceinline__ NmTabs tabs_from(const TabLds* s, const NmTwo* __restrict__ two) {
  const uint32_t* blk = reinterpret_cast<const uint32_t*>(two + NM_TWO_SIZE);
  return NmTabs{s->two, two, s->blk, blk + NM_BLK_WORDS, blk + NM_BLK_WORDS + NM_CP_WORDS, s->misc, reinterpret_cast<const NmLea*>(blk + NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS + 4)};
}

// Bytes beyond ASCII are the exception (a dword of plain ASCII never gets here), and what they need is long: kept OUT of line, so that the
// unrolled loops of the kernels stay short enough for the instruction cache (inlined into every copy of a loop body, the classifier and the
// two-byte / Hangul output code made k_norm_emit2 57 % larger and 7 % slower on text that has none of these characters).
// the character that begins at raw_x, byte x of a staged range of `n` bytes (nm_classify_char; what lies outside the range reads as 0)
__device__ __noinline__ uint32_t classify_high_char(const uint8_t* raw_x, int x, int n, const TabLds* ts, const NmTwo* two) {
  const NmTabs tabs = tabs_from(ts, two);
  return nm_classify_char(raw_x[0], x >= 1 ? raw_x[-1] : 0u, x >= 2 ? raw_x[-2] : 0u, x >= 3 ? raw_x[-3] : 0u, x + 1 < n ? raw_x[1] : 0u, x + 2 < n ? raw_x[2] : 0u,
                          x + 3 < n ? raw_x[3] : 0u, tabs);
}
// what the lane of a byte >= 0x80 emits in k_norm_emit2 (tm_norm_masks.h): the bytes of a two-byte character come from the table - the lead
// lane its first byte, or the ASCII letter the character decomposes into; the second lane its second byte, or the two bytes of the combining
// mark -; every lane of a Hangul syllable (NFD) emits the three bytes of one of its jamo, or - the third lane of a syllable without a final
// consonant - nothing at all.  In: r = the byte in LDS, fl its class byte, code its rule-table entry; o = {o3, ysp, m3, len1} as the rule
// table left them.  Returns the same four, len1 = 0xFF for "no byte at all".
struct HighOut { uint32_t o3, ysp, m3, len1; };
__device__ __noinline__ HighOut emit_high_byte(const uint8_t* r, uint32_t fl, uint32_t code, HighOut o, const TabLds* ts, const NmTwo* two) {
  const NmTabs tabs = tabs_from(ts, two);
  const uint32_t b = r[0], bm1 = r[-1], bp1 = r[1];
  const bool lead2 = nm_two_lead(b), cont2 = nm_cont_byte(b) && nm_two_lead(bm1);
  if (lead2 || cont2) {
    const NmTwo e = nm_two_get(tabs, lead2 ? nm_two_index(b, bp1) : nm_two_index(bm1, b));
    uint32_t y = 0, mm = 0;
    const uint32_t extra = nm_two_out(e, cont2, (code & 4u) != 0, true, &o.o3, &y, &mm);
    if (extra >= 1u) { o.len1 = extra; o.ysp = y; o.m3 = mm; }
  } else {
    // a byte of a three-byte character that changes under NFD (one decoding of the character, then by its range - the characters that come here
    // for nothing, general punctuation and ideographs, leave after four compares)
    uint32_t role, cp;
    if (fl != NF_BAD && (tabs.misc & (NM_MISC_LEA | NM_MISC_KANA | NM_MISC_DEC3 | NM_MISC_HANGUL)) && nm_three_role(b, bm1, r[-2], bp1, r[2], &role, &cp)) {
      if ((tabs.misc & NM_MISC_LEA) && cp - 0x1E00u < (uint32_t)NM_LEA_SIZE) {
        // a letter of Latin Extended Additional: the letter, its first mark, its second mark or nothing
        const NmLea e = tabs.lea[cp - 0x1E00u];
        if (e.a & NT_OK) {
          if (role == 0u) o.o3 = (code & 4u) ? ((e.a >> 16) & 0xFFu) : ((e.a >> 8) & 0xFFu);
          else if (role == 1u) { o.len1 = 1u; o.ysp = e.b & 0xFFu; o.o3 = (e.b >> 8) & 0xFFu; }
          else if (((e.a >> 24) & 3u) == 2u) { o.len1 = 1u; o.ysp = (e.b >> 16) & 0xFFu; o.o3 = e.b >> 24; }
          else o.len1 = 0xFFu;
        }
      } else if ((tabs.misc & NM_MISC_KANA) && cp - 0x3040u < (uint32_t)NM_KANA_SIZE) {
        // a voiced kana: the base kana, the mark, nothing
        const uint32_t e = nm_kana_tab(tabs)[cp - 0x3040u];
        if (e & NK_OK) o.len1 = nm_kana_out(e, role, &o.m3, &o.ysp, &o.o3) ? 2u : 0xFFu;
      } else if ((tabs.misc & NM_MISC_DEC3) && cp - NM_DEC3_BASE < NM_DEC3_SIZE) {
        // a character NFD splits in two three-byte ones: the first, the second, nothing
        const uint32_t e = nm_dec3_tab(tabs)[cp - NM_DEC3_BASE];
        if (e & ND_OK) o.len1 = nm_dec3_out(tabs, e, role, &o.m3, &o.ysp, &o.o3) ? 2u : 0xFFu;
      } else if ((tabs.misc & NM_MISC_HANGUL) && nm_hangul(cp)) {
        // a Hangul syllable: one of its jamo - or nothing
        o.len1 = nm_hangul_out(cp, role, &o.m3, &o.ysp, &o.o3) ? 2u : 0xFFu;
      }
    }
  }
  return o;
}

// stage the piece (+ margins) and classify every byte; continuation bytes inherit the class of their lead byte.
// returns the piece length; LDS index of document byte (pb + i) is PMARGIN + i.
// The staged range is a WINDOW of the wavefront on the raw text (tm_device.h: a buffer resource cut to the document): what lies outside the
// document reads as 0 - class O - without a compare or a branch per dword (the loop this replaces spent 18 scalar instructions per step on
// 64-bit range tests and exec masks, on a kernel that is bound by its scalar instructions).
template <typename LDS>
__device__ __forceinline__ int norm_load_piece(LDS& L, const uint8_t* __restrict__ raw, uint64_t rb, uint64_t re, uint64_t pb, int lane,
                                               const uint8_t* s_cls, const TabLds* ts, const NmTwo* __restrict__ two) {
  const uint64_t left = re - pb;
  const uint32_t before = pb != rb ? (uint32_t)PMARGIN : 0u;            // (pb - rb is a multiple of PIECE: the whole margin in front, or none of it)
  const uint32_t after = left > (uint64_t)(PIECE + PMARGIN) ? (uint32_t)(PIECE + PMARGIN) : (uint32_t)left;
  const uint32_t a = (uint32_t)PMARGIN - before, e = (uint32_t)PMARGIN + after;      // LDS indices of the first byte of the document in the range, and one past its last
  const TmWindow win = tm_window(raw + (pb - before), (before + after) & ~3u);        // whole dwords only: a dword that straddles the document's end is outside
  constexpr int STEPS = (PLDS / 4 + 63) / 64;
  uint32_t w4[STEPS], high = 0u;
#pragma unroll
  for (int s = 0; s < STEPS; s++) w4[s] = tm_window_u32(win, (uint32_t)(4 * (lane + 64 * s)) - a);       // (a is a multiple of 4: the dwords of the range are the dwords of the window)
#pragma unroll
  for (int s = 0; s < STEPS; s++) {
    const int i = lane + 64 * s;
    if (s < STEPS - 1 || i < PLDS / 4) {
      const uint32_t v = w4[s];
      reinterpret_cast<uint32_t*>(L.raw)[i] = v;
      // four table reads classify a dword of ASCII; a dword with anything else in it is done again below, byte by byte
      reinterpret_cast<uint32_t*>(L.f)[i] = (uint32_t)s_cls[v & 0x7Fu] | ((uint32_t)s_cls[(v >> 8) & 0x7Fu] << 8) | ((uint32_t)s_cls[(v >> 16) & 0x7Fu] << 16) | ((uint32_t)s_cls[(v >> 24) & 0x7Fu] << 24);
      high |= v;
    }
  }
  if (lane < 32) L.chg[lane] = 0;
  // the last dword of the document may be a partial one: its bytes one by one (behind the zero the loop above has put there)
  __builtin_amdgcn_wave_barrier();
  const uint32_t tail = e & 3u;
  if ((uint32_t)lane < tail) {
    const uint32_t x = (e & ~3u) + (uint32_t)lane, bt = raw[pb + x - (uint32_t)PMARGIN];
    L.raw[x] = (uint8_t)bt;
    L.f[x] = bt < 0x80u ? s_cls[bt] : (uint8_t)0;
    high |= bt;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  if (__ballot((high & 0x80808080u) != 0u) != 0ull) {
    // bytes beyond ASCII somewhere in the range (the exception): their dwords again.  A character is classified ONCE, at its first byte, by the
    // classifier that looks three bytes either way, and the lane that holds that byte writes the class bytes of the whole character (text in
    // another script is two- and three-byte characters from end to end: a decoding per byte was most of what the pass took there - 13 - 17 ms
    // per GiB against 3); every byte beyond ASCII is NF_BAD beforehand, which is what is left of a byte no well-formed character claims.
#pragma unroll 1
    for (int i = lane; i < PLDS / 4; i += 64) {
      const uint32_t v = reinterpret_cast<const uint32_t*>(L.raw)[i];
      if ((v & 0x80808080u) != 0u) {
        uint32_t f4 = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int x = 4 * i + q;
          const uint32_t b = (v >> (8 * q)) & 0xFFu;
          const uint32_t fl = b < 0x80u ? (uint32_t)s_cls[b] : ((x >= 3 && x < PLDS - 3) ? (uint32_t)NF_BAD : 0u);      // (the three bytes at either end of the staged range are never looked at)
          f4 |= fl << (8 * q);
        }
        reinterpret_cast<uint32_t*>(L.f)[i] = f4;
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
#pragma unroll 1
    for (int i = lane; i < PLDS / 4; i += 64) {
      const uint32_t v = reinterpret_cast<const uint32_t*>(L.raw)[i];
      // the bytes >= 0xC0 of the dword, one after the other: a character begins at each (as many trips as the lane with the most of them has -
      // two in text of three-byte characters, where a loop over the four byte positions makes four calls, each for a third of the lanes)
      // (this shape and no other: as `for (lm = ...; lm != 0; lm &= lm - 1)` with a `continue` behind the call and a loop over the character's bytes,
      // k_norm_emit<3> - and only it - came out with wrong class bytes on the device; profiles/r06_scripts_on_device.txt)
      uint32_t lm = v & (v << 1) & 0x80808080u;
#pragma unroll 1
      while (lm != 0u) {
        const int x = 4 * i + (__builtin_ctz(lm) >> 3);
        lm &= lm - 1u;
        const uint32_t r = classify_high_char(L.raw + x, x, PLDS, ts, two);
        const uint32_t c0 = r & 0xFFu, c1 = (r >> 8) & 0xFFu, nb = c0 == NF_BAD ? 0u : (r >> 16) & 0xFFu;
        uint8_t* f = L.f + x;
        if (nb >= 1u && x >= 3 && x < PLDS - 3) f[0] = (uint8_t)c0;
        if (nb >= 2u && x + 1 >= 3 && x + 1 < PLDS - 3) f[1] = (uint8_t)c1;
        if (nb >= 3u && x + 2 >= 3 && x + 2 < PLDS - 3) f[2] = (uint8_t)c1;
        if (nb >= 4u && x + 3 >= 3 && x + 3 < PLDS - 3) f[3] = (uint8_t)c1;
        if ((r >> 24) != 0u && nb != 0u) {                     // a character the pass changes: its chunk(s) of the piece (every writer writes 1)
          const uint32_t i0 = (uint32_t)(x - PMARGIN), i1 = i0 + nb - 1u;
          if (i0 < (uint32_t)PIECE) L.chg[i0 >> 6] = 1;
          if (i1 < (uint32_t)PIECE) L.chg[i1 >> 6] = 1;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
  }
  return left > (uint64_t)PIECE ? PIECE : (int)left;
}

__global__ __launch_bounds__(256) void k_norm_summary(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ rbegin,
                                                      const uint64_t* __restrict__ rend, const uint32_t* __restrict__ piece_doc,
                                                      const uint64_t* __restrict__ doc_piece_start, uint64_t npieces, uint32_t lower_all,
                                                      const NmTwo* __restrict__ two, uint32_t* __restrict__ piece_sum) {
  __shared__ PieceLds s_l[4];
  __shared__ uint8_t s_cls[128];
  __shared__ TabLds s_tab;
  if (threadIdx.x < 128) s_cls[threadIdx.x] = (uint8_t)ncls_ascii(threadIdx.x, lower_all != 0);
  const NmTabs tabs = stage_tabs(s_tab, two);
  __syncthreads();
  // (wave-uniform wavefront index: the run bookkeeping below is arithmetic on ballots and then runs on the scalar unit)
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t k = (uint64_t)blockIdx.x * 4 + wv;
  if (k >= npieces) return;
  PieceLds& L = s_l[wv];
  const uint32_t d = piece_doc[k];
  const uint64_t rb = rbegin[d], re = rend[d], pb = rb + (k - doc_piece_start[d]) * PIECE;
  const int m = __builtin_amdgcn_readfirstlane(norm_load_piece(L, raw, rb, re, pb, lane, s_cls, &s_tab, two));
  bool lead_open = true, lead_tl = false, bad = false;
  uint32_t lead_u = 0, trail_u = 0;
  for (int c = 0; c * 64 < m; c++) {
    const int i = c * 64 + lane;
    const bool in = i < m;
    const uint32_t fl = in ? L.f[PMARGIN + i] : 0u, cls = fl & NF_CLASS;
    bad |= in && fl == NF_BAD;
    const unsigned long long V = __ballot(in), mB = __ballot(in && fl != NF_BAD && nblock(cls)), mU = __ballot(in && fl != NF_BAD && cls == NC_U),
                             mL = __ballot(in && fl != NF_BAD && cls == NC_L);
    const unsigned long long nonblock = V & ~mB;
    if (lead_open) {
      if (nonblock != 0) {
        const int e = __ffsll((long long)nonblock) - 1;
        lead_u = min(lead_u + (uint32_t)__popcll(mU & ((1ull << e) - 1ull)), 2u);
        lead_tl = (mL >> e) & 1ull;
        lead_open = false;
      } else lead_u = min(lead_u + (uint32_t)__popcll(mU), 2u);
    }
    if (nonblock != 0) {
      const int hi = 63 - __clzll((long long)nonblock);
      trail_u = min((uint32_t)__popcll(hi == 63 ? 0ull : (mU & (~0ull << (hi + 1)))), 2u);
    } else trail_u = min(trail_u + (uint32_t)__popcll(mU), 2u);
  }
  bad = __any(bad);
  if (lane == 0) {
    const uint32_t f0 = L.f[PMARGIN], c0 = f0 & NF_CLASS;
    uint32_t s = (lead_open ? PS_WHOLE : 0u) | (lead_u << PS_LEADU_SHIFT) | (lead_tl ? PS_LEADTL : 0u) | (trail_u << PS_TRAILU_SHIFT);
    if (m > 0 && f0 != NF_BAD && nblock(c0)) s |= PS_FIRSTBLOCK;
    if (m > 0 && f0 != NF_BAD && c0 == NC_L) s |= PS_FIRSTL;
    if (bad) s |= PS_BAD;
    piece_sum[k] = s;
  }
}

// carry byte of a piece: ub[0..1] | ua[2..3] | tL[4]
__global__ void k_norm_carry(const uint32_t* __restrict__ piece_sum, const uint64_t* __restrict__ doc_piece_start, uint32_t ndocs,
                             uint8_t* __restrict__ piece_carry, uint8_t* __restrict__ need_host, unsigned long long* __restrict__ ninfo,
                             uint32_t* __restrict__ fb_ids, uint32_t all_host) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= ndocs) return;
  const uint64_t ps = doc_piece_start[d], pe = doc_piece_start[d + 1];
  uint32_t ub = 0;
  bool bad = all_host != 0;        // normalizer flags the device pass does not implement: every document takes the host path
  for (uint64_t k = ps; k < pe; k++) {
    const uint32_t s = piece_sum[k];
    piece_carry[k] = (uint8_t)ub;
    bad |= (s & PS_BAD) != 0;
    if (s & PS_WHOLE) ub = min(ub + ((s >> PS_LEADU_SHIFT) & 3u), 2u);
    else ub = (s >> PS_TRAILU_SHIFT) & 3u;
  }
  uint32_t ua = 0, tl = 0;
  for (uint64_t k = pe; k > ps; k--) {
    const uint32_t s = piece_sum[k - 1];
    piece_carry[k - 1] = (uint8_t)(piece_carry[k - 1] | (ua << 2) | (tl << 4));
    if (s & PS_WHOLE) ua = min(ua + ((s >> PS_LEADU_SHIFT) & 3u), 2u);
    else if (s & PS_FIRSTBLOCK) { ua = (s >> PS_LEADU_SHIFT) & 3u; tl = (s & PS_LEADTL) ? 1u : 0u; }
    else { ua = 0; tl = (s & PS_FIRSTL) ? 1u : 0u; }
  }
  need_host[d] = bad ? 1 : 0;
  if (bad) fb_ids[atomicAdd(&ninfo[0], 1ull)] = d;           // the documents the host has to normalize, in no particular order
}

// MODE 0: normalized length of every piece.  MODE 1: the bytes, packed at piece_off.  MODE 2: the bytes into the piece's
// private slab (SLAB bytes apart; a piece that would not fit raises the overflow flag) and the length.  MODE 3: a vocabulary WITHOUT
// capcode in one pass, as k_norm_emit2<false> is for capcode 2: nothing is known about the documents beforehand (no k_norm_summary /
// k_norm_carry: without capcode a byte's output depends on nothing but its character), the bytes go into the slabs, and a piece that finds
// a byte it cannot normalize marks its document in need_host.  MODE 4: the origin pass behind tm_batch_raw_spans - the same path over the
// resident raw text with the carries given, but no text: for every normalized byte, packed at piece_off like MODE 1's text, the offset in the
// raw document of the first byte of the character whose lane wrote it (`out` is that array of u32; need_host and piece_len are only read).
constexpr int SLAB = 2 * PIECE;
// the first byte of the character that byte x of a staged piece belongs to: steps back over its continuation bytes (the documents the device
// normalizes are well-formed UTF-8: anything else is NF_BAD and the host's)
__device__ __forceinline__ uint32_t norm_lead_back(const uint8_t* raw_x) {
  uint32_t back = 0;
  while (back < 3u && (raw_x[-(int)back] & 0xC0u) == 0x80u) back++;
  return back;
}
static_assert(SLAB == SLAB_BYTES, "k_match_branch stages the text from these slabs");
static_assert(PIECE == RAW_PIECE, "the ring's issuer counts the pieces of a chunk (tm_host.hip)");
template <int MODE>
__global__ __launch_bounds__(256) void k_norm_emit(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ rbegin,
                                                   const uint64_t* __restrict__ rend, const uint32_t* __restrict__ piece_doc,
                                                   const uint64_t* __restrict__ doc_piece_start, uint64_t npieces, uint32_t capcode,
                                                   uint32_t lower_all, const uint8_t* __restrict__ piece_carry,
                                                   uint8_t* __restrict__ need_host, uint32_t* __restrict__ piece_len,
                                                   const uint64_t* __restrict__ piece_off, uint8_t* __restrict__ out,
                                                   unsigned long long* __restrict__ overflow, const NmTwo* __restrict__ two,
                                                   const uint64_t* __restrict__ np_dev) {
  constexpr bool WRITE = MODE != 0;
  if (np_dev) npieces = min(npieces, np_dev[0]);       // (the ring behind a filter pass: launched over a bound, the count is the device's)
  __shared__ PieceLds s_l[4];
  __shared__ uint8_t s_cls[128];
  __shared__ TabLds s_tab;
  if (threadIdx.x < 128) s_cls[threadIdx.x] = (uint8_t)ncls_ascii(threadIdx.x, lower_all != 0);
  const NmTabs tabs = stage_tabs(s_tab, two);
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t k = (uint64_t)blockIdx.x * 4 + wv;
  if (k >= npieces) return;
  PieceLds& L = s_l[wv];
  const uint32_t d = piece_doc[k];
  if (MODE != 3 && need_host[d]) { if (MODE != 1 && MODE != 4 && lane == 0) piece_len[k] = 0; return; }
  const uint64_t rb = rbegin[d], re = rend[d], pb = rb + (k - doc_piece_start[d]) * PIECE;
  const int m = norm_load_piece(L, raw, rb, re, pb, lane, s_cls, &s_tab, two);
  uint8_t* dst = MODE == 1 ? out + piece_off[k] : ((MODE == 2 || MODE == 3) ? out + k * (uint64_t)SLAB : nullptr);
  // MODE 4: where the piece's owners go, what they count from, and how many there are (the pass that wrote the text left the length)
  uint32_t* own = MODE == 4 ? reinterpret_cast<uint32_t*>(out) + piece_off[k] : nullptr;
  const uint32_t own_base = MODE == 4 ? (uint32_t)(pb - rb) : 0u, own_n = MODE == 4 ? piece_len[k] : 0u;
  if (MODE == 4 && capcode != 2) {                          // no capcode: byte i of the piece is byte i of its output
    for (int i = lane; i < m && (uint32_t)i < own_n; i += 64) own[i] = own_base + (uint32_t)i - norm_lead_back(L.raw + PMARGIN + i);
    return;
  }
  if (capcode != 2 || MODE == 3) {                          // no capcode: same length, only the lower-case flag applies
    if (MODE != 1 && lane == 0) piece_len[k] = (uint32_t)m;
    bool bad = false;
    if (WRITE) for (int i = lane; i < m; i += 64) {
      const int x = PMARGIN + i;
      if (MODE == 3) bad |= L.f[x] == NF_BAD;
      uint32_t b = L.raw[x], y = 0, m3 = 0;
      if (lower_all && b - 'A' < 26u) b |= 0x20u;
      const uint32_t bm1 = L.raw[x - 1];
      // (a two-byte character that stays one: its bytes under the vocabulary's flags; those that decompose are not in this table)
      if (nm_two_lead(b)) (void)nm_two_out(nm_two_get(tabs, nm_two_index(b, L.raw[x + 1])), false, false, false, &b, &y, &m3);
      else if (nm_cont_byte(b) && nm_two_lead(bm1)) (void)nm_two_out(nm_two_get(tabs, nm_two_index(bm1, b)), true, false, false, &b, &y, &m3);
      dst[i] = (uint8_t)b;
    }
    if (MODE == 3 && __any(bad) && lane == 0) need_host[d] = 1;      // (every writer writes 1; the piece lengths of such a document are zeroed by k_norm_bad)
    return;
  }
  const uint32_t carry = piece_carry[k];
  const unsigned long long below = (1ull << lane) - 1ull;
  // ---- backward sweep: ua and tL of every block byte --------------------------------------------------------------
  {
    uint32_t carry_ua = (carry >> 2) & 3u;
    bool carry_tl = (carry >> 4) & 1u;
    for (int c = (m - 1) / 64; c >= 0; c--) {
      const int i = c * 64 + lane;
      const bool in = i < m;
      const uint32_t fl = in ? L.f[PMARGIN + i] : 0u, cls = fl & NF_CLASS;
      const unsigned long long V = __ballot(in), mB = __ballot(in && nblock(cls)), mU = __ballot(in && cls == NC_U), mL = __ballot(in && cls == NC_L);
      const unsigned long long above = lane == 63 ? 0ull : (~0ull << (lane + 1));
      const unsigned long long stop = V & ~mB & above;         // first non-block byte to my right inside the chunk
      uint32_t ua;
      bool tl;
      if (stop != 0) {
        const int e = __ffsll((long long)stop) - 1;
        ua = (uint32_t)__popcll(mU & above & ((1ull << e) - 1ull));
        tl = (mL >> e) & 1ull;
      } else {
        ua = (uint32_t)__popcll(mU & above) + carry_ua;
        tl = carry_tl;
      }
      ua = min(ua, 2u);
      if (in && nblock(cls)) L.f[PMARGIN + i] = (uint8_t)(fl | (tl ? NF_TERML : 0u) | (ua << NF_UA_SHIFT));
      const uint32_t ua0 = __shfl(ua, 0), cls0 = __shfl(cls, 0);
      const bool tl0 = __shfl((int)tl, 0) != 0;
      if (nblock(cls0)) { carry_ua = min(ua0 + (cls0 == NC_U ? 1u : 0u), 2u); carry_tl = tl0; }
      else { carry_ua = 0; carry_tl = cls0 == NC_L; }
    }
  }
  // tL of the first byte of the NEXT piece (a space at the very end of this piece may turn into its marker)
  const bool next_tl = (carry >> 4) & 1u;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  // ---- forward sweep: ub, then every character's output ------------------------------------------------------------
  uint32_t carry_ub = carry & 3u;
  uint32_t pos = 0;
  for (int c = 0; c * 64 < m; c++) {
    const int i = c * 64 + lane, x = PMARGIN + i;
    const bool in = i < m;
    const uint32_t fl = in ? L.f[x] : 0u, cls = fl & NF_CLASS;
    const unsigned long long mB = __ballot(in && nblock(cls)), mU = __ballot(in && cls == NC_U);
    const unsigned long long gap = ~mB & below;                // non-block bytes to my left inside the chunk
    uint32_t ub;
    if (gap != 0) {
      const int s = 64 - __clzll((long long)gap);
      ub = (uint32_t)__popcll(mU & below & ~((1ull << s) - 1ull));
    } else ub = (uint32_t)__popcll(mU & below) + carry_ub;
    ub = min(ub, 2u);
    {
      const uint32_t ub63 = __shfl(ub, 63), cls63 = __shfl(cls, 63);
      carry_ub = nblock(cls63) ? min(ub63 + (cls63 == NC_U ? 1u : 0u), 2u) : 0u;
    }
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0, len = 0;
    if (in) {
      const uint32_t b = L.raw[x];
      const uint32_t fm1 = L.f[x - 1], P = fm1 & NF_CLASS;
      uint32_t P2 = NC_O;
      if (P == NC_AP) P2 = L.f[(fm1 & NF_CONT) ? x - 4 : x - 2] & NF_CLASS;
      const bool inword = ub >= 1;                             // javascript/tokenmonster.js `inWord` before this character
      const bool tl = (fl & NF_TERML) != 0;
      // the rules themselves are the ones k_norm_emit2 reads from its table (tm_norm_masks.h: nm_lut_entry); what this kernel does
      // differently is how it finds inWord and the 'C' look-ahead (per-lane counting instead of flood fills on the ballots)
      const uint32_t code = nm_lut_entry(nm_lut_index((fl & NF_CONT) ? (uint32_t)NC_O : cls, P, P2, inword ? 1u : 0u, tl ? 1u : 0u), lower_all != 0);
      len = (code & 3u) + 1u;
      o0 = 'D'; o1 = code >> 8; o2 = ' ';
      o3 = b | ((code & 4u) << 3);
      if (cls == NC_SP) {
        const bool last = i + 1 == m;                          // the next byte lives in the next piece (or nowhere)
        const uint32_t fp1 = L.f[x + 1];
        if ((fp1 & NF_CLASS) == NC_U && fp1 != NF_BAD && !(fp1 & NF_CONT)) o3 = (last ? next_tl : (fp1 & NF_TERML) != 0) ? 'C' : 'W';   // :976-979
      }
      // one byte of a two-byte character: its bytes come from the table (a decomposed character's second half emits the two bytes of the mark)
      const uint32_t bm1 = L.raw[x - 1];
      const bool lead2 = nm_two_lead(b), cont2 = nm_cont_byte(b) && nm_two_lead(bm1);
      if (lead2 || cont2) {
        const NmTwo e = nm_two_get(tabs, lead2 ? nm_two_index(b, L.raw[x + 1]) : nm_two_index(bm1, b));
        uint32_t y = 0, m3 = 0;
        const uint32_t extra = nm_two_out(e, cont2, (code & 4u) != 0, true, &o3, &y, &m3);
        if (extra >= 1u) { len = 1u + extra; o2 = y; o1 = m3; }
      }
      // one byte of a Hangul syllable (NFD): its lane emits one of the syllable's jamo - or nothing (tm_norm_masks.h)
      uint32_t hrole, hcp;
      if ((tabs.misc & NM_MISC_HANGUL) && fl != NF_BAD && nm_hangul_role(b, bm1, L.raw[x - 2], L.raw[x + 1], L.raw[x + 2], &hrole, &hcp)) len = nm_hangul_out(hcp, hrole, &o1, &o2, &o3);
      // ... or of a letter of Latin Extended Additional (NFD): the letter, its first mark, its second mark or nothing
      uint32_t lrole, lidx;
      if ((tabs.misc & NM_MISC_LEA) && fl != NF_BAD && nm_lea_role(b, bm1, L.raw[x - 2], L.raw[x + 1], L.raw[x + 2], &lrole, &lidx) && (tabs.lea[lidx].a & NT_OK)) {
        const NmLea le = tabs.lea[lidx];
        if (lrole == 0u) o3 = (code & 4u) ? ((le.a >> 16) & 0xFFu) : ((le.a >> 8) & 0xFFu);
        else if (lrole == 1u) { len = 2u; o2 = le.b & 0xFFu; o3 = (le.b >> 8) & 0xFFu; }
        else if (((le.a >> 24) & 3u) == 2u) { len = 2u; o2 = (le.b >> 16) & 0xFFu; o3 = le.b >> 24; }
        else len = 0u;
      }
      // ... or of a voiced kana (NFD): the base kana, the mark, nothing
      uint32_t krole, kidx;
      if ((tabs.misc & NM_MISC_KANA) && fl != NF_BAD && nm_kana_role(b, bm1, L.raw[x - 2], L.raw[x + 1], L.raw[x + 2], &krole, &kidx) && (nm_kana_tab(tabs)[kidx] & NK_OK))
        len = nm_kana_out(nm_kana_tab(tabs)[kidx], krole, &o1, &o2, &o3);
      // ... or of a character NFD splits in two three-byte ones
      uint32_t drole, dcp;
      if ((tabs.misc & NM_MISC_DEC3) && fl != NF_BAD && nm_three_role(b, bm1, L.raw[x - 2], L.raw[x + 1], L.raw[x + 2], &drole, &dcp) && (nm_dec3(tabs, dcp) & ND_OK))
        len = nm_dec3_out(tabs, nm_dec3(tabs, dcp), drole, &o1, &o2, &o3);
    }
    // inclusive prefix sum of len (0..4) over the wavefront: bytes-with-len>=k ballots, counted below the lane
    uint32_t incl = len;
#pragma unroll
    for (uint32_t q = 1; q <= 4; q++) {
      const unsigned long long bq = __ballot(len >= q);
      incl = __builtin_amdgcn_mbcnt_hi((uint32_t)(bq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bq, incl));
    }
    if (MODE == 4) {
      if (in && pos + incl <= own_n) {
        const uint32_t o = own_base + (uint32_t)i - norm_lead_back(L.raw + x);
        uint32_t* w = own + pos + (incl - len);
        for (uint32_t q = 0; q < len; q++) w[q] = o;
      }
    } else if (WRITE && in && (MODE == 1 || pos + incl <= (uint32_t)SLAB)) {
      uint8_t* w = dst + pos + (incl - len);
      if (len == 4) { w[0] = (uint8_t)o0; w[1] = (uint8_t)o1; w[2] = (uint8_t)o2; w[3] = (uint8_t)o3; }
      else if (len == 3) { w[0] = (uint8_t)o1; w[1] = (uint8_t)o2; w[2] = (uint8_t)o3; }
      else if (len == 2) { w[0] = (uint8_t)o2; w[1] = (uint8_t)o3; }
      else if (len == 1) w[0] = (uint8_t)o3;
    }
    pos += __shfl(incl, 63);
  }
  if (MODE != 1 && MODE != 4 && lane == 0) {
    piece_len[k] = pos;
    if (MODE == 2 && pos > (uint32_t)SLAB) atomicAdd(overflow, 1ull);
  }
}

// ---- capcode level 2, one pass into the slabs ------------------------------------------------------------------------------
// Same rules as k_norm_emit (which stays for the exact two-pass path and for capcode 0) at ~40 % of its vector instructions
// (the normalizer is bound by vector-instruction issue like the match kernel): the two run-dependent facts of a byte — inWord
// and the 'C'/'W' lookahead — are flood fills on the chunk's class ballots, done by the scalar unit; the rule chain is a
// 2048-entry table in LDS (tm_norm_masks.h; both checked on the CPU by tools/norm_masks_check.cpp); the output is assembled in
// LDS and leaves for the slab in 16-byte stores.
struct PieceLds2 { uint8_t raw[PLDS]; uint8_t f[PLDS]; uint8_t chg[32]; alignas(16) uint8_t out[2 * PIECE + 64]; };   // out: slab image + one dump byte per lane

__device__ const NmLut g_norm_lut = nm_make_lut();

// CARRY = true: the carries of the piece (inWord at its first byte, how the block at its end ends) and the documents that need the host
// normalizer are known (k_norm_summary + k_norm_carry have run: the exact path).  CARRY = false (the usual path): no pass before this
// one — the carries come from the 64 bytes either side of the piece (nm_margin_carries), a piece whose margins cannot tell raises
// overflow[1] and the exact path runs after all; a piece that finds a byte it cannot normalize marks its document in need_host.
#ifndef TM_NORM_UNROLL
#define TM_NORM_UNROLL 2
#endif
template <bool CARRY>
__global__ __launch_bounds__(256) void k_norm_emit2(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ rbegin,
                                                    const uint64_t* __restrict__ rend, const uint32_t* __restrict__ piece_doc,
                                                    const uint64_t* __restrict__ doc_piece_start, uint64_t npieces, uint32_t lower_all,
                                                    const uint8_t* __restrict__ piece_carry, uint8_t* __restrict__ need_host,
                                                    uint32_t* __restrict__ piece_len, uint8_t* __restrict__ slab,
                                                    unsigned long long* __restrict__ overflow, const NmTwo* __restrict__ two,
                                                    const uint64_t* __restrict__ np_dev) {
  constexpr int SLAB2 = 2 * PIECE, NCH = PIECE / 64;
  if (np_dev) npieces = min(npieces, np_dev[0]);       // (the ring behind a filter pass: launched over a bound, the count is the device's)
  __shared__ PieceLds2 s_l[4];
  __shared__ uint8_t s_cls[128];
  __shared__ TabLds s_tab;
  const NmTabs tabs = stage_tabs(s_tab, two);
  alignas(16) __shared__ uint16_t s_lut[NM_LUT_SIZE];
  static_assert(NM_LUT_SIZE * sizeof(uint16_t) == 256 * sizeof(uint4), "one 16-byte load per thread stages the rule table");
  if (threadIdx.x < 128) s_cls[threadIdx.x] = (uint8_t)ncls_ascii(threadIdx.x, lower_all != 0);
  reinterpret_cast<uint4*>(s_lut)[threadIdx.x] = reinterpret_cast<const uint4*>(g_norm_lut.e[lower_all ? 1 : 0])[threadIdx.x];
  __syncthreads();
  // the wavefront index is made visibly wave-uniform: everything derived from it (piece, length, carries) then lives in scalar
  // registers, and so does the mask algebra below
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  PieceLds2& L = s_l[wv];
  // A wavefront takes piece after piece (the grid: norm_grid()): the tables above are staged once per workgroup, not once per four pieces.
#pragma unroll 1
  for (uint64_t k = (uint64_t)blockIdx.x * 4 + wv; k < npieces; k += (uint64_t)gridDim.x * 4) {
  const uint32_t d = piece_doc[k];
  if (CARRY && need_host[d]) { if (lane == 0) piece_len[k] = 0; continue; }
  const uint64_t rb = rbegin[d], re = rend[d], pb = rb + (k - doc_piece_start[d]) * PIECE;
  const int m = __builtin_amdgcn_readfirstlane(norm_load_piece(L, raw, rb, re, pb, lane, s_cls, &s_tab, two));
  const uint32_t carry = CARRY ? __builtin_amdgcn_readfirstlane((uint32_t)piece_carry[k]) : 0u;
  const int nch = (m + 63) >> 6;
  const uint8_t* fl0 = L.f + PMARGIN + lane;       // class byte of byte (64 c + lane) of the piece = fl0[64 c]; chunk -1 and chunk NCH are the margins
  // (norm_load_piece has classified the LDS bytes from 66 before the piece to 66 after its 1024; behind the end of the document they are class O)
  unsigned long long w_seed = (carry & 3u) ? 1ull : 0ull;
  const unsigned long long t0_beyond = CARRY ? (unsigned long long)((carry >> 4) & 1u) : 0ull;       // T0 (tm_norm_masks.h) of what lies behind the margin: looked at only when all of the margin is one block
  if (!CARRY) {
    const uint32_t fb = fl0[-64], fa = m == PIECE ? (uint32_t)fl0[64 * NCH] : 0u;       // (a shorter piece is the last of its document: nothing follows)
    uint64_t w_in;
    const bool known = nm_margin_carries(__ballot((fb & NF_BLOCK) != 0), __ballot((fb & NF_CLASS) == NC_U), __ballot((fa & NF_BLOCK) != 0), &w_in);
    if (!known && lane == 0) atomicAdd(overflow + 1, 1ull);
    w_seed = w_in;
  }
  // ---- ONE sweep, forwards: W carried from chunk to chunk, T from the ballots of the chunk and of the one behind it (nm_t0 / nm_tx) -----------
  // No masks for the end of the document: the bytes behind it are class O, which take no part in anything and emit themselves - one zero
  // byte per lane, behind everything else in the output image, and subtracted from the length below.
  typedef TM_LDS_SPACE uint8_t lds_u8;
  const uint32_t out0 = TM_LDS_ADDR(L.out);
  const uint32_t dump = out0 + (uint32_t)SLAB2 + (uint32_t)lane;     // where a lane's "not this byte" stores go
  const uint32_t lim = out0 + (uint32_t)SLAB2;
  unsigned long long w = w_seed, badm = 0ull;
  uint32_t posabs = out0;                                             // LDS address of the next output byte (wave-uniform)
  bool over = false;
  uint32_t chC = 'C', chW = 'W', chSP = ' ', chD = 'D';
  TM_KEEP_IN_VGPRS4(chC, chW, chSP, chD);      // four registers for the whole sweep, not four moves per chunk
  const uint8_t* fc = fl0;                      // this lane's class byte in chunk c
  const uint8_t* rc = L.raw + PMARGIN + lane;   // and its byte
  uint32_t fl = fc[0];
  unsigned long long Bcur = __ballot((fl & NF_BLOCK) != 0), Lcur = __ballot((fl & NF_CLASS) == NC_L), Ucur = __ballot((fl & NF_CLASS) == NC_U);
  int c = 0;
  auto chunk = [&]() __attribute__((always_inline)) {
    // the chunk behind this one (chunk NCH is the margin): its capitals (its first byte may be the capital a trailing space announces), and what
    // a block that reaches the end of this chunk ends in
    const uint32_t fnext = fc[64];
    const unsigned long long Bn = __ballot((fnext & NF_BLOCK) != 0), Ln = __ballot((fnext & NF_CLASS) == NC_L), Un = __ballot((fnext & NF_CLASS) == NC_U);
    // (bit 63 set in what ctz looks at: defined when every byte is in the block, and no compare-and-select when - as good as always - not)
    unsigned long long t0n = Ln >> __builtin_ctzll(~Bn | (1ull << 63));
    if (__builtin_expect(Bn == ~0ull, 0)) {       // 64 bytes of one block behind this chunk: the first chunk behind that with anything else in it decides
      t0n = t0_beyond;
#pragma unroll 1
      for (int j = c + 2; j <= NCH; j++) {
        const uint32_t fj = fl0[64 * j];
        const unsigned long long Bj = __ballot((fj & NF_BLOCK) != 0), Lj = __ballot((fj & NF_CLASS) == NC_L);
        if (Bj != ~0ull) { t0n = nm_t0(Bj, Lj, 0ull); break; }
      }
    }
    const unsigned long long TXc = nm_tx(Bcur, Lcur, t0n);
    const uint32_t fp = fc[-1], f2 = fc[-2], f4 = fc[-4];
    const uint32_t b = rc[0];
    uint64_t w_out, spC, spW;
    if (!CARRY) badm |= __ballot(fl == NF_BAD);
    const unsigned long long W = nm_inword(Bcur, Ucur, ~0ull, w, &w_out);
    nm_space_markers(__ballot((fl & NF_CLASS) == NC_SP), Ucur, Un, ~0ull, TXc, t0n, &spC, &spW);
    w = w_out;
    // the rule table: index = class | previous class << 3 | class before the apostrophe << 6 | W << 9 | T << 10
    // (a continuation byte takes no part in the rules as a character of its own: class O here; as the PREVIOUS byte it stands for its character)
    const uint32_t p2 = (fp & NF_CONT) ? f4 : f2;
    uint32_t idx = ((fl & NF_CONT) ? (uint32_t)NC_O : (fl & 7u)) | ((fp & 7u) << 3) | ((p2 & 7u) << 6);
    idx = sel_mask(W, idx | 512u, idx);
    idx = sel_mask(TXc, idx | 1024u, idx);
    const uint32_t code = s_lut[idx];
    uint32_t len1 = code & 3u;                                         // bytes emitted - 1
    uint32_t o3 = b | ((code & 4u) << 3);
    o3 = sel_mask(spC, chC, o3);
    o3 = sel_mask(spW, chW, o3);
    uint32_t ysp = chSP, m3 = code >> 8;
    // Everything a character beyond ASCII needs sits behind ONE test of the chunk and out of line (emit_high_byte): chunks of plain ASCII are
    // the rule.  E = the lanes that emit at least one byte: all, but for the third lane of a Hangul syllable without a final consonant.
    unsigned long long E = ~0ull;
    uint32_t below = posabs + (uint32_t)lane, n = len1 + 1u;           // first output byte of the lane before the extra bytes of the lanes below it; bytes it emits
    if (__ballot(b >= 0x80u) != 0ull && __builtin_amdgcn_readfirstlane((int)L.chg[c]) != 0) {      // (a chunk of nothing but inert characters - punctuation, ideographs, Thai ... - emits its bytes as they are)
      if (b >= 0x80u) {
        const HighOut h = emit_high_byte(rc, fl, code, HighOut{o3, ysp, m3, len1}, &s_tab, two);
        o3 = h.o3; ysp = h.ysp; m3 = h.m3; len1 = h.len1;
      }
      E = ~__ballot(len1 == 0xFFu);
      len1 = len1 == 0xFFu ? 0u : len1;
      n = sel_mask(E, len1 + 1u, 0u);
      below = mbcnt64(E, posabs);
    }
    const unsigned long long ge2 = __ballot(len1 >= 1u), ge3 = __ballot(len1 >= 2u), ge4 = __ballot(len1 >= 3u);
    // first output byte of the lane = the bytes of the lanes below behind posabs; its last byte is len1 further; the chunk ends where lane 63 does
    const uint32_t first = mbcnt64(ge4, mbcnt64(ge3, mbcnt64(ge2, below)));
    const uint32_t last = first + len1;
    const uint32_t end = read_lane(first + n, 63);
    if (end <= lim) {
      *TM_LDS_PTR(lds_u8, sel_mask(E, last, dump)) = (uint8_t)o3;
      *TM_LDS_PTR(lds_u8, sel_mask(ge2, last - 1u, dump)) = (uint8_t)ysp;
      *TM_LDS_PTR(lds_u8, sel_mask(ge3, last - 2u, dump)) = (uint8_t)m3;
      *TM_LDS_PTR(lds_u8, sel_mask(ge4, first, dump)) = (uint8_t)chD;
    } else over = true;                                   // wave-uniform: the piece does not fit its slab (exact two-pass path)
    posabs = end;
    fl = fnext; Bcur = Bn; Lcur = Ln; Ucur = Un;
    c++; fc += 64; rc += 64;
  };
  // (two chunks per trip: what the chunk behind hands on stays where it is instead of being copied back - five scalar moves and a branch per chunk)
#pragma unroll 1
  while (c + TM_NORM_UNROLL <= nch) {
#pragma unroll
    for (int u = 0; u < TM_NORM_UNROLL; u++) chunk();
  }
#pragma unroll 1
  while (c < nch) chunk();
  const uint32_t pos = posabs - out0 - (uint32_t)(64 * nch - m);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0);
  if (!over) {
    uint8_t* dst = slab + k * (uint64_t)SLAB2;
    for (uint32_t j = (uint32_t)lane * 16u; j < pos; j += 64u * 16u)
      *reinterpret_cast<uint4*>(dst + j) = *reinterpret_cast<const uint4*>(L.out + j);    // the slab is 16-byte aligned and 2 KiB long
  }
  if (lane == 0) {
    piece_len[k] = pos;
    if (over) atomicAdd(overflow, 1ull);             // (with the zero bytes of a last chunk counted in: a piece within 63 bytes of its slab's end may take the exact path for nothing)
    if (!CARRY && badm != 0ull) need_host[d] = 1;      // (every writer writes 1; the piece lengths of such a document are zeroed by k_norm_bad)
  }
  __builtin_amdgcn_wave_barrier();                     // (the output image is read above and written again by the next piece)
  }
}


// pieces per document; clears what the pass writes to on the side (need_host, the info words): no memset commands of their own
__global__ void k_norm_begin(const uint64_t* __restrict__ rbegin, const uint64_t* __restrict__ rend, uint32_t ndocs, uint32_t* __restrict__ doc_npiece, uint8_t* __restrict__ need_host,
                             unsigned long long* __restrict__ ninfo) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < 8) ninfo[d] = 0ull;
  if (d < ndocs) {
    doc_npiece[d] = (uint32_t)((rend[d] - rbegin[d] + PIECE - 1) / PIECE);
    need_host[d] = 0;
  }
}

// behind k_norm_emit2<false>: the pieces of the documents that turned out to need the host normalizer count for nothing, and those documents
// are listed for the host (in no particular order) - thread k looks at piece k and at document k
// ... and ninfo[6] counts the pieces that are not the last of their document yet shorter than what a segment looks at (TEXT_LEN): with one
// of those the text cannot be staged from the slabs by k_match_branch (which looks at two pieces at most) and is packed after all
__global__ void k_norm_bad(const uint32_t* __restrict__ piece_doc, const uint8_t* __restrict__ need_host, const uint64_t* __restrict__ doc_piece_start, uint64_t npieces,
                           uint32_t ndocs, uint32_t* __restrict__ piece_len, unsigned long long* __restrict__ ninfo, uint32_t* __restrict__ fb_ids,
                           const uint64_t* __restrict__ np_dev) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (np_dev && k >= np_dev[0]) { if (k < npieces) piece_len[k] = 0; }       // (launched over a bound: what lies behind the device's count is empty)
  else if (k < npieces) {
    const uint32_t d = piece_doc[k];
    if (need_host[d]) piece_len[k] = 0;
    else if (piece_len[k] < (uint32_t)TEXT_LEN && k + 1 != doc_piece_start[d + 1]) atomicAdd(&ninfo[6], 1ull);
  }
  if (k < ndocs && need_host[k]) fb_ids[atomicAdd(&ninfo[0], 1ull)] = (uint32_t)k;
}

// the exact path's share of k_norm_bad: ninfo[6] counts the pieces that are too short for the text to stay in the slabs
__global__ void k_norm_short(const uint32_t* __restrict__ piece_doc, const uint8_t* __restrict__ need_host, const uint64_t* __restrict__ doc_piece_start, uint64_t npieces,
                             const uint32_t* __restrict__ piece_len, unsigned long long* __restrict__ ninfo) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= npieces) return;
  const uint32_t d = piece_doc[k];
  if (!need_host[d] && piece_len[k] < (uint32_t)TEXT_LEN && k + 1 != doc_piece_start[d + 1]) atomicAdd(&ninfo[6], 1ull);
}

// pack the slabs: piece k's bytes go to out[piece_off[k] ..); a piece that would end behind `cap` bytes is left out (the caller - which
// has not seen the total yet when it launches this - then reports TM_E_LIMIT)
__global__ __launch_bounds__(256) void k_norm_compact(const uint8_t* __restrict__ slab, const uint32_t* __restrict__ piece_len,
                                                      const uint64_t* __restrict__ piece_off, uint64_t npieces, uint8_t* __restrict__ out, uint64_t cap) {
  const int lane = threadIdx.x & 63;
  const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= npieces) return;
  const uint32_t len = piece_len[k];
  if (piece_off[k] + len > cap) return;
  const uint8_t* src = slab + k * (uint64_t)SLAB;
  uint8_t* dst = out + piece_off[k];
  for (uint32_t i = (uint32_t)lane * 16u; i < len; i += 64u * 16u) {
    if (i + 16u <= len) { uint4 q; __builtin_memcpy(&q, src + i, 16); __builtin_memcpy(dst + i, &q, 16); }
    else for (uint32_t j = i; j < len; j++) dst[j] = src[j];
  }
}

// normalized range of every device-normalized document; segment / long-document counts
__global__ void k_norm_ranges(const uint64_t* __restrict__ piece_off, const uint64_t* __restrict__ doc_piece_start, const uint8_t* __restrict__ need_host,
                              uint32_t ndocs, uint64_t* __restrict__ nbegin, uint64_t* __restrict__ nend) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= ndocs) return;
  if (need_host[d]) return;                      // (k_place_fallback writes the range of a host-normalized document, possibly at the same time)
  nbegin[d] = piece_off[doc_piece_start[d]];
  nend[d] = piece_off[doc_piece_start[d + 1]];
}
// k_norm_ranges and k_norm_info in one launch, for a batch without host-normalized documents (a document that needs the host counts for
// nothing here: the caller runs k_norm_info again once those are placed)
__global__ void k_norm_ranges_info(const uint64_t* __restrict__ piece_off, const uint64_t* __restrict__ doc_piece_start, const uint8_t* __restrict__ need_host,
                                   uint32_t ndocs, uint64_t* __restrict__ nbegin, uint64_t* __restrict__ nend, unsigned long long* __restrict__ ninfo, uint32_t long_segs) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t nseg = 0;
  if (d < ndocs && !need_host[d]) {
    const uint64_t a = piece_off[doc_piece_start[d]], b = piece_off[doc_piece_start[d + 1]];
    nbegin[d] = a; nend[d] = b;
    nseg = (b - a + SEG - 1) / SEG;
    if (nseg > long_segs) atomicAdd(&ninfo[1], 1ull);
  }
  for (int o = 32; o > 0; o >>= 1) nseg += __shfl_xor(nseg, o);
  if ((threadIdx.x & 63) == 0 && nseg) atomicAdd(&ninfo[2], (unsigned long long)nseg);
}
__global__ void k_norm_info(const uint64_t* __restrict__ nbegin, const uint64_t* __restrict__ nend, uint32_t ndocs, unsigned long long* __restrict__ ninfo,
                            uint32_t long_segs) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t nseg = 0;
  if (d < ndocs) { nseg = (nend[d] - nbegin[d] + SEG - 1) / SEG; if (nseg > long_segs) atomicAdd(&ninfo[1], 1ull); }
  for (int o = 32; o > 0; o >>= 1) nseg += __shfl_xor(nseg, o);
  if ((threadIdx.x & 63) == 0 && nseg) atomicAdd(&ninfo[2], (unsigned long long)nseg);
}
// ---- the filter pass in front of the normalizer pass (round 6): the flags that drop and replace BYTES ------------------------------------------
// quotemarks 8, collapse 16, trim 32, leadingspace 64, unixlines 128 (training/README.md:110-123; tokenmonster.cpp:245-425, 428-462) and what
// accents 4 (:231-243) does to the two-byte characters, on the device: raw text in, filtered text + the documents' new ranges out, and the
// normalizer pass (NFD / lowercase / capcode) runs on that.  The host form is tm_normalize.cpp (squeeze, unix_lines, trim_and_lead,
// remove_marks), fuzzed against the reference runtime for all 256 flag values; this is the same function of the text, stated per byte:
//   * a space goes when the byte before it in the INPUT is a space; a '\r' goes when a '\n' follows; E2 80 {98,99 | 9C,9D} becomes ' or " -
//     all local - EXCEPT that the reference compacts in place and looks for the E2 80 in the buffer it is compacting: after exactly ONE
//     byte has been dropped (and until the next one is) the look-behind finds a byte that was already moved, and the quote stays.  The
//     offset by which the text has shrunk only grows - one for a dropped byte, two for a replaced quote - so it equals one exactly between the
//     first single drop of a document and the second, provided no quote was replaced before the first: three numbers per document
//     (first and second single drop, first quote candidate).
//     (unixlines WITHOUT collapse is a pass of its own in the reference, into a fresh buffer: no single drops in the loop that follows.)
//   * trim keeps what lies between the first and the last byte above 32, leadingspace puts a space in front of a first byte that is not
//     one; together, on a text WITHOUT leading blanks, the reference also cuts the last non-blank byte (:274-277) - kept.
//   * accents: a two-byte character becomes what NFD-and-drop-Mn leaves of it (nothing, one byte, two bytes: a table from the host's own
//     function, build_accent_table); whatever else would decompose or is a mark reaches the normalizer pass, whose tables in this mode
//     refuse it (norm_tables): that document is normalized by the host from its ORIGINAL bytes.
// Second form (the first - a piece per wavefront, a byte per lane, three launches that each read the text - took 9 ms per GiB): ONE launch, a
// wavefront per document, a dword per lane.  The wavefront first looks for the document's numbers - as a rule in its first and last 256
// bytes: the search for the single drops ends at the second one or at a quote in front of the first, the blanks at either end are short -,
// then sweeps the text once, 256 bytes per step: the tests are byte-parallel arithmetic on the lane's dword and on the same dword shifted
// against its neighbours' (DPP moves; the dword behind the step's last is the first of the next step's, which is already under way), a quote is
// found ONCE, at its first byte, and its other two bytes take their verdict from there, the lane packs the bytes it keeps and writes them
// with one store (two where it dropped something).  The filtered documents are not packed: document d begins on a 16-byte boundary of its
// own, PF_GAP bytes further from where it began for every document in front of it (the normalizer pass takes begin and end of a document
// from two arrays).  A document of more than PF_WHOLE bytes (rare) is filtered by a wavefront per span of PF_SPAN in three launches - numbers per span,
// sizes per span, bytes - of which the last two skip every other document.
constexpr uint32_t PF_NONE = 0xFFFFFFFFu;
#ifndef TM_PF_SPAN
#define TM_PF_SPAN 4096u        // (the emulated fuzz also runs with 1024 / 1024: documents of many spans)
#endif
#ifndef TM_PF_WHOLE
#define TM_PF_WHOLE 16384u
#endif
// a document of up to PF_WHOLE bytes is one wavefront's; a longer one is cut into spans of PF_SPAN (a span is a wavefront's work from end to end - 16 steps, three times)
constexpr uint32_t PF_SPAN = TM_PF_SPAN, PF_WHOLE = TM_PF_WHOLE, PF_GAP = 32u;
static_assert(PF_SPAN % 256u == 0u && PF_SPAN >= (uint32_t)PIECE && PF_WHOLE >= PF_SPAN, "a span is whole steps of the sweep, and the spans' table lives in the pieces' arrays");
__host__ __device__ __forceinline__ uint32_t pf_spans(uint64_t n) { return n <= PF_WHOLE ? (n ? 1u : 0u) : (uint32_t)((n + PF_SPAN - 1) / PF_SPAN); }
struct PfPiece { uint32_t s1, s2, fq, a, z; };      // of a span; positions in the document: first / second single drop, first quote candidate (its third byte), first / last byte above 32
struct PfDoc { uint32_t s1, s2, qb, a, z, zlo; };   // qb: a quote candidate lies before s1; zlo: where the last non-blank OUTPUT byte begins (z, or z - 2 for a replaced quote)
__host__ __device__ __forceinline__ uint64_t pf_out_begin(uint64_t raw_begin, uint32_t d) { return ((raw_begin + 15ull) & ~15ull) + (uint64_t)PF_GAP * d; }
__device__ __forceinline__ bool pf_isq(uint32_t y) { return y == 0x98u || y == 0x99u || y == 0x9Cu || y == 0x9Du; }
// four bytes at once: bit 7 of every byte of v that equals the byte c4 holds four times / that is one of 98 99 9C 9D / that is above 32
__device__ __forceinline__ uint32_t pf_eq(uint32_t v, uint32_t c4) { const uint32_t t = v ^ c4; return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u; }
__device__ __forceinline__ uint32_t pf_isq4(uint32_t v) { return pf_eq(v & 0xFAFAFAFAu, 0x98989898u); }
__device__ __forceinline__ uint32_t pf_nb4(uint32_t v) { return (((v & 0x7F7F7F7Fu) + 0x5F5F5F5Fu) | v) & 0x80808080u; }
// the dword at `off` of a document of n bytes behind `win` (a window of (n + 3) & ~3 bytes: the raw text has 256 bytes of room behind its last document): 0 for what lies behind the document
__device__ __forceinline__ uint32_t pf_load(const TmWindow& win, uint32_t off, uint32_t n) {
  uint32_t v = tm_window_u32(win, off);
  const uint32_t rem = n - off;
  if (rem < 4u) v &= (1u << (8u * rem)) - 1u;
  return v;
}
// position of the first (last) marked byte of the wavefront's 256: `any` = the ballot of m != 0
__device__ __forceinline__ uint32_t pf_first(unsigned long long any, uint32_t m, uint32_t base) {
  const int l = __builtin_ctzll(any);
  return base + 4u * (uint32_t)l + ((uint32_t)__builtin_ctz(read_lane(m, l)) >> 3);
}
__device__ __forceinline__ uint32_t pf_last(unsigned long long any, uint32_t m, uint32_t base) {
  const int l = 63 - __builtin_clzll(any);
  return base + 4u * (uint32_t)l + ((31u - (uint32_t)__builtin_clz(read_lane(m, l))) >> 3);
}
// is the quote whose third byte lies at t left alone (the in-place quirk above)?
__device__ __forceinline__ bool pf_suppressed(uint32_t flags, const PfDoc& d, uint32_t t) {
  return (flags & 16u) && d.s1 < t && t < d.s2 && d.qb == 0u;      // (d.s2 == PF_NONE: no second drop)
}
// the numbers of the span [rb, re) of a document.  `whole`: the span is the document, and the search for the drops may end at a quote
// candidate in front of the first of them as well (qb is then 1 whatever follows; spans are combined by positions and need the drops).
__device__ __forceinline__ PfPiece pf_scan_span(const TmWindow& win, uint32_t n, uint32_t rb, uint32_t re, uint32_t flags, bool whole, uint32_t lane) {
  PfPiece r{PF_NONE, PF_NONE, PF_NONE, PF_NONE, PF_NONE};
  const bool fused = (flags & 16u) && (flags & 128u), trim = flags & 32u;
  bool want_s = (flags & 8u) && (flags & 16u), want_a = trim;
  uint32_t carry = rb >= 4u ? pf_load(win, rb - 4u, n) : 0u;
#pragma unroll 1
  for (uint32_t base = rb; base < re && (want_s || want_a); base += 256u) {
    const uint32_t x = pf_load(win, base + 4u * lane, n);
    const uint32_t pd = TM_DPP(carry, x, 0x138, 0xF);           // wave_shr:1 - the dword of the lane below (lane 0: the last of the step before)
    carry = read_lane(x, 63);
    if (want_s) {
      const uint32_t p1 = (x << 8) | (pd >> 24), p2 = (x << 16) | (pd >> 16);      // the bytes one / two places in front of the lane's four
      uint32_t S = pf_eq(x, 0x20202020u) & pf_eq(p1, 0x20202020u);
      if (fused) S |= pf_eq(x, 0x0A0A0A0Au) & pf_eq(p1, 0x0D0D0D0Du);
      const uint32_t Q = pf_isq4(x) & pf_eq(p1, 0x80808080u) & pf_eq(p2, 0xE2E2E2E2u);
      unsigned long long mS = __ballot(S != 0u);
      while (mS != 0ull && r.s2 == PF_NONE) {
        const int l = __builtin_ctzll(mS);
        uint32_t m = read_lane(S, l);
        const uint32_t pos = base + 4u * (uint32_t)l + ((uint32_t)__builtin_ctz(m) >> 3);
        if (r.s1 == PF_NONE) r.s1 = pos; else r.s2 = pos;
        m &= m - 1u;
        if ((int)lane == l) S = m;
        if (m == 0u) mS &= mS - 1ull;
      }
      const unsigned long long mQ = __ballot(Q != 0u);
      if (mQ != 0ull && r.fq == PF_NONE) r.fq = pf_first(mQ, Q, base);
      if (r.s2 != PF_NONE || (whole && r.fq != PF_NONE && (r.s1 == PF_NONE || r.fq < r.s1))) want_s = false;
    }
    if (want_a) {
      const uint32_t N = pf_nb4(x);
      const unsigned long long mN = __ballot(N != 0u);
      if (mN != 0ull) { r.a = pf_first(mN, N, base); want_a = false; }
    }
  }
  if (trim && r.a != PF_NONE) {
#pragma unroll 1
    for (uint32_t base = rb + ((re - 1u - rb) & ~255u);; base -= 256u) {
      const uint32_t N = pf_nb4(pf_load(win, base + 4u * lane, n));
      const unsigned long long mN = __ballot(N != 0u);
      if (mN != 0ull) { r.z = pf_last(mN, N, base); break; }
      if (base == rb) break;
    }
  }
  return r;
}
// the document's numbers from those of its spans, in order (the numbers of one span: the document's own)
__device__ __forceinline__ void pf_add_span(PfDoc& r, uint32_t& fq, const PfPiece& p) {
  if (r.s1 == PF_NONE) { r.s1 = p.s1; r.s2 = p.s2; } else if (r.s2 == PF_NONE) r.s2 = p.s1;
  if (fq == PF_NONE) fq = p.fq;
  if (r.a == PF_NONE) r.a = p.a;
  if (p.z != PF_NONE) r.z = p.z;
}
__device__ __forceinline__ void pf_finish(PfDoc& r, uint32_t fq, const uint8_t* __restrict__ doc, uint32_t flags) {
  r.qb = fq < r.s1 ? 1u : 0u;
  r.zlo = r.z;
  // the last non-blank byte is the end of a quote that is replaced: the output byte begins two bytes earlier
  if (r.z != PF_NONE && (flags & 8u) && r.z >= 2u && pf_isq(doc[r.z]) && doc[r.z - 1u] == 0x80u && doc[r.z - 2u] == 0xE2u && !pf_suppressed(flags, r, r.z)) r.zlo = r.z - 2u;
}
// what the span [rb, re) of the document leaves: the number of bytes, and (EMIT) the bytes themselves at `out`
template <bool EMIT>
__device__ __forceinline__ uint32_t pf_emit_span(const uint8_t* __restrict__ doc, const TmWindow& win, uint32_t n, uint32_t rb, uint32_t re, uint32_t flags, const PfDoc& dd,
                                                 const uint32_t* __restrict__ acc, uint8_t* __restrict__ out, uint32_t lane) {
  const bool q = flags & 8u, c = flags & 16u, u = flags & 128u, trim = flags & 32u, lead = flags & 64u, accents = flags & 4u;
  // trim / leadingspace: [lo, hi) stays, and a space may go in front of it
  uint32_t lo = 0u, hi = n;
  bool pre = false;
  if (trim) {
    if (dd.a == PF_NONE) return 0u;                          // blank from end to end: nothing is left
    if (lead && dd.a == 0u) { if (dd.zlo == 0u) return 0u; hi = dd.zlo; pre = true; }      // (:274-277: the last non-blank byte goes as well)
    else { lo = dd.a; hi = dd.z + 1u; pre = lead; }
  } else if (lead) pre = doc[0] != ' ';                      // (n > 0: an empty document has no span)
  const uint32_t elo = max(lo, rb), ehi = min(hi, re);
  if (elo >= ehi) return 0u;
  uint32_t o = 0u;                                           // bytes of the span so far (wave-uniform)
  if (pre && lo >= rb) { if (EMIT && lane == 0u) out[0] = ' '; o = 1u; }
  const bool sup_on = q && c && dd.qb == 0u && dd.s1 != PF_NONE;
  // the sweep begins a dword in front of the first byte that stays: a quote that began there is found where it begins, and the first lane that
  // matters has its neighbour (nothing of what the sweep looks at lies further back than two bytes)
  uint32_t base = elo & ~3u;
  if (base >= 4u) base -= 4u;
  uint32_t xn = pf_load(win, base + 4u * lane, n), carry = 0u, carry_s = 0u;
#pragma unroll 1
  for (; base < ehi; base += 256u) {
    const uint32_t x = xn, off = base + 4u * lane;
    xn = pf_load(win, off + 256u, n);
    const uint32_t pd = TM_DPP(carry, x, 0x138, 0xF);                   // the dword of the lane below (lane 0: the last of the step before)
    const uint32_t nx = TM_DPP(read_lane(xn, 0), x, 0x130, 0xF);        // the dword of the lane above (lane 63: the first of the next step)
    carry = read_lane(x, 63);
    uint32_t D = 0u, y = x;                                              // bit 7 of a byte: it goes; the bytes as they leave
    if (c) D |= pf_eq(x, 0x20202020u) & pf_eq((x << 8) | (pd >> 24), 0x20202020u);
    if (u) D |= pf_eq(x, 0x0D0D0D0Du) & pf_eq((x >> 8) | (nx << 24), 0x0A0A0A0Au);
    if (q) {
      const uint32_t n1 = (x >> 8) | (nx << 24), n2 = (x >> 16) | (nx << 16);
      uint32_t S = pf_eq(x, 0xE2E2E2E2u) & pf_eq(n1, 0x80808080u) & pf_isq4(n2);      // a quote begins here
      if (sup_on && S != 0u) {
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) { const uint32_t t = off + j + 2u; if (dd.s1 < t && t < dd.s2) S &= ~(0x80u << (8u * j)); }
      }
      const uint32_t sp = TM_DPP(carry_s, S, 0x138, 0xF);
      carry_s = read_lane(S, 63);
      D |= ((S << 8) | (sp >> 24)) | ((S << 16) | (sp >> 16));           // its second and third byte go
      const uint32_t full = (S >> 7) * 0xFFu;
      y = (x & ~full) | ((0x27272727u ^ (((n2 >> 2) & 0x01010101u) * 5u)) & full);      // 98 99 -> ', 9C 9D -> "
    }
    if (accents && (x & 0x80808080u) != 0u) {
      const unsigned long long xx = (unsigned long long)x | ((unsigned long long)nx << 32);
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t b = (x >> (8u * j)) & 0xFFu, i = off + j;
        if (b < 0x80u) continue;
        const uint32_t bn = (uint32_t)(xx >> (8u * j + 8u)) & 0xFFu, bp = j ? (x >> (8u * j - 8u)) & 0xFFu : pd >> 24;
        // (both halves of the character must have stayed: the cut of trim + leadingspace may have taken the second)
        if (nm_two_lead(b) && i + 1u < hi && nm_cont_byte(bn)) {
          const uint32_t e = acc[nm_two_index(b, bn)];
          if ((e & 3u) == 1u) D |= 0x80u << (8u * j);
          else if ((e & 3u) >= 2u) y = (y & ~(0xFFu << (8u * j))) | (((e >> 8) & 0xFFu) << (8u * j));
        } else if (nm_cont_byte(b) && i >= lo + 1u && nm_two_lead(bp)) {
          const uint32_t e = acc[nm_two_index(bp, b)];
          if ((e & 3u) == 1u || (e & 3u) == 2u) D |= 0x80u << (8u * j);
          else if ((e & 3u) == 3u) y = (y & ~(0xFFu << (8u * j))) | (((e >> 16) & 0xFFu) << (8u * j));
        }
      }
    }
    if (base < elo || base + 256u > ehi) {                               // the first and the last step: what lies outside [elo, ehi) goes
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++) if (off + j < elo || off + j >= ehi) D |= 0x80u << (8u * j);
    }
    // the bytes that stay, packed: w, cnt of them
    uint32_t w = 0u, s = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
      const uint32_t gone = (D >> (8u * j + 7u)) & 1u;
      w |= (gone ? 0u : (y >> (8u * j)) & 0xFFu) << s;
      s += gone ? 0u : 8u;
    }
    const uint32_t cnt = s >> 3;
    const unsigned long long b0 = __ballot((cnt & 1u) != 0u), b1 = __ballot((cnt & 2u) != 0u), b2 = __ballot((cnt & 4u) != 0u);
    if (EMIT) {
      uint8_t* p = out + (o + mbcnt64(b0, 0u) + 2u * mbcnt64(b1, 0u) + 4u * mbcnt64(b2, 0u));
      if (cnt == 4u) __builtin_memcpy(p, &w, 4);
      else {
        if (cnt & 2u) { const uint16_t h = (uint16_t)w; __builtin_memcpy(p, &h, 2); p += 2; w >>= 16; }
        if (cnt & 1u) *p = (uint8_t)w;
      }
    }
    o += (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
  }
  return o;
}
// A wavefront per span (span_doc null: per document, every document one span or none).  A document that is one span is filtered here from end
// to end; of a longer one the span's numbers are left for the two kernels below.  rbegin / rend: the filtered document's range in `out`.
__global__ __launch_bounds__(256) void k_pf_filter(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off, const uint32_t* __restrict__ span_doc,
                                                   const uint64_t* __restrict__ doc_span_start, uint64_t nspans, uint32_t flags, const uint32_t* __restrict__ acc,
                                                   PfPiece* __restrict__ span_sum, uint8_t* __restrict__ out, uint64_t* __restrict__ rbegin, uint64_t* __restrict__ rend) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t k = (uint64_t)blockIdx.x * 4u + (uint64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (k >= nspans) return;
  const uint32_t d = span_doc ? span_doc[k] : (uint32_t)k;
  const uint64_t db = raw_off[d], ob = pf_out_begin(db, d);
  const uint32_t n = (uint32_t)(raw_off[d + 1] - db);
  if (n == 0u) { if (lane == 0u) { rbegin[d] = ob; rend[d] = ob; } return; }
  const bool whole = n <= PF_WHOLE;
  const uint32_t rb = span_doc ? (uint32_t)(k - doc_span_start[d]) * PF_SPAN : 0u, re = whole ? n : min(n, rb + PF_SPAN);
  const uint8_t* doc = raw + db;
  const TmWindow win = tm_window(doc, (n + 3u) & ~3u);
  const PfPiece p = pf_scan_span(win, n, rb, re, flags, whole, lane);
  if (!whole) { if (lane == 0u) span_sum[k] = p; return; }
  PfDoc dd{PF_NONE, PF_NONE, 0u, PF_NONE, PF_NONE, PF_NONE};
  uint32_t fq = PF_NONE;
  pf_add_span(dd, fq, p);
  pf_finish(dd, fq, doc, flags);
  const uint32_t len = pf_emit_span<true>(doc, win, n, rb, re, flags, dd, acc, out + ob, lane);
  if (lane == 0u) { rbegin[d] = ob; rend[d] = ob + len; }
}
// the spans of the documents of more than one: EMIT == false - the document's numbers (left in `docs` by its first span) and the bytes the span
// leaves (span_len); EMIT == true - the bytes themselves, behind those of the document's spans in front
template <bool EMIT>
__global__ __launch_bounds__(256) void k_pf_long(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off, const uint32_t* __restrict__ span_doc,
                                                 const uint64_t* __restrict__ doc_span_start, uint64_t nspans, uint32_t flags, const uint32_t* __restrict__ acc,
                                                 const PfPiece* __restrict__ span_sum, PfDoc* __restrict__ docs, uint32_t* __restrict__ span_len,
                                                 uint8_t* __restrict__ out, uint64_t* __restrict__ rbegin, uint64_t* __restrict__ rend) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t k = (uint64_t)blockIdx.x * 4u + (uint64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (k >= nspans) return;
  const uint32_t d = span_doc[k];
  const uint64_t db = raw_off[d], ob = pf_out_begin(db, d), k0 = doc_span_start[d];
  const uint32_t n = (uint32_t)(raw_off[d + 1] - db);
  if (n <= PF_WHOLE) return;
  const uint32_t rb = (uint32_t)(k - k0) * PF_SPAN, re = min(n, rb + PF_SPAN);
  const uint8_t* doc = raw + db;
  const TmWindow win = tm_window(doc, (n + 3u) & ~3u);
  if (!EMIT) {
    PfDoc dd{PF_NONE, PF_NONE, 0u, PF_NONE, PF_NONE, PF_NONE};
    uint32_t fq = PF_NONE;
    for (uint64_t j = k0; j < doc_span_start[d + 1]; j++) pf_add_span(dd, fq, span_sum[j]);
    pf_finish(dd, fq, doc, flags);
    const uint32_t len = pf_emit_span<false>(doc, win, n, rb, re, flags, dd, acc, nullptr, lane);
    if (lane == 0u) { span_len[k] = len; if (k == k0) docs[d] = dd; }
  } else {
    const PfDoc dd = docs[d];
    uint64_t at = 0;
    for (uint64_t j = k0; j < k; j++) at += span_len[j];
    const uint32_t len = pf_emit_span<true>(doc, win, n, rb, re, flags, dd, acc, out + ob + at, lane);
    if (lane == 0u && k + 1 == doc_span_start[d + 1]) { rbegin[d] = ob; rend[d] = ob + at + len; }
  }
}
// spans per document, for a batch with a document of more than one (an empty document has none: its range is written here)
__global__ void k_pf_begin(const uint64_t* __restrict__ raw_off, uint32_t ndocs, uint32_t* __restrict__ doc_nspan, uint64_t* __restrict__ rbegin, uint64_t* __restrict__ rend) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= ndocs) return;
  const uint64_t db = raw_off[d], n = raw_off[d + 1] - db;
  doc_nspan[d] = pf_spans(n);
  if (n == 0) { rbegin[d] = pf_out_begin(db, d); rend[d] = rbegin[d]; }
}

// One side of these two copies is pinned HOST memory, reached over PCIe: that side is accessed in aligned 16-byte units (a byte
// per lane made a 64-byte request per wavefront), the device side at whatever alignment is left.
template <bool DST_IS_HOST>
__device__ __forceinline__ void copy_doc(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t len) {
  const uintptr_t host_side = DST_IS_HOST ? (uintptr_t)dst : (uintptr_t)src;
  uint64_t head = (16u - (uint32_t)(host_side & 15u)) & 15u;
  if (head > len) head = len;
  for (uint64_t j = threadIdx.x; j < head; j += blockDim.x) dst[j] = src[j];
  const uint64_t nvec = (len - head) >> 4;
  for (uint64_t v = threadIdx.x; v < nvec; v += blockDim.x) {
    uint4 t;
    __builtin_memcpy(&t, src + head + 16 * v, 16);
    __builtin_memcpy(dst + head + 16 * v, &t, 16);
  }
  for (uint64_t j = head + 16 * nvec + threadIdx.x; j < len; j += blockDim.x) dst[j] = src[j];
}
__global__ void k_gather_docs(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ raw_off, const uint32_t* __restrict__ doc_ids,
                              const uint64_t* __restrict__ dst_off, uint32_t n, uint8_t* __restrict__ staging) {
  const uint32_t k = blockIdx.x;
  if (k >= n) return;
  const uint64_t s = raw_off[doc_ids[k]], len = raw_off[doc_ids[k] + 1] - s, o = dst_off[k];
  copy_doc<true>(staging + o, raw + s, len);
}
// place the host-normalized documents after the device-normalized text and record their ranges
__global__ void k_place_fallback(const uint8_t* __restrict__ staging, const uint64_t* __restrict__ src_off, const uint32_t* __restrict__ doc_ids,
                                 uint32_t n, uint64_t base, uint8_t* __restrict__ out, uint64_t* __restrict__ nbegin, uint64_t* __restrict__ nend) {
  const uint32_t k = blockIdx.x;
  if (k >= n) return;
  const uint64_t s = src_off[k], len = src_off[k + 1] - s;
  if (threadIdx.x == 0) { nbegin[doc_ids[k]] = base + s; nend[doc_ids[k]] = base + s + len; }
  copy_doc<false>(out + base + s, staging + s, len);
}

}  // namespace tmh

namespace {
// the normalizer's tables for {NFD, lowercase} x {capcode 2 or not}, built once per process from the host normalizer's functions (a few
// milliseconds of ICU calls: every lane's workspace uploads its own copy)
// flags: NFD 1, lowercase 2, accents 4.  `accents` (which implies NFD) strips the marks in the filter pass in front of the normalizer pass;
// what that pass does not handle - a two-byte character that would still decompose or is a non-spacing mark cannot reach this one, a
// three-byte mark can - has no entry here, so that its document goes to the host normalizer (with its original bytes).
const std::vector<uint8_t>& norm_tables(uint32_t flags, bool capcode2) {
  static std::mutex mu;
  static std::vector<uint8_t> cache[16];
  std::lock_guard<std::mutex> g(mu);
  const bool accents = (flags & 4u) != 0;
  if (accents) flags |= 1u;
  std::vector<uint8_t>& t = cache[(flags & 7u) | (capcode2 ? 8u : 0u)];
  if (t.empty()) {
    t.resize(NM_TABLE_BYTES);
    NmTwo* two = reinterpret_cast<NmTwo*>(t.data());
    uint32_t* blk = reinterpret_cast<uint32_t*>(two + NM_TWO_SIZE);
    build_two_table(flags & 3u, two);
    if (!capcode2) for (int k = 0; k < NM_TWO_SIZE; k++) if (two[k].a & (NT_DECOMP | NT_DECOMP2)) two[k].a = 0;      // (without capcode the pass keeps lengths: decomposing characters take the host path)
    build_three_tables(flags & 3u, blk, blk + NM_BLK_WORDS);
    build_four_table(flags & 3u, blk + NM_BLK_WORDS + NM_CP_WORDS);
    blk[NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS] = (capcode2 && (flags & 1u)) ? NM_MISC_HANGUL : 0u;      // NFD of the Hangul syllables: by arithmetic, where the pass may change lengths
    NmLea* lea = reinterpret_cast<NmLea*>(blk + NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS + 4);
    for (int k = 0; k < NM_LEA_SIZE; k++) lea[k] = NmLea{0, 0};
    if (capcode2 && (flags & 1u) && !accents) {      // ... and of Latin Extended Additional: a letter and one or two marks (under `accents` the marks would have to go: the host)
      build_lea_table(flags & 3u, lea);
      blk[NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS] |= NM_MISC_LEA;
    }
    uint16_t* kana = reinterpret_cast<uint16_t*>(lea + NM_LEA_SIZE);
    for (int k = 0; k < NM_KANA_SIZE; k++) kana[k] = 0;
    if (capcode2 && (flags & 1u) && !accents) {      // ... and of the voiced kana: a kana and its mark
      build_kana_table(kana);
      blk[NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS] |= NM_MISC_KANA;
    }
    uint8_t* ccc = reinterpret_cast<uint8_t*>(kana + NM_KANA_SIZE);
    for (uint32_t k = 0; k < NM_CCC_SIZE; k++) ccc[k] = 0;
    // ... the three-byte marks of canonical class > 0 (Indic, Thai ...): in place where they stand in order (under NFD without `accents`; without
    // NFD they are inert, build_three_tables), and the three-byte digits
    build_ccc_table(flags & 3u, (flags & 1u) && !accents, ccc);
    blk[NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS] |= NM_MISC_CCC;
    uint32_t* dec3 = reinterpret_cast<uint32_t*>(ccc + NM_CCC_SIZE);
    for (uint32_t k = 0; k < NM_DEC3_SIZE + NM_DEC3_THIRDS; k++) dec3[k] = 0;
    if (capcode2 && (flags & 1u) && !accents) {      // ... and the three-byte characters NFD splits in two (the two-part vowel signs of Bengali, Tamil ...; the nukta letters)
      build_dec3_table(dec3);
      blk[NM_BLK_WORDS + NM_CP_WORDS + NM_BLK4_WORDS] |= NM_MISC_DEC3;
    }
    if (accents) {
      std::vector<uint32_t> acc(NM_TWO_SIZE);
      build_accent_table(acc.data());
      for (int k = 0; k < NM_TWO_SIZE; k++) if ((acc[k] & 3u) != 0u || (two[k].a & (NT_DECOMP | NT_DECOMP2))) two[k].a = 0;      // (the filter pass has dealt with the first kind; a decomposition whose mark stays is rare enough for the host)
      uint32_t* cpt = blk + NM_BLK_WORDS;
      for (int w = 0; w < NM_CP_WORDS; w++) for (int j = 0; j < 16; j++) if (((cpt[w] >> (2 * j)) & 3u) == 3u) cpt[w] &= ~(3u << (2 * j));      // three-byte marks (a variation selector is Mn): the host
    }
  }
  return t;
}
}  // namespace

extern "C" {

int tm_batch_upload_raw(tm_batch* b, const uint8_t* raw, const uint64_t* raw_offsets, uint32_t ndocs) {
  int rc = tmh::batch_upload_raw_on(b, raw, raw_offsets, ndocs, nullptr);
  if (rc == TM_OK) { hipError_t e = hipStreamSynchronize(nullptr); if (e != hipSuccess) rc = hip_fail(e, "H2D raw text"); }
  return rc;
}

}  // extern "C"
namespace tmh {
int batch_upload_raw_on(tm_batch* b, const uint8_t* raw, const uint64_t* raw_offsets, uint32_t ndocs, hipStream_t st) {
  if (!b || (ndocs && !raw_offsets)) return set_error(TM_E_INVALID, "null argument");
  { int rc = enter_device(b->vocab); if (rc != TM_OK) return rc; }
  if (ndocs > b->max_docs) return set_error(TM_E_LIMIT, "batch has %u documents, workspace sized for %u", ndocs, b->max_docs);
  const uint64_t nbytes = ndocs ? raw_offsets[ndocs] : 0;
  if (ndocs && raw_offsets[0] != 0) return set_error(TM_E_INVALID, "offsets[0] must be 0");
  for (uint32_t d = 0; d < ndocs; d++)
    if (raw_offsets[d + 1] < raw_offsets[d]) return set_error(TM_E_INVALID, "offsets not monotone at document %u", d);
  { int rc = raw_prepare(b, nbytes, ndocs, raw_piece_count(b->vocab, raw_offsets, ndocs), st); if (rc != TM_OK) return rc; }
  hipError_t e;
  if (nbytes && (e = hipMemcpyAsync(b->d_raw, raw, nbytes, hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e, "H2D raw text");
  b->h_raw_off.assign(raw_offsets, raw_offsets + (ndocs ? ndocs + 1 : 0));      // (the batch's own copy: it outlives the caller's array)
  if (ndocs) { int rc = small_h2d(b, b->d_raw_off, b->h_raw_off.data(), ((uint64_t)ndocs + 1) * 8, st); if (rc != TM_OK) return rc; }
  return TM_OK;
}

// The normalizer's per-document and per-piece arrays, listed ONCE: raw_prepare frees and allocates them, raw_upload_replaces_buffers asks whether it
// would, piece_device_bytes counts them, raw_free frees them.  An array holds its kind's capacity + `extra` elements of `elem` bytes.
struct NormArray { void** p; uint32_t elem, extra; bool per_piece; };
static std::array<NormArray, 14> norm_arrays(tm_batch* b) {
  return {{{(void**)&b->d_raw_off, 8, 0, false}, {(void**)&b->d_doc_npiece, 4, 0, false}, {(void**)&b->d_doc_piece_start, 8, 1, false}, {(void**)&b->d_need_host, 1, 0, false},
           {(void**)&b->d_nbegin, 8, 0, false}, {(void**)&b->d_nend, 8, 0, false}, {(void**)&b->d_fb_ids, 4, 0, false}, {(void**)&b->d_fb_roff, 8, 1, false},
           {(void**)&b->d_fb_noff, 8, 1, false},
           {(void**)&b->d_piece_doc, 4, 0, true}, {(void**)&b->d_piece_sum, 4, 0, true}, {(void**)&b->d_piece_carry, 1, 0, true}, {(void**)&b->d_piece_len, 4, 0, true},
           {(void**)&b->d_piece_off, 8, 1, true}}};
}
// a kind's capacity as the batch keeps it (0: nothing allocated yet; raw_docs_cap is two less than the documents' arrays were allocated for), and
// whether its arrays take a batch of n documents / pieces as they are: two entries to spare
static uint64_t norm_cap(const tm_batch* b, bool per_piece) { return per_piece ? (b->d_piece_doc ? b->piece_cap : 0) : (b->d_raw_off ? b->raw_docs_cap : 0); }
static bool norm_holds(const tm_batch* b, bool per_piece, uint64_t n) { return n + 2 <= norm_cap(b, per_piece); }
static uint64_t slab_bytes(uint64_t npieces) { return (npieces + 1) * (uint64_t)SLAB; }
// the arrays of one kind freed and allocated again for n documents / pieces + 25 % + 16; after a failure none is left
static int norm_replace(tm_batch* b, bool per_piece, uint64_t n) {
  const auto arrays = norm_arrays(b);
  const uint64_t cap = n + n / 4 + 16;
  uint64_t each = 0;
  for (const NormArray& a : arrays) if (a.per_piece == per_piece) each += a.elem;
  if (norm_cap(b, per_piece)) trace_grow(per_piece ? "normalizer per-piece arrays" : "normalizer per-document arrays", n * each);
  hipError_t e = hipSuccess;
  for (const NormArray& a : arrays) if (a.per_piece == per_piece) { (void)hipFree(*a.p); *a.p = nullptr; }
  for (const NormArray& a : arrays) if (a.per_piece == per_piece && e == hipSuccess) e = hipMalloc(a.p, (cap + a.extra) * a.elem);
  if (e != hipSuccess) {
    for (const NormArray& a : arrays) if (a.per_piece == per_piece) { (void)hipFree(*a.p); *a.p = nullptr; }
    return hip_fail(e, per_piece ? "hipMalloc (pieces)" : "hipMalloc (raw documents)");
  }
  if (per_piece) b->piece_cap = cap;
  else b->raw_docs_cap = (uint32_t)std::min<uint64_t>(cap - 2, 0xFFFFFFFFull);
  return TM_OK;
}

// the 1 KiB pieces of a raw batch: of every document, and of the byte leadingspace may put in front of it in the filter pass
uint64_t raw_piece_count(const tm_vocab* v, const uint64_t* offsets, uint32_t ndocs) {
  const uint64_t grows = (v->host.norm_flag & 64u) ? 1u : 0u;
  uint64_t npieces = 0;
  for (uint32_t d = 0; d < ndocs; d++) npieces += (offsets[d + 1] - offsets[d] + grows + PIECE - 1) / PIECE;
  return npieces;
}

// the device buffers of a raw batch of this size (grow-only), the normalizer's tables on first use, and the batch's counts
int raw_prepare(tm_batch* b, uint64_t nbytes, uint32_t ndocs, uint64_t npieces, hipStream_t st) {
  // the normalized text cannot be shorter than what capcode leaves of the raw text, and the scans of tm_batch_normalize run over
  // one entry per piece with block sums sized (make_workspace) for max_bytes / 256 + max_docs entries
  if (ndocs > b->max_docs) return set_error(TM_E_LIMIT, "batch has %u documents, workspace sized for %u", ndocs, b->max_docs);
  if (nbytes > b->max_bytes) return set_error(TM_E_LIMIT, "raw batch has %llu bytes, workspace sized for %llu", (unsigned long long)nbytes, (unsigned long long)b->max_bytes);
  if (npieces > b->max_bytes / 256 + (uint64_t)b->max_docs) return set_error(TM_E_LIMIT, "raw batch has %llu pieces, workspace scans hold %llu", (unsigned long long)npieces, (unsigned long long)(b->max_bytes / 256 + b->max_docs));
  hipError_t e;
  int rc;
  if ((rc = grow_device(&b->d_raw, &b->raw_cap, nbytes + 256, nbytes + 256 + (nbytes + 256) / 4, "raw text")) != TM_OK) return rc;
  if (!norm_holds(b, false, ndocs) && (rc = norm_replace(b, false, ndocs)) != TM_OK) return rc;
  if (!b->d_ninfo && (e = hipMalloc((void**)&b->d_ninfo, 64)) != hipSuccess) return hip_fail(e, "hipMalloc");
  if (!b->d_two) {
    // what the vocabulary's flags {NFD, lowercase} do to the two-byte characters U+0080..U+017F, from the host normalizer's own building blocks
    if ((e = hipMalloc((void**)&b->d_two, NM_TABLE_BYTES)) != hipSuccess) return hip_fail(e, "hipMalloc");
    const std::vector<uint8_t>& tab = norm_tables(b->vocab->host.norm_flag & 7u, b->vocab->host.capcode == 2);
    if ((rc = small_h2d(b, b->d_two, tab.data(), NM_TABLE_BYTES, st)) != TM_OK) return rc;
  }
  if (!norm_holds(b, true, npieces) && (rc = norm_replace(b, true, npieces)) != TM_OK) return rc;
  if ((rc = grow_device(&b->d_slab, &b->slab_cap, slab_bytes(npieces), slab_bytes(npieces) + slab_bytes(npieces) / 4, "normalizer slabs")) != TM_OK) return rc;
  b->raw_bytes = nbytes;
  b->raw_docs = ndocs;
  b->raw_pieces = npieces;
  b->has_output = false;
  units_forget(b, 3u);
  return TM_OK;
}

// Would batch_upload_raw_on(these documents) replace a buffer that the batch in flight still reads?  After its normalizer pass that is the
// per-document ranges (always) and - when the text stays in the slabs for k_match_branch - the slabs and the pieces' offsets.  The
// host-to-host pipeline asks before it uploads a lane's next chunk beside the tokenizer kernels of the current one.
bool raw_upload_replaces_buffers(const tm_batch* b, const uint64_t* raw_offsets, uint32_t ndocs) {
  if (!b) return true;
  const uint64_t npieces = raw_piece_count(b->vocab, raw_offsets, ndocs);
  return !norm_holds(b, false, ndocs) || !norm_holds(b, true, npieces) || slab_bytes(npieces) > b->slab_cap;
}
// every device buffer raw_prepare and the filter pass have allocated (tm_batch_free)
void raw_free(tm_batch* b) {
  for (const NormArray& a : norm_arrays(b)) (void)hipFree(*a.p);
  void* rest[] = {b->d_raw, b->d_slab, b->d_ninfo, b->d_two, b->d_rawf, b->d_rawf_off, b->d_pf_piece, b->d_pf_doc, b->d_acc};
  for (void* p : rest) (void)hipFree(p);
}

// the slabs of the current batch packed into d_text (what tm_batch_normalize leaves out in the usual case); piece lengths and offsets are
// those of the last normalize call
void pack_text(tm_batch* b, hipStream_t st) {
  if (!b->text_in_slabs) return;
  b->text_in_slabs = false;
  const uint64_t np = b->slab_pieces;
  if (np > 0) TM_LAUNCH(k_norm_compact, (uint32_t)((np + 3) / 4), 256, 0, st, b->d_slab, b->d_piece_len, b->d_piece_off, np, b->d_text, b->max_bytes);
}
}  // namespace tmh
extern "C" {


// The grid of k_norm_emit2: its wavefronts take piece after piece, so that the tables are staged once per workgroup instead of once per four
// pieces - but NOT one workgroup per slot of the device (6 per compute unit: 25 KB of LDS each): the dispatcher does not spread those evenly, and
// a compute unit that got a seventh finishes late.  Measured per 512 MiB (MI355X, 256 compute units): one piece per wavefront 1.54 ms; 6 workgroups
// per compute unit 1.58; 12: 1.49; 24: 1.43; 48 - 96: 1.365; 256: 1.43.  (TM_NORM_WG_PER_CU: the sweep.)
static uint32_t norm_grid() {
  // (once per device and process: this runs per chunk and lane of the host-to-host pipeline)
  static std::mutex mu;
  static uint32_t cached[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
  std::lock_guard<std::mutex> g(mu);
  uint32_t& slot = cached[dev >= 0 && dev < 64 ? dev : 0];
  if (slot == 0) {
    const char* e = getenv("TM_NORM_WG_PER_CU");
    const int v = e ? atoi(e) : 0;
    const uint32_t wg_per_cu = v > 0 ? (uint32_t)v : 64u;
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) { (void)hipGetLastError(); cu = 256; }
    slot = (uint32_t)cu * wg_per_cu;
  }
  return slot;
}

// What a normalizer pass reads: the text and where its documents begin and end - the upload's, or what the filter pass makes of it - and its
// np pieces.  np_dev != null (a chunk of the ring behind a filter pass): np is a bound and *np_dev, on the device, the count.
struct NormSrc {
  const uint8_t* R; const uint64_t* RB; const uint64_t* RE; uint64_t np; const uint64_t* np_dev;
  uint32_t pgrid() const { return (uint32_t)((np + 3) / 4); }              // a wavefront per piece
  uint32_t egrid() const { return std::min(pgrid(), norm_grid()); }        // k_norm_emit2: its wavefronts take piece after piece
};

// the filter pass's buffers (grow-only) for a batch of raw_bytes in nd documents; long_spans: the 16 KiB spans of the batch when a document has
// more than one of them, else 0
static int prefilter_reserve(tm_batch* b, uint64_t raw_bytes, uint32_t nd, uint64_t long_spans) {
  const uint64_t out_cap = raw_bytes + (uint64_t)PF_GAP * nd + 256;
  int rc = grow_device(&b->d_rawf, &b->rawf_cap, out_cap, out_cap + out_cap / 4, "filtered text");
  if (rc != TM_OK) return rc;
  if (!b->d_rawf_off || b->rawf_docs_cap < (uint64_t)nd + 2) {
    (void)hipFree(b->d_rawf_off); (void)hipFree(b->d_pf_doc);
    b->d_rawf_off = nullptr; b->d_pf_doc = nullptr;
    b->rawf_docs_cap = (uint64_t)nd + nd / 4 + 16;
    hipError_t e;
    if ((e = hipMalloc((void**)&b->d_rawf_off, b->rawf_docs_cap * 16)) != hipSuccess || (e = hipMalloc((void**)&b->d_pf_doc, b->rawf_docs_cap * sizeof(PfDoc))) != hipSuccess)
      return hip_fail(e, "hipMalloc (filtered documents)");
  }
  const uint64_t span_bytes = (long_spans + 1) * sizeof(PfPiece);
  return long_spans ? grow_device(&b->d_pf_piece, &b->pf_piece_cap, span_bytes, span_bytes + span_bytes / 4, "filter pass spans") : TM_OK;
}

// The filter pass (k_pf_*, above) on the uploaded text, enqueued: s->R = the filtered text, s->RB / s->RE = where its documents begin and end (device); the
// table of its pieces (k_norm_begin + scan) is made here as well, their count is left in d_totals[3].
static int prefilter_enqueue(tm_batch* b, hipStream_t st, uint32_t norm_flag, const uint64_t* h_raw_off, NormSrc* s) {
  const uint32_t nd = b->raw_docs;
  hipError_t e;
  uint64_t nspans = 0;
  bool any_long = false;
  for (uint32_t d = 0; d < nd; d++) {
    const uint64_t len = h_raw_off[d + 1] - h_raw_off[d];
    if (len >= 0xFFFF0000ull) return set_error(TM_E_LIMIT, "document %u has %llu bytes: beyond what the filter pass addresses", d, (unsigned long long)len);
    nspans += pf_spans(len);
    any_long = any_long || len > PF_WHOLE;
  }
  { int rc = prefilter_reserve(b, b->raw_bytes, nd, any_long ? nspans : 0); if (rc != TM_OK) return rc; }
  if (any_long && nspans + 2 > b->piece_cap)
    return set_error(TM_E_INTERNAL, "the filter pass has %llu spans, the workspace holds %llu pieces", (unsigned long long)nspans, (unsigned long long)b->piece_cap);
  if ((norm_flag & 4u) && !b->d_acc) {
    std::vector<uint32_t> acc(NM_TWO_SIZE);
    build_accent_table(acc.data());
    if ((e = hipMalloc((void**)&b->d_acc, acc.size() * 4)) != hipSuccess) return hip_fail(e, "hipMalloc");
    int rc = small_h2d(b, b->d_acc, acc.data(), acc.size() * 4, st);
    if (rc != TM_OK) return rc;
  }
  uint64_t* rb = b->d_rawf_off;
  uint64_t* re = b->d_rawf_off + b->rawf_docs_cap;
  if (!any_long)
    TM_LAUNCH(k_pf_filter, (nd + 3) / 4, 256, 0, st, b->d_raw, b->d_raw_off, nullptr, nullptr, (uint64_t)nd, norm_flag, b->d_acc, nullptr, b->d_rawf, rb, re);
  else {
    // a document of more than one span: the spans' table (in the arrays the pieces' table takes afterwards), and three launches over it
    PfPiece* sums = (PfPiece*)b->d_pf_piece;
    PfDoc* docs = (PfDoc*)b->d_pf_doc;
    const uint32_t sgrid = (uint32_t)((nspans + 3) / 4);
    TM_LAUNCH(k_pf_begin, (nd + 255) / 256, 256, 0, st, b->d_raw_off, nd, b->d_doc_npiece, rb, re);
    scan_u32(b->d_doc_npiece, nd, b->d_scan_tmp, b->d_totals + 3, b->d_doc_piece_start, st);
    launch_unit_owner(b->d_doc_piece_start, nd, nspans, b->d_piece_doc, st);
    TM_LAUNCH(k_pf_filter, sgrid, 256, 0, st, b->d_raw, b->d_raw_off, b->d_piece_doc, b->d_doc_piece_start, nspans, norm_flag, b->d_acc, sums, b->d_rawf, rb, re);
    TM_LAUNCH(k_pf_long<false>, sgrid, 256, 0, st, b->d_raw, b->d_raw_off, b->d_piece_doc, b->d_doc_piece_start, nspans, norm_flag, b->d_acc, sums, docs, b->d_piece_len, nullptr, rb, re);
    TM_LAUNCH(k_pf_long<true>, sgrid, 256, 0, st, b->d_raw, b->d_raw_off, b->d_piece_doc, b->d_doc_piece_start, nspans, norm_flag, b->d_acc, sums, docs, b->d_piece_len, b->d_rawf, rb, re);
  }
  // the pieces of the filtered documents
  TM_LAUNCH(k_norm_begin, (std::max(nd, 8u) + 255) / 256, 256, 0, st, rb, re, nd, b->d_doc_npiece, b->d_need_host, (unsigned long long*)b->d_ninfo);
  scan_u32(b->d_doc_npiece, nd, b->d_scan_tmp, b->d_totals + 3, b->d_doc_piece_start, st);
  s->R = b->d_rawf; s->RB = rb; s->RE = re;
  return TM_OK;
}

// ---- tm_batch_normalize, stage by stage ----------------------------------------------------------------------------------------------------------
// How every normalizer call on an uploaded batch begins: the filter pass where the vocabulary has one (h_raw_off: the documents' offsets on the host),
// the batch's state reset, the piece table and the document of every piece.  Behind a filter pass the count of the pieces is fetched (a trip of its
// own: the pass is launched over it) - unless count_on_device: then s->np stays raw_prepare's bound and s->np_dev points at the count.
static int norm_begin(tm_batch* b, hipStream_t st, const uint64_t* h_raw_off, bool count_on_device, NormSrc* s) {
  const uint32_t capcode = b->vocab->host.capcode, norm_flag = b->vocab->host.norm_flag, nd = b->raw_docs;
  *s = NormSrc{b->d_raw, b->d_raw_off, b->d_raw_off + 1, b->raw_pieces, nullptr};
  const bool filtered = (norm_flag & ~3u) && nd > 0 && (capcode == 0 || capcode == 2);
  if (filtered) {
    int rc = prefilter_enqueue(b, st, norm_flag, h_raw_off, s);
    if (rc != TM_OK) return rc;
    if (count_on_device) s->np_dev = b->d_totals + 3;
    else {
      hipError_t e;
      uint64_t np = 0;
      if ((e = hipMemcpyAsync(&np, b->d_totals + 3, 8, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "D2H filtered piece count");
      if (np + 2 > b->piece_cap || slab_bytes(np) > b->slab_cap)
        return set_error(TM_E_INTERNAL, "the filter pass left %llu pieces, the workspace holds %llu", (unsigned long long)np, (unsigned long long)b->piece_cap);
      s->np = np;
    }
  }
  b->host_fallback_docs = 0;
  b->d_doc_begin = b->d_nbegin;
  b->d_doc_end = b->d_nend;
  b->ndocs = nd; b->nbytes = 0; b->nseg = 0; b->ngroups = 0; b->nlong = 0;
  b->text_in_slabs = false;
  units_forget(b, 1u);
  b->slab_pieces = s->np;
  if (nd == 0) return TM_OK;
  if (!filtered) {                             // (the filter pass has made the table of ITS documents' pieces)
    TM_LAUNCH(k_norm_begin, (std::max(nd, 8u) + 255) / 256, 256, 0, st, s->RB, s->RE, nd, b->d_doc_npiece, b->d_need_host, (unsigned long long*)b->d_ninfo);
    scan_u32(b->d_doc_npiece, nd, b->d_scan_tmp, b->d_totals + 3, b->d_doc_piece_start, st);
  }
  if (s->np > 0) launch_unit_owner(b->d_doc_piece_start, nd, s->np, b->d_piece_doc, st, s->np_dev);
  return TM_OK;
}

// The one-pass form, enqueued on `st` and NOT waited for: norm_begin, then ONE pass over the raw text - the emit kernel takes the carries of a piece
// from the 64 bytes either side of it and finds the documents that need the host normalizer as it goes -, the scan of the piece lengths, the
// documents' ranges and segment counts.  It leaves in d_ninfo: [0] documents for the host normalizer, [1] long documents, [2] segments, [3] pieces
// whose margins could not tell (a run of 64 digits / apostrophes / capitals across a piece boundary), [4] pieces that outgrew their slab, [5] the
// normalized size (the scan's total lands beside the info words: one copy brings everything), [6] short pieces inside a document.  NO compaction
// pass: the text stays in the slabs, k_match_branch stages its segments from there (packing was 0.8 ms per GiB); pack_text() where it is needed.
static int onepass_enqueue(tm_batch* b, hipStream_t st, const uint64_t* h_raw_off, bool count_on_device, NormSrc* s) {
  int rc = norm_begin(b, st, h_raw_off, count_on_device, s);
  if (rc != TM_OK || s->np == 0) return rc;
  const uint32_t capcode = b->vocab->host.capcode, lower_all = (b->vocab->host.norm_flag & 2u) ? 1u : 0u, nd = b->raw_docs;
  unsigned long long* ninfo = (unsigned long long*)b->d_ninfo;
  if (capcode == 2)
    TM_LAUNCH(k_norm_emit2<false>, s->egrid(), 256, 0, st, s->R, s->RB, s->RE, b->d_piece_doc, b->d_doc_piece_start, s->np, lower_all, nullptr,
                                               b->d_need_host, b->d_piece_len, b->d_slab, ninfo + 3, b->d_two, s->np_dev);
  else
    TM_LAUNCH(k_norm_emit<3>, s->pgrid(), 256, 0, st, s->R, s->RB, s->RE, b->d_piece_doc, b->d_doc_piece_start, s->np, capcode, lower_all,
                                          nullptr, b->d_need_host, b->d_piece_len, nullptr, b->d_slab, ninfo + 3, b->d_two, s->np_dev);
  TM_LAUNCH(k_norm_bad, (uint32_t)((std::max<uint64_t>(s->np, nd) + 255) / 256), 256, 0, st, b->d_piece_doc, b->d_need_host, b->d_doc_piece_start, s->np, nd, b->d_piece_len, ninfo, b->d_fb_ids, s->np_dev);
  scan_u32(b->d_piece_len, s->np, b->d_scan_tmp, reinterpret_cast<uint64_t*>(ninfo + 5), b->d_piece_off, st);
  TM_LAUNCH(k_norm_ranges_info, (nd + 255) / 256, 256, 0, st, b->d_piece_off, b->d_doc_piece_start, b->d_need_host, nd, b->d_nbegin, b->d_nend, ninfo, long_segs());
  return TM_OK;
}
// the exact path's first half: summaries of the pieces, then the carries per document (the origin pass has its document flags, info words and list written on the side)
static void launch_carries(tm_batch* b, hipStream_t st, const NormSrc& s, uint32_t nd, uint8_t* need_host, unsigned long long* ninfo, uint32_t* fb_ids) {
  const uint32_t lower_all = (b->vocab->host.norm_flag & 2u) ? 1u : 0u;
  if (s.np > 0) TM_LAUNCH(k_norm_summary, s.pgrid(), 256, 0, st, s.R, s.RB, s.RE, b->d_piece_doc, b->d_doc_piece_start, s.np, lower_all, b->d_two, b->d_piece_sum);
  TM_LAUNCH(k_norm_carry, (nd + 255) / 256, 256, 0, st, b->d_piece_sum, b->d_doc_piece_start, nd, b->d_piece_carry, need_host, ninfo, fb_ids, 0u);
}
// the documents' ranges to the host, on the caller's stream, and the group tree of the long ones (what the tokenize pipeline needs behind the normalizer)
static int groups_from_ranges(tm_batch* b, hipStream_t st) {
  const uint32_t nd = b->ndocs;
  std::vector<uint64_t> hb(nd), he(nd);
  hipError_t e;
  if ((e = hipMemcpyAsync(hb.data(), b->d_nbegin, (size_t)nd * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipMemcpyAsync(he.data(), b->d_nend, (size_t)nd * 8, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "D2H ranges");
  return build_groups(b, hb.data(), he.data(), nd, st);
}
// pooled workers for `docs` documents of `bytes` in all: up to 128, but only this process's share of the host when there is one process per GPU of
// the node - and only one per 2^shift bytes: the pool runs one job at a time, so a chunk of the host-to-host pipeline (a few dozen fallback
// documents) normalizes them on its own lane thread and leaves the pool to batches that need it
static uint32_t norm_workers(size_t docs, uint64_t bytes, uint32_t shift) {
  static const uint32_t host_share = std::max(8u, std::max(1u, std::thread::hardware_concurrency()) / (uint32_t)std::max(1, tm_device_count()));
  return (uint32_t)std::min<size_t>(std::min<size_t>(std::min<uint32_t>(128u, host_share), docs / 8 + 1), (size_t)(bytes >> shift) + 1);
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static bool norm_trace() { static const bool on = getenv("TM_TRACE") != nullptr; return on; }

// The documents the device leaves to the host normalizer (other non-ASCII content: NFD / Unicode case need ICU); none: every step is a no-op.
struct HostDocs {
  std::vector<uint32_t> ids;            // in document order
  std::vector<uint64_t> roff, noff;     // their offsets in the pinned staging of the raw and of the normalized bytes
  double t[4] = {0, 0, 0, 0};
  uint64_t bytes() const { return noff.empty() ? 0 : noff.back(); }
};
// ... fetched on a second stream, so that the fetch does not hold up the pass on the caller's, and normalized by the host's workers
static int host_docs_normalize(tm_batch* b, uint32_t nf, HostDocs* h) {
  if (nf == 0) return TM_OK;
  hipError_t e;
  h->t[0] = now_ms();
  if (!b->aux_stream && (e = hipStreamCreateWithFlags(&b->aux_stream, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e, "hipStreamCreate");
  hipStream_t sx = b->aux_stream;
  h->ids.resize(nf);
  int rc;
  if ((rc = small_d2h(b, h->ids.data(), b->d_fb_ids, (uint64_t)nf * 4, sx)) != TM_OK || (rc = small_sync(b, sx)) != TM_OK) return rc;
  std::sort(h->ids.begin(), h->ids.end());
  h->roff.assign(nf + 1, 0);
  for (size_t k = 0; k < nf; k++) h->roff[k + 1] = h->roff[k] + (b->h_raw_off[h->ids[k] + 1] - b->h_raw_off[h->ids[k]]);
  const uint64_t raw_bytes = h->roff.back();
  if ((rc = grow_pinned(&b->h_fb_raw, &b->h_fb_raw_cap, raw_bytes + 16, raw_bytes + raw_bytes / 4 + 4096, "fallback staging")) != TM_OK) return rc;
  if ((rc = small_h2d(b, b->d_fb_ids, h->ids.data(), (uint64_t)nf * 4, sx)) != TM_OK || (rc = small_h2d(b, b->d_fb_roff, h->roff.data(), h->roff.size() * 8, sx)) != TM_OK) return rc;
  // the gather writes straight into the pinned host buffer (no staging copy, nothing on the copy engines)
  TM_LAUNCH(k_gather_docs, nf, 256, 0, sx, b->d_raw, b->d_raw_off, b->d_fb_ids, b->d_fb_roff, nf, b->h_fb_raw);
  if ((e = hipStreamSynchronize(sx)) != hipSuccess) return hip_fail(e, "fallback documents to the host");
  h->t[1] = now_ms();
  h->noff.assign(nf + 1, 0);
  int grc = TM_OK;
  rc = normalize_batch_into(b->h_fb_raw, h->roff.data(), nf, b->vocab->host.capcode, b->vocab->host.norm_flag, norm_workers(nf, raw_bytes, 18), h->noff.data(), [&](uint64_t total) -> uint8_t* {
    grc = grow_pinned(&b->h_fb_norm, &b->h_fb_norm_cap, total + 16, total + total / 4 + 4096, "fallback output");      // pinned: the placement kernel reads it where it lies
    return b->h_fb_norm;
  });
  h->t[2] = now_ms();
  return grc != TM_OK ? grc : rc;
}
// ... placed behind the `base` bytes of the device part (reads over PCIe) on the second stream: different bytes of d_text, different documents' ranges
static int host_docs_place(tm_batch* b, const HostDocs& h, uint64_t base) {
  if (h.ids.empty()) return TM_OK;
  int rc = small_h2d(b, b->d_fb_noff, h.noff.data(), h.noff.size() * 8, b->aux_stream);
  if (rc != TM_OK) return rc;
  TM_LAUNCH(k_place_fallback, (uint32_t)h.ids.size(), 256, 0, b->aux_stream, b->h_fb_norm, b->d_fb_noff, b->d_fb_ids, (uint32_t)h.ids.size(), base, b->d_text, b->d_nbegin, b->d_nend);
  return TM_OK;
}
// ... and waited for: the text and ranges the placement wrote are read on the caller's stream next
static int host_docs_wait(tm_batch* b, HostDocs* h) {
  if (h->ids.empty()) return TM_OK;
  int rc = small_sync(b, b->aux_stream);
  if (rc != TM_OK) return rc;
  b->host_fallback_docs = (uint32_t)h->ids.size();
  h->t[3] = now_ms();
  if (norm_trace()) fprintf(stderr, "[fallback] flags+gather+D2H %.2f ms, host normalize (overlaps the device pass) %.2f ms, wait + H2D + place %.2f ms\n", h->t[1] - h->t[0], h->t[2] - h->t[1], h->t[3] - h->t[2]);
  return TM_OK;
}
static int limit_bytes(const tm_batch* b, uint64_t bytes) {
  return bytes <= b->max_bytes ? TM_OK : set_error(TM_E_LIMIT, "normalized text needs %llu bytes, workspace sized for %llu", (unsigned long long)bytes, (unsigned long long)b->max_bytes);
}
struct NormCall { hipStream_t st; bool one_piece; double t0, t1; };      // one_piece: below; t0, t1: the call's start and the end of its first trip (TM_TRACE)

// How every path but the usual one ends: the documents' ranges, then what the tokenize pipeline needs to know on the host - the segments, and the
// long documents if any.  recount: k_norm_ranges_info has counted the device's documents already, count them all again.
static int norm_close(tm_batch* b, const NormCall& c, uint64_t device_bytes, HostDocs* h, bool recount) {
  const uint32_t nd = b->ndocs;
  unsigned long long* ninfo = (unsigned long long*)b->d_ninfo;
  TM_LAUNCH(k_norm_ranges, (nd + 255) / 256, 256, 0, c.st, b->d_piece_off, b->d_doc_piece_start, b->d_need_host, nd, b->d_nbegin, b->d_nend);
  int rc = host_docs_wait(b, h);
  if (rc != TM_OK) return rc;
  const double t2 = now_ms();
  if (recount) (void)hipMemsetAsync(ninfo + 1, 0, 16, c.st);
  TM_LAUNCH(k_norm_info, (nd + 255) / 256, 256, 0, c.st, b->d_nbegin, b->d_nend, nd, ninfo, long_segs());
  unsigned long long h_info[3] = {0, 0, 0};
  if ((rc = small_d2h(b, h_info, ninfo, 24, c.st)) != TM_OK || (rc = small_sync(b, c.st)) != TM_OK) return rc;
  b->nbytes = device_bytes + h->bytes();
  b->nseg = h_info[2];
  if (h_info[1] > 0 && !c.one_piece) rc = groups_from_ranges(b, c.st);
  if (norm_trace()) fprintf(stderr, "[tm_batch_normalize] summaries %.2f ms, device pass + host fallback (%u docs) %.2f ms, info %.2f ms\n", c.t1 - c.t0, (unsigned)h->ids.size(), t2 - c.t1, now_ms() - t2);
  return rc;
}
// Outcome 1, the usual one: the one pass normalized every document.  The text stays in the slabs, but for a short piece inside a document (or the test hook).
static int onepass_done(tm_batch* b, const NormCall& c, const unsigned long long* h_info) {
  int rc = limit_bytes(b, h_info[5]);
  if (rc != TM_OK) return rc;
  b->nbytes = h_info[5];
  b->nseg = h_info[2];
  b->text_in_slabs = true;
  if (h_info[6] != 0 || (debug_flags() & 2048)) pack_text(b, c.st);
  if (h_info[1] > 0 && !c.one_piece) rc = groups_from_ranges(b, c.st);
  if (norm_trace()) fprintf(stderr, "[tm_batch_normalize] one trip: %.2f ms\n", now_ms() - c.t0);
  return rc;
}
// Outcome 2: the one pass is valid, and h_info[0] documents need the host normalizer - the device part is packed and they are placed behind it.
static int onepass_with_host_docs(tm_batch* b, const NormCall& c, unsigned long long* h_info) {
  const uint64_t device_bytes = h_info[5];
  b->text_in_slabs = true;
  pack_text(b, c.st);
  HostDocs h;
  int rc = host_docs_normalize(b, (uint32_t)h_info[0], &h);
  if (rc != TM_OK) return rc;
  if ((rc = small_d2h(b, h_info, b->d_ninfo, 56, c.st)) != TM_OK || (rc = small_sync(b, c.st)) != TM_OK) return rc;
  if ((rc = limit_bytes(b, device_bytes + h.bytes())) != TM_OK || (rc = host_docs_place(b, h, device_bytes)) != TM_OK) return rc;
  return norm_close(b, c, device_bytes, &h, true);
}

// Outcomes 3 to 5, the exact path - after a piece whose margins could not tell or one that outgrew its slab, or from the start (flags the one pass
// does not take, hook 8): summaries of the pieces, carries per document, then the device normalizes its documents with the carries given (one pass
// into per-piece slabs, lengths on the side; capcode 0 or hook 8: the per-lane version of the rules) while the host normalizes the others.  A piece
// that outgrows its slab even so (long runs of capitals) sends the device part through the two-pass emit, which writes the packed text.
static int exact_path(tm_batch* b, NormCall& c, const NormSrc& s) {
  hipStream_t st = c.st;
  const uint32_t capcode = b->vocab->host.capcode, lower_all = (b->vocab->host.norm_flag & 2u) ? 1u : 0u, nd = b->raw_docs;
  unsigned long long* ninfo = (unsigned long long*)b->d_ninfo;
  unsigned long long h_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  launch_carries(b, st, s, nd, b->d_need_host, ninfo, b->d_fb_ids);
  int rc;
  if ((rc = small_d2h(b, h_info, ninfo, 8, st)) != TM_OK || (rc = small_sync(b, st)) != TM_OK) return rc;
  c.t1 = now_ms();
  const uint32_t nf = (uint32_t)h_info[0];
  if (s.np > 0 && capcode == 2 && !(debug_flags() & 256))
    TM_LAUNCH(k_norm_emit2<true>, s.egrid(), 256, 0, st, s.R, s.RB, s.RE, b->d_piece_doc, b->d_doc_piece_start, s.np, lower_all, b->d_piece_carry,
                                              b->d_need_host, b->d_piece_len, b->d_slab, ninfo + 3, b->d_two, nullptr);
  else if (s.np > 0)
    TM_LAUNCH(k_norm_emit<2>, s.pgrid(), 256, 0, st, s.R, s.RB, s.RE, b->d_piece_doc, b->d_doc_piece_start, s.np, capcode, lower_all,
                                          b->d_piece_carry, b->d_need_host, b->d_piece_len, nullptr, b->d_slab, ninfo + 3, b->d_two, nullptr);
  scan_u32(b->d_piece_len, s.np, b->d_scan_tmp, b->d_totals + 2, b->d_piece_off, st);
  if (s.np > 0 && nf == 0) TM_LAUNCH(k_norm_short, (uint32_t)((s.np + 255) / 256), 256, 0, st, b->d_piece_doc, b->d_need_host, b->d_doc_piece_start, s.np, b->d_piece_len, ninfo);
  HostDocs h;
  if ((rc = host_docs_normalize(b, nf, &h)) != TM_OK) return rc;
  uint64_t device_bytes = 0;
  if ((rc = small_d2h(b, h_info, ninfo, 56, st)) != TM_OK || (rc = small_d2h(b, &device_bytes, b->d_totals + 2, 8, st)) != TM_OK || (rc = small_sync(b, st)) != TM_OK) return rc;
  if ((rc = limit_bytes(b, device_bytes + h.bytes())) != TM_OK || (rc = host_docs_place(b, h, device_bytes)) != TM_OK) return rc;
  if (s.np > 0 && h_info[3] == 0) {
    // no short piece inside a document and no host document: the text stays in the slabs here too (k_match_branch stages it from there);
    // otherwise it is packed - the host-normalized documents are placed behind the packed device part
    b->text_in_slabs = true;
    if (nf > 0 || h_info[6] != 0 || (debug_flags() & 2048)) pack_text(b, st);
  } else if (s.np > 0)
    TM_LAUNCH(k_norm_emit<1>, s.pgrid(), 256, 0, st, s.R, s.RB, s.RE, b->d_piece_doc, b->d_doc_piece_start, s.np, capcode, lower_all,
                                          b->d_piece_carry, b->d_need_host, b->d_piece_len, b->d_piece_off, b->d_text, nullptr, b->d_two, nullptr);
  return norm_close(b, c, device_bytes, &h, false);
}

// tm_batch_normalize: the one-pass form and ONE trip to the host - the whole device part is enqueued before anything comes back, and what comes
// back is everything at once.  (A chunk of the host-to-host pipeline used to wait for the device three times here; with four lanes' launches
// queueing on the runtime's lock every wait was also a gap in its stream.)  What the info words say decides the outcome.  one_piece: the batch is
// a raw piece of the streaming encoder (tm_encoder.hip), which wants the normalized text and no group tree (the workspace of such a batch has none)
static int batch_normalize_impl(tm_batch* b, void* stream, bool one_piece) {
  if (!b) return set_error(TM_E_INVALID, "null argument");
  const tm_vocab* v = b->vocab;
  { int rc = enter_device(v); if (rc != TM_OK) return rc; }
  const uint32_t capcode = v->host.capcode, norm_flag = v->host.norm_flag;
  if (!normalize_supported(capcode, norm_flag))
    return set_error(TM_E_INVALID, "normalization flags %u / capcode %u not supported by the normalizer", norm_flag, capcode);
  NormCall c{(hipStream_t)stream, one_piece, now_ms(), 0};
  NormSrc s;
  const bool one_pass = (capcode == 2 || capcode == 0) && normalize_on_device(capcode, norm_flag) && !(debug_flags() & 256);
  int rc = one_pass ? onepass_enqueue(b, c.st, b->h_raw_off.data(), false, &s) : norm_begin(b, c.st, b->h_raw_off.data(), false, &s);
  if (rc != TM_OK || b->raw_docs == 0) return rc;
  if (one_pass && s.np > 0) {
    unsigned long long h_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = small_d2h(b, h_info, b->d_ninfo, 56, c.st)) != TM_OK || (rc = small_sync(b, c.st)) != TM_OK) return rc;
    c.t1 = now_ms();
    if (h_info[3] == 0 && h_info[4] == 0) return h_info[0] == 0 ? onepass_done(b, c, h_info) : onepass_with_host_docs(b, c, h_info);
    (void)hipMemsetAsync(b->d_ninfo, 0, 64, c.st);        // a piece whose margins could not tell, or one that outgrew its slab: the exact path, from the start
  }
  return exact_path(b, c, s);
}

int tm_batch_normalize(tm_batch* b, void* stream) { return batch_normalize_impl(b, stream, false); }

}  // extern "C"
namespace tmh {
// ---- the origin pass (tm_batch_raw_spans, tm_spans.hip) ---------------------------------------------------------------------------------------
// For every byte of the batch's normalized text, where the documents' ranges (d_nbegin) put it, the offset in its RAW document of the first byte
// of the unit that owns it (tm_build.h: tm_normalize_origins) - a u32 per normalized byte in the batch's grow-only d_own.  The documents the
// device normalized, of a vocabulary without a filter pass, get theirs from k_norm_emit<4> over the resident raw text, with the carries of
// k_norm_summary + k_norm_carry (made again here: the one-pass normalizer never makes them) - the carry kernel's document flags and list go to
// a scratch buffer, nothing the normalizer left is written.  Every other document - the host-normalized ones; all of them under a byte-level
// flag or `accents` - is fetched back from d_raw, mapped by normalize_origins on the pooled workers and its owners uploaded.
int origin_ready(const tm_batch* b, const char* who) {
  if (!b->d_nbegin || b->d_doc_begin != b->d_nbegin || b->raw_docs != b->ndocs || !b->d_raw)
    return set_error(TM_E_INVALID, "%s: the batch's text did not come from tm_batch_upload_raw + tm_batch_normalize (there is no raw text to point into)", who);
  for (uint32_t d = 0; d < b->ndocs; d++)
    if (b->h_raw_off[d + 1] - b->h_raw_off[d] >= (1ull << 32))
      return set_error(TM_E_LIMIT, "%s: document %u has %llu raw bytes (offsets are 32 bits)", who, d, (unsigned long long)(b->h_raw_off[d + 1] - b->h_raw_off[d]));
  return TM_OK;
}

int origin_pass_on(tm_batch* b, hipStream_t st, uint32_t* host_docs) {
  if (host_docs) *host_docs = 0;
  const uint32_t nd = b->ndocs;
  if (nd == 0 || b->nbytes == 0) return TM_OK;
  const uint32_t capcode = b->vocab->host.capcode, norm_flag = b->vocab->host.norm_flag;
  int rc = grow_batch(b, (void**)&b->d_own, &b->own_cap, b->nbytes, b->nbytes + b->nbytes / 4 + 1024, 4, "origins");
  if (rc != TM_OK) return rc;
  // scratch of the carry kernel: need_host[nd] | ninfo[8] | fb_ids[nd]
  const uint64_t o_info = ((uint64_t)nd + 7) & ~7ull, o_ids = o_info + 64, tmp_bytes = o_ids + (uint64_t)nd * 4;
  if ((rc = grow_batch(b, (void**)&b->d_own_tmp, &b->own_tmp_cap, tmp_bytes, tmp_bytes + tmp_bytes / 4 + 256, 1, "origins scratch")) != TM_OK) return rc;
  hipError_t e;
  (void)hipGetLastError();
  const bool on_device = (norm_flag & ~3u) == 0u && (capcode == 0 || capcode == 2);
  const uint64_t np = b->slab_pieces;
  std::vector<uint8_t> need(nd, 1);
  if (on_device) {
    const uint32_t lower_all = (norm_flag & 2u) ? 1u : 0u;
    const NormSrc s{b->d_raw, b->d_raw_off, b->d_raw_off + 1, np, nullptr};
    if (np > 0 && capcode == 2) {
      (void)hipMemsetAsync(b->d_own_tmp + o_info, 0, 64, st);
      launch_carries(b, st, s, nd, b->d_own_tmp, (unsigned long long*)(b->d_own_tmp + o_info), reinterpret_cast<uint32_t*>(b->d_own_tmp + o_ids));
    }
    if (np > 0)
      TM_LAUNCH(k_norm_emit<4>, s.pgrid(), 256, 0, st, s.R, s.RB, s.RE, b->d_piece_doc, b->d_doc_piece_start, np, capcode, lower_all, b->d_piece_carry,
                b->d_need_host, b->d_piece_len, b->d_piece_off, reinterpret_cast<uint8_t*>(b->d_own), nullptr, b->d_two, nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "kernel launch");
    if (b->host_fallback_docs == 0) return TM_OK;
    if ((e = hipMemcpyAsync(need.data(), b->d_need_host, nd, hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "D2H document flags");
  }
  // the host's documents: ranges, raw bytes (neighbouring documents in one copy), owners
  std::vector<uint64_t> nb(nd), ne(nd);
  if ((e = hipMemcpyAsync(nb.data(), b->d_nbegin, (size_t)nd * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipMemcpyAsync(ne.data(), b->d_nend, (size_t)nd * 8, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "D2H ranges");
  std::vector<uint32_t> ids;
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t d = 0; d < nd; d++) if (need[d]) { ids.push_back(d); lo = std::min(lo, nb[d]); hi = std::max(hi, ne[d]); }
  if (host_docs) *host_docs = (uint32_t)ids.size();
  if (ids.empty() || hi <= lo) return TM_OK;
  if (hi > b->nbytes) return set_error(TM_E_INTERNAL, "origin pass: a document's range ends at %llu of %llu normalized bytes", (unsigned long long)hi, (unsigned long long)b->nbytes);
  const std::vector<uint64_t>& ro = b->h_raw_off;
  std::vector<uint8_t> rawh;
  std::vector<uint64_t> at(ids.size());
  {
    uint64_t total = 0;
    for (size_t k = 0; k < ids.size(); k++) { at[k] = total; total += ro[ids[k] + 1] - ro[ids[k]]; }
    rawh.resize(total + 1);
    for (size_t k = 0; k < ids.size();) {
      size_t j = k + 1;
      while (j < ids.size() && ids[j] == ids[j - 1] + 1) j++;
      const uint64_t s = ro[ids[k]], n = ro[ids[j - 1] + 1] - s;
      if (n && (e = hipMemcpyAsync(rawh.data() + at[k], b->d_raw + s, n, hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "D2H raw documents");
      k = j;
    }
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "D2H raw documents");
  }
  std::vector<uint32_t> stage(hi - lo, 0u);
  std::atomic<uint32_t> next{0};
  std::atomic<int> bad{0};
  run_on_workers(norm_workers(ids.size(), rawh.size(), 16), [&]() {
    std::vector<uint8_t> text;
    std::vector<uint32_t> own;
    for (;;) {
      const uint32_t k = next.fetch_add(1);
      if (k >= ids.size()) break;
      const uint32_t d = ids[k];
      if (!normalize_origins(rawh.data() + at[k], (size_t)(ro[d + 1] - ro[d]), capcode, norm_flag, text, own) || own.size() != ne[d] - nb[d]) { bad = 1; continue; }
      if (!own.empty()) std::memcpy(stage.data() + (nb[d] - lo), own.data(), own.size() * 4);
    }
  });
  if (bad) return set_error(TM_E_INTERNAL, "origin pass: the host's owners do not fit the batch's normalized text");
  if ((e = hipMemcpyAsync(b->d_own + lo, stage.data(), stage.size() * 4, hipMemcpyHostToDevice, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "H2D owners");
  return TM_OK;
}
// The host-to-host ring takes a vocabulary whose normalizer pass is the one-pass form (capcode 0 or 2 with flags the device implements)
bool ring_supported(const tm_vocab* v) {
  const uint32_t capcode = v->host.capcode, norm_flag = v->host.norm_flag;
  // (a vocabulary with byte-level flags: the filter pass in front is enqueued like everything else, and the normalizer pass behind it is launched
  // over the pieces of the RAW documents - a bound: a filtered document is no longer than the raw one, but for the space leadingspace may put in
  // front, which raw_prepare has counted - and takes the count from the device)
  return normalize_supported(capcode, norm_flag) && (capcode == 2 || capcode == 0) && !(debug_flags() & (256 | 2048));
}
// tm_batch_normalize's usual path (onepass_enqueue) on the chunk raw_prepare + the upload have put into the workspace, enqueued on `st`
// and NOT waited for: what the host would read back stays in d_ninfo, k_chunk_ctl turns it into the control words the kernels behind it
// look at (the segments are launched over `seg_bound`), and a chunk the pass cannot finish by itself (documents for the host normalizer, a
// piece whose margins could not tell, a long document ...) is marked there and run through tm_batch_normalize by the caller afterwards.
int ring_enqueue_normalize(tm_batch* b, hipStream_t st, uint64_t seg_bound, const uint64_t* h_raw_off) {
  if (b->raw_docs == 0 || b->raw_pieces == 0) return set_error(TM_E_INTERNAL, "ring_enqueue_normalize: empty chunk");
  hipError_t e;
  if (!b->d_ctl_store && (e = hipMalloc((void**)&b->d_ctl_store, 64)) != hipSuccess) return hip_fail(e, "hipMalloc");
  (void)hipGetLastError();
  NormSrc s;
  int rc = onepass_enqueue(b, st, h_raw_off, true, &s);
  if (rc != TM_OK) return rc;
  b->d_ctl = b->d_ctl_store;
  b->nseg = std::min<uint64_t>(seg_bound, b->max_segs);
  b->text_in_slabs = true;
  launch_chunk_ctl(b, b->nseg, st);
  e = hipGetLastError();
  return e == hipSuccess ? TM_OK : hip_fail(e, "kernel launch");
}

// ---- the streaming encoder's raw pieces (tm_encoder.hip) ----------------------------------------------------------------------------------------
// A raw piece is ONE document of the encoder's normalizer workspace.  piece_reserve grows every buffer the normalizer (and the filter pass in
// front of it) takes for a piece of max_raw bytes, once, so that no later piece allocates; piece_device_bytes is what those buffers hold.
int piece_reserve(tm_batch* b, uint64_t max_raw, hipStream_t st) {
  int rc = raw_prepare(b, max_raw, 1, (max_raw + PIECE - 1) / PIECE, st);
  if (rc != TM_OK || !(b->vocab->host.norm_flag & ~3u)) return rc;
  return prefilter_reserve(b, max_raw, 1, max_raw > PF_WHOLE ? pf_spans(max_raw) : 0);
}
uint64_t piece_device_bytes(tm_batch* b) {
  uint64_t n = b->raw_cap + 64 + NM_TABLE_BYTES + b->slab_cap;      // the raw text, the info words, the tables, the slabs
  for (const NormArray& a : norm_arrays(b)) n += (norm_cap(b, a.per_piece) + (a.per_piece ? 0 : 2) + a.extra) * a.elem;
  if (b->d_rawf) n += b->rawf_cap + b->rawf_docs_cap * (16 + sizeof(PfDoc)) + b->pf_piece_cap;
  if (b->vocab->host.norm_flag & 4u) n += (uint64_t)NM_TWO_SIZE * 4;      // (the accent table: made by the first piece's filter pass)
  return n;
}
int piece_normalize_on(tm_batch* b, hipStream_t st) { return batch_normalize_impl(b, st, true); }

// The normalized bytes [from, from + n) of the piece go to dst: from the slabs (a wavefront per slab, which takes what of its piece lies in the
// range) or, where the normalizer has packed the text, from there (a wavefront per 2 KiB of the range).  Neither end is aligned - dst lies
// behind the look-ahead the encoder carries, a portion begins in mid-piece -, so a run is staged in LDS: 16-byte loads from the aligned chunks
// that hold it, 16-byte stores to the aligned chunks of dst, each made of two aligned LDS reads shifted against each other; the up to 15
// bytes in front of and behind dst's aligned part go byte by byte.
constexpr int EP_STAGE = SLAB / 16 + 5;
__global__ __launch_bounds__(256) void k_enc_pack(const uint8_t* __restrict__ slab, const uint32_t* __restrict__ piece_len, const uint64_t* __restrict__ piece_off,
                                                  const uint8_t* __restrict__ text, uint64_t nruns, uint64_t from, uint64_t n, uint8_t* __restrict__ dst) {
  __shared__ uint4 stage[4][EP_STAGE];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t k = (uint64_t)blockIdx.x * 4 + w;
  const uint8_t* src = nullptr;
  uint8_t* out = nullptr;
  uint32_t len = 0;
  if (k < nruns) {
    if (slab) {
      const uint64_t off = piece_off[k], a = off > from ? off : from, z = off + piece_len[k] < from + n ? off + piece_len[k] : from + n;
      if (a < z) { src = slab + k * (uint64_t)SLAB + (a - off); out = dst + (a - from); len = (uint32_t)(z - a); }
    } else {
      const uint64_t a = k * (uint64_t)SLAB;
      if (a < n) { src = text + from + a; out = dst + a; len = (uint32_t)(n - a < (uint64_t)SLAB ? n - a : (uint64_t)SLAB); }
    }
  }
  const uint32_t sa = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
  const uint32_t nch = len ? (sa + len + 15u) / 16u : 0u;                    // <= (15 + SLAB + 15) / 16 < EP_STAGE - 2
  const uint4* s16 = reinterpret_cast<const uint4*>(src - sa);
  for (uint32_t c = lane; c < nch; c += 64u) stage[w][c] = s16[c];
  __syncthreads();
  const uint8_t* img = reinterpret_cast<const uint8_t*>(stage[w]) + sa;      // the run as it lies in LDS
  uint32_t da = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u;
  if (da > len) da = len;
  if (lane < da) out[lane] = img[lane];
  const uint32_t body = (len - da) / 16u;
  const uint32_t m = (sa + da) & 15u, base = (sa + da) / 16u, mw = m >> 2, sh = (m & 3u) * 8u;
  for (uint32_t c = lane; c < body; c += 64u) {
    const uint4 A = stage[w][base + c], B = stage[w][base + c + 1];
    // the five dwords that hold the sixteen bytes from byte m of A on
    const uint32_t d0 = mw == 0 ? A.x : mw == 1 ? A.y : mw == 2 ? A.z : A.w, d1 = mw == 0 ? A.y : mw == 1 ? A.z : mw == 2 ? A.w : B.x,
                   d2 = mw == 0 ? A.z : mw == 1 ? A.w : mw == 2 ? B.x : B.y, d3 = mw == 0 ? A.w : mw == 1 ? B.x : mw == 2 ? B.y : B.z,
                   d4 = mw == 0 ? B.x : mw == 1 ? B.y : mw == 2 ? B.z : B.w;
    uint4 q;
    q.x = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh); q.y = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
    q.z = (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh); q.w = (uint32_t)((((uint64_t)d4 << 32) | d3) >> sh);
    *reinterpret_cast<uint4*>(out + da + 16u * c) = q;
  }
  const uint32_t t0 = da + body * 16u;
  if (t0 + lane < len) out[t0 + lane] = img[t0 + lane];                      // (fewer than 16 bytes)
}
// b: the encoder's normalizer workspace behind piece_normalize_on; [from, from + n) lies inside its normalized text
void launch_enc_pack(const tm_batch* b, uint64_t from, uint64_t n, uint8_t* dst, hipStream_t st) {
  if (!n) return;
  if (b->text_in_slabs) TM_LAUNCH(k_enc_pack, (uint32_t)((b->slab_pieces + 3) / 4), 256, 0, st, b->d_slab, b->d_piece_len, b->d_piece_off, nullptr, b->slab_pieces, from, n, dst);
  else {
    const uint64_t runs = (n + SLAB - 1) / SLAB;
    TM_LAUNCH(k_enc_pack, (uint32_t)((runs + 3) / 4), 256, 0, st, nullptr, nullptr, nullptr, b->d_text, runs, from, n, dst);
  }
}
}  // namespace tmh
extern "C" {

uint64_t tm_batch_normalized_bytes(const tm_batch* b) { return b->nbytes; }
uint32_t tm_batch_host_fallback_docs(const tm_batch* b) { return b->host_fallback_docs; }

// D2H of the normalized text of the current batch in DOCUMENT ORDER (for tests): text_out[nbytes], offsets_out[ndocs+1]
int tm_batch_download_text(tm_batch* b, uint8_t* text_out, uint64_t text_cap, uint64_t* offsets_out) {
  if (!b) return set_error(TM_E_INVALID, "null argument");
  hipError_t e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "sync");
  pack_text(b, nullptr);
  if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "sync");
  if (b->nbytes > text_cap) return set_error(TM_E_NOSPACE, "text_cap too small");
  const uint32_t nd = b->ndocs;
  std::vector<uint64_t> hb(nd), he(nd);
  std::vector<uint8_t> all(b->nbytes);
  if (nd && ((e = hipMemcpy(hb.data(), b->d_doc_begin, (size_t)nd * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
             (e = hipMemcpy(he.data(), b->d_doc_end, (size_t)nd * 8, hipMemcpyDeviceToHost)) != hipSuccess)) return hip_fail(e, "D2H ranges");
  if (b->nbytes && (e = hipMemcpy(all.data(), b->d_text, b->nbytes, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "D2H text");
  uint64_t o = 0;
  for (uint32_t d = 0; d < nd; d++) {
    if (offsets_out) offsets_out[d] = o;
    if (he[d] > hb[d]) std::memcpy(text_out + o, all.data() + hb[d], he[d] - hb[d]);
    o += he[d] - hb[d];
  }
  if (offsets_out) offsets_out[nd] = o;
  return TM_OK;
}

}  // extern "C"

// tm_cuts.h — where ONE document may be cut into pieces: shared by the streaming encoder (tm_encoder.hip) and tm_tokenize_document
// (tm_document.hip).  Plain host C++ with no dependency on the device runtime, so that a stand-alone program can check it by itself.
//
// Normalized text: a piece that is followed by more text owns its bytes and may look at HALO more; the walk enters it in one of 80 entry
// states whose offsets, < 40, must lie inside the piece, so every piece that follows another is at least MIN_RANGE bytes long.
// Raw text: behind a line feed - and behind any byte of the fallback set - the normalizer is in the state it starts a text in
// (tests/test_safe_cuts.py keeps that claim checked against the host normalizer), so normalize(a + b) == normalize(a) + normalize(b) there.
#pragma once
#include <cstdint>

namespace tmh {

constexpr uint64_t CUT_HALO = 128, CUT_MIN_RANGE = 64;

// bytes behind which the normalizer is in its start state: '\n' wherever there is one, these once a line outgrows a piece
inline bool fallback_cut(uint8_t c) {
  switch (c) {
    case '\n': case '\t': case '.': case ',': case ';': case ':': case '!': case '?': case '(': case ')': case '[': case ']': case '{': case '}':
    case '<': case '>': case '=': case '/': case '-': case '"': return true;
    default: return false;
  }
}

// the bytes of p[0, n) up to and including the last line feed / the last byte of the fallback set; 0: there is none
inline uint64_t cut_behind_line_feed(const uint8_t* p, uint64_t n) {
  for (uint64_t i = n; i > 0; i--) if (p[i - 1] == '\n') return i;
  return 0;
}
inline uint64_t cut_behind_fallback(const uint8_t* p, uint64_t n) {
  for (uint64_t i = n; i > 0; i--) if (fallback_cut(p[i - 1])) return i;
  return 0;
}

// A whole raw text of n bytes in hand, pieces of at most `piece` bytes: the length of the piece that begins at p.  What is left goes as the
// last piece when it fits; otherwise the cut lies behind the last line feed of the first `piece` bytes, else behind their last fallback
// byte.  0: those bytes hold neither (the text cannot be cut here).
inline uint64_t raw_piece_length(const uint8_t* p, uint64_t left, uint64_t piece) {
  if (left <= piece) return left;
  const uint64_t lf = cut_behind_line_feed(p, piece);
  return lf ? lf : cut_behind_fallback(p, piece);
}

// the normalized size a raw piece of max_piece bytes may have on the device: three times (a Hangul syllable under NFD) and some
inline uint64_t piece_norm_cap(uint64_t max_piece) { return 3 * max_piece + 4096; }

// Normalized text of n bytes in pieces of `piece` bytes (>= CUT_MIN_RANGE): piece k owns [k * piece, (k + 1) * piece), the last one everything
// that is left - a tail shorter than CUT_MIN_RANGE is folded into the piece before it - and a piece may look at CUT_HALO bytes behind what it
// owns (fewer where the text ends there).
struct PieceRange { uint64_t begin, own_end, vis_end; };
inline uint64_t norm_piece_count(uint64_t n, uint64_t piece) {
  if (n == 0) return 0;
  uint64_t k = (n + piece - 1) / piece;
  if (k > 1 && n - (k - 1) * piece < CUT_MIN_RANGE) k--;
  return k;
}
inline PieceRange norm_piece(uint64_t n, uint64_t piece, uint64_t count, uint64_t k) {
  PieceRange r;
  r.begin = k * piece;
  r.own_end = k + 1 == count ? n : (k + 1) * piece;
  r.vis_end = n - r.own_end < CUT_HALO ? n : r.own_end + CUT_HALO;
  return r;
}

}  // namespace tmh

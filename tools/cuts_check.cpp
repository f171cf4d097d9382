// cuts_check.cpp — stand-alone check of tm_cuts.h (the piece layout of normalized text and the cut search of raw text that the streaming
// encoder and tm_tokenize_document share), meant to be built with -fsanitize=address,undefined and run by itself: tests/test_document_cuts.py.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tm_cuts.h"
using namespace tmh;
int main() {
  // layout arithmetic: pieces tile [0, n), every non-first piece >= MIN_RANGE, vis within n and within HALO
  for (uint64_t piece : {64ull, 65ull, 127ull, 128ull, 256ull, 1000ull}) for (uint64_t n = 0; n < 5000; n++) {
    const uint64_t c = norm_piece_count(n, piece);
    uint64_t at = 0;
    for (uint64_t k = 0; k < c; k++) {
      PieceRange r = norm_piece(n, piece, c, k);
      assert(r.begin == at && r.own_end > r.begin && r.vis_end >= r.own_end && r.vis_end <= n && r.vis_end - r.own_end <= CUT_HALO);
      assert(r.vis_end - r.begin <= piece + CUT_HALO);
      if (c > 1) assert(r.own_end - r.begin >= CUT_MIN_RANGE);
      if (k + 1 < c) assert(r.vis_end == (n - r.own_end < CUT_HALO ? n : r.own_end + CUT_HALO));
      at = r.own_end;
    }
    assert(at == n);
  }
  // cut search on random text
  srand(7);
  for (int t = 0; t < 2000; t++) {
    const uint64_t n = rand() % 3000, piece = 64 + rand() % 500;
    std::vector<uint8_t> v(n);
    for (auto& b : v) { int r = rand() % 100; b = r < 2 ? '\n' : r < 5 ? '.' : 'a' + r % 26; }
    for (uint64_t pos = 0; pos < n;) {
      const uint64_t take = raw_piece_length(v.data() + pos, n - pos, piece);
      if (!take) break;
      assert(take <= piece && pos + take <= n);
      if (pos + take < n) assert(fallback_cut(v[pos + take - 1]));
      pos += take;
    }
  }
  puts("cuts ok");
  return 0;
}

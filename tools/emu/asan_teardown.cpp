// tools/emu/asan_teardown.cpp — what the boundary sweeps (tests/test_gpu_normalize_boundaries.py, tests/test_gpu_decode_boundaries.py) do to the
// library, and then every teardown, under AddressSanitizer and UndefinedBehaviorSanitizer with the kernels on the emulated device (tools/emu).
// Development aid, a stand-alone program without Python:
//   bash tools/emu/asan_teardown.sh           everything is freed in order: batches, then vocabularies
//   bash tools/emu/asan_teardown.sh leave     nothing is freed: workspaces, lanes and vocabularies are left to the exit of the process
// Per vocabulary (capcode 2 + NFD, capcode 0 + NFD, the filter pass in front) and hook (0, 256, 2048): a batch of a thousand documents with
// constructs across the piece seams, a third of them the host normalizer's - normalized, tokenized and decoded resident -, the same text through
// the host-buffer calls (a lane of the vocabulary's pool), and one workspace of one document reused for a hundred and fifty batches.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "tm_build.h"
#include "tokenmonster_hip.h"
#define CHECK(x) do { int rc_ = (x); if (rc_ != TM_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #x, rc_, tm_last_error()); std::exit(1); } } while (0)
int main(int argc, char** argv) {
  const bool leave = argc > 1;      // leave everything to exit
  std::vector<uint8_t> blob(256); std::vector<uint32_t> boff(257);
  for (int c = 0; c < 256; c++) { blob[c] = (uint8_t)c; boff[c] = c; } boff[256] = 256;
  const char* con[] = {"Hello", "\xd0\x96", "\xc3\x89T\xc3\x89", "\xe1\xba\xbe", "\xea\xb0\x92", "\xe1\xba\x9e", "\xff", "\xf0\x9f\x98\x80", "e\xcc\xa3\xcc\x81", "\xc4\xb0"};
  const char* fill[] = {"x", "Q", "xQ 7'", "the Quick 7th fox's IT ", " "};
  std::vector<std::string> docs;
  for (int rep = 0; rep < 3; rep++) for (auto c : con) for (auto f : fill) for (int start : {60, 63, 955, 959, 1020, 1023, 2046}) {
    std::string d; while ((int)d.size() < start) d += f; d.resize(start); d += c; for (int k = 0; k < 70; k++) d += "3"; d += "Q z";
    docs.push_back(d);
  }
  std::vector<uint8_t> raw; std::vector<uint64_t> roff{0};
  for (auto& d : docs) { raw.insert(raw.end(), d.begin(), d.end()); roff.push_back(raw.size()); }
  const uint32_t nd = (uint32_t)docs.size();
  std::fprintf(stderr, "%u documents, %zu bytes\n", nd, raw.size());
  std::vector<tm_vocab*> vs;
  for (auto cf : std::vector<std::pair<int,int>>{{2, 1}, {0, 1}, {2, 186}}) {
    tm_vocab* v = nullptr;
    CHECK(tm_vocab_build(blob.data(), boff.data(), 256, nullptr, cf.first, 1, cf.second, 5, 0, 0, &v));
    vs.push_back(v);
    for (int hook : {0, 256, 2048}) {
      tm_debug_flags(hook);
      tm_batch* b = nullptr;
      CHECK(tm_batch_create(v, raw.size() * 4 + 16 * nd + 1024, nd, &b));
      CHECK(tm_batch_upload_raw(b, raw.data(), roff.data(), nd));
      CHECK(tm_batch_normalize(b, nullptr));
      const uint64_t n = tm_batch_normalized_bytes(b);
      std::vector<uint8_t> text(n + 1); std::vector<uint64_t> noff(nd + 1);
      CHECK(tm_batch_download_text(b, text.data(), n, noff.data()));
      CHECK(tm_batch_run(b, nullptr));
      uint64_t nt = 0; CHECK(tm_batch_totals(b, &nt, nullptr));
      if (cf.first == 2) {
        uint64_t nb = 0; uint32_t hd = 0; CHECK(tm_batch_decode(b, 0, nullptr, &nb, &hd));
        std::vector<uint8_t> out(n + 64); std::vector<uint64_t> ooff(nd + 1);
        CHECK(tm_batch_decoded_download(b, out.data(), out.size(), ooff.data()));
      }
      std::vector<uint32_t> ids(n + 64); std::vector<uint64_t> toff(nd + 1); std::vector<uint32_t> miss(nd + 1);
      CHECK(tm_tokenize_batch(v, text.data(), noff.data(), nd, ids.data(), ids.size(), toff.data(), miss.data()));
      std::vector<uint8_t> dec(8 * toff[nd] + 64); std::vector<uint64_t> doff(nd + 1);
      CHECK(tm_decode_batch(v, ids.data(), toff.data(), nd, 0, dec.data(), dec.size(), doff.data()));
      std::fprintf(stderr, "vocab (%d, %d) hook %d: %llu normalized bytes, %u host docs, %llu ids\n", cf.first, cf.second, hook, (unsigned long long)n, tm_batch_host_fallback_docs(b), (unsigned long long)nt);
      if (!leave) tm_batch_free(b);
      // one workspace, many batches of one document
      tm_batch* one = nullptr;
      CHECK(tm_batch_create(v, 4 * 4096 + 4096, 1, &one));
      for (uint32_t d = 0; d < nd; d += 7) {
        uint64_t o[2] = {0, roff[d + 1] - roff[d]};
        CHECK(tm_batch_upload_raw(one, raw.data() + roff[d], o, 1));
        CHECK(tm_batch_normalize(one, nullptr));
        const uint64_t m = tm_batch_normalized_bytes(one);
        std::vector<uint8_t> t(m + 1); uint64_t no[2];
        CHECK(tm_batch_download_text(one, t.data(), m, no));
      }
      if (!leave) tm_batch_free(one);
    }
    tm_debug_flags(0);
  }
  if (!leave) for (tm_vocab* v : vs) tm_vocab_free(v);
  std::fprintf(stderr, "done\n");
  return 0;
}

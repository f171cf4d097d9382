// chunks_check.cpp — stand-alone check of tm_chunks.h (how tm_tokenize_pipeline cuts a batch into chunks), meant to be built with
// -fsanitize=address,undefined and run by itself: tests/test_pipeline_chunks.py.  Synthetic offset arrays only, no text.
//   chunks_check <tables>    every layout checked against its limits and against the recorded layout of the same name in <tables>
//   chunks_check --print     the layouts as <tables> holds them (tests/golden/pipeline_chunks.txt was printed from the loop as it stood in
//                            tokenize_pipeline_on, moved into the header word for word, before anything else about it changed)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>
#include "tm_chunks.h"
using namespace tmh;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "chunks_check: %s: ", name.c_str()); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", #cond); exit(1); } } while (0)

static const uint64_t KiB = 1024, MiB = 1024 * 1024;
typedef std::vector<uint64_t> Offsets;

static uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }
static Offsets from_lengths(const std::vector<uint64_t>& len) { Offsets o(1, 0); for (uint64_t n : len) o.push_back(o.back() + n); return o; }

// The limit in force for chunk `ci` with `left` bytes from its first byte to the end of the batch, as the comment of tm_chunks.h states it.
static uint64_t stated_limit(size_t ci, uint64_t left, uint32_t nv, uint32_t lanes, uint64_t chunk_bytes, bool ring, uint64_t ramp_first, uint64_t ramp_pct) {
  uint64_t ramp = chunk_bytes, tail = chunk_bytes;
  if (ring) {
    ramp = ramp_first;
    for (size_t i = 0; i < ci && ramp < chunk_bytes; i++) ramp = ramp / 100 * ramp_pct;               // c bytes, then c / 100 x ramp_pct
    const uint64_t floor = chunk_bytes < 4 * MiB ? chunk_bytes : 4 * MiB;
    if (left < 2ull * nv * chunk_bytes) { tail = left / (2ull * nv); if (tail < floor) tail = floor; }   // the tail halves per device
  } else {
    const uint64_t w = (uint64_t)lanes * nv;
    if (ci < w) {                                                                                        // chunk_bytes / 2^W ... chunk_bytes / 2
      ramp = w - ci >= 64 ? 0 : chunk_bytes >> (w - ci);
      const uint64_t floor = chunk_bytes < MiB ? chunk_bytes : MiB;
      if (ramp < floor) ramp = floor;
    }
    const uint64_t floor = chunk_bytes < 2 * MiB ? chunk_bytes : 2 * MiB;
    if (left < w * chunk_bytes) { tail = left / w; if (tail < floor) tail = floor; }                    // 1 / W of what is left
  }
  uint64_t limit = chunk_bytes;
  if (ramp < limit) limit = ramp;
  if (tail < limit) limit = tail;
  return limit;
}

static bool print_mode = false;
static std::map<std::string, std::string> recorded;
static size_t ncases = 0;

static void run(const std::string& name, const Offsets& off, uint32_t nv, uint32_t lanes, uint64_t chunk_bytes, bool ring, uint64_t ramp_first, uint64_t ramp_pct) {
  const uint32_t ndocs = (uint32_t)off.size() - 1;
  std::vector<uint32_t> first;
  chunk_layout(off.data(), ndocs, nv, lanes, chunk_bytes, ring, ramp_first, ramp_pct, first);
  CHECK(!first.empty() && first[0] == 0 && first.back() == ndocs, "ends");
  for (size_t k = 0; k + 1 < first.size(); k++) {
    CHECK(first[k] < first[k + 1], "chunk %zu is empty or runs backwards", k);
    const uint64_t bytes = off[first[k + 1]] - off[first[k]];
    const uint64_t limit = stated_limit(k, off[ndocs] - off[first[k]], nv, lanes, chunk_bytes, ring, ramp_first, ramp_pct);
    CHECK(first[k + 1] - first[k] == 1 || bytes <= limit, "chunk %zu of %u documents has %llu bytes, limit %llu", k, first[k + 1] - first[k], (unsigned long long)bytes, (unsigned long long)limit);
    // ... and it is a maximal run: the document behind it would not have fitted
    CHECK(first[k + 1] == ndocs || off[first[k + 1] + 1] - off[first[k]] > limit, "chunk %zu stops short of its limit %llu", k, (unsigned long long)limit);
  }
  std::string line;
  for (uint32_t d : first) { if (!line.empty()) line += ' '; line += std::to_string(d); }
  ncases++;
  if (print_mode) { printf("%s|%s\n", name.c_str(), line.c_str()); return; }
  const auto it = recorded.find(name);
  CHECK(it != recorded.end(), "no recorded layout");
  CHECK(it->second == line, "layout differs from the recorded one:\n  have %s\n  want %s\n", line.c_str(), it->second.c_str());
  recorded.erase(it);
}

static std::string size_name(uint64_t b) { return b % MiB == 0 ? std::to_string(b / MiB) + "M" : std::to_string(b / KiB) + "K"; }

// both forms of one batch: the lanes' form for every (nv, lanes), the ring's for every nv and every (ramp_first, ramp_pct)
static void both_forms(const std::string& batch, const Offsets& off, const std::vector<uint64_t>& chunk_sizes, bool all_ramps) {
  static const uint32_t shapes[][2] = {{1, 1}, {1, 4}, {2, 2}, {3, 8}, {8, 8}, {2, 1}, {3, 1}};      // nv, lanes: lanes x nv = 1, 4, 4, 24, 64, 2, 3
  static const uint64_t first_kib[] = {2048, 64, 1 << 20}, pcts[] = {150, 110, 400};                  // the defaults, then the ends of the ranges
  for (uint64_t cb : chunk_sizes) {
    for (const auto& s : shapes) run(batch + "/lanes/nv" + std::to_string(s[0]) + "/l" + std::to_string(s[1]) + "/c" + size_name(cb), off, s[0], s[1], cb, false, 2048 * KiB, 150);
    for (uint32_t nv = 1; nv <= 3; nv++)
      for (uint64_t fk : first_kib) for (uint64_t pct : pcts) {
        if (!all_ramps && (fk != 2048) + (pct != 150) > 1) continue;
        run(batch + "/ring/nv" + std::to_string(nv) + "/c" + size_name(cb) + "/f" + std::to_string(fk) + "K/r" + std::to_string(pct), off, nv, 4, cb, true, fk * KiB, pct);
      }
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: chunks_check <tables> | --print\n"); return 2; }
  print_mode = !strcmp(argv[1], "--print");
  if (!print_mode) {
    std::ifstream in(argv[1]);
    std::string l;
    while (std::getline(in, l)) { const size_t bar = l.find('|'); if (bar != std::string::npos) recorded[l.substr(0, bar)] = l.substr(bar + 1); }
    if (recorded.empty()) { fprintf(stderr, "chunks_check: no tables in %s\n", argv[1]); return 2; }
  }
  const std::vector<uint64_t> small_chunks = {8 * MiB, 32 * MiB, 512 * KiB};
  both_forms("none", Offsets(1, 0), {32 * MiB}, false);                                               // ndocs == 0
  both_forms("one", from_lengths({100}), {32 * MiB}, false);
  both_forms("one-empty", from_lengths({0}), {32 * MiB}, false);
  both_forms("one-large", from_lengths({100 * MiB}), small_chunks, false);
  // runs of empty documents: in front of a document that does not fit they are a zero-byte chunk, which the ring hands to the exact path with no slot
  both_forms("empties", from_lengths({0, 0, 0, 40 * MiB, 0, 0, 300 * KiB, 0, 64 * MiB, 0, 0, 0, 0, 9 * MiB, 0}), small_chunks, true);
  { std::vector<uint64_t> len(1000, 0); both_forms("all-empty", from_lengths(len), {8 * MiB}, false); }
  // one document larger than chunk_bytes among small ones
  { std::vector<uint64_t> len; uint64_t s = 3; for (int i = 0; i < 400; i++) len.push_back(i == 170 ? 50 * MiB : 100 * KiB + lcg(s) % (400 * KiB)); both_forms("large-among-small", from_lengths(len), small_chunks, true); }
  // documents that end exactly on the limit: every ramp step, floor and full chunk is a multiple of these
  { std::vector<uint64_t> len(600, 256 * KiB); both_forms("exact-256K", from_lengths(len), small_chunks, true); }
  { std::vector<uint64_t> len(2400, 64 * KiB); both_forms("exact-64K", from_lengths(len), small_chunks, true); }
  { std::vector<uint64_t> len(40, 8 * MiB); both_forms("exact-8M", from_lengths(len), small_chunks, false); }
  // ... and one byte to either side of it
  { std::vector<uint64_t> len; for (int i = 0; i < 600; i++) len.push_back(256 * KiB + (i % 3) - 1); both_forms("around-256K", from_lengths(len), small_chunks, false); }
  // the benchmark's shape: about 300 000 documents of at most 64 KiB, 1 GiB in all
  {
    std::vector<uint64_t> len; uint64_t s = 0x5EED, total = 0;
    while (total < 1024 * MiB) {
      const uint64_t r = lcg(s), n = std::min<uint64_t>(1024 * MiB - total, r % 100 < 95 ? lcg(s) % 4096 : lcg(s) % (64 * KiB + 1));
      len.push_back(n); total += n;
    }
    const std::string name = "bench";
    CHECK(len.size() > 250000 && len.size() < 350000, "%zu documents", len.size());
    both_forms("bench", from_lengths(len), {32 * MiB, 48 * MiB}, true);
  }
  if (!print_mode && !recorded.empty()) { fprintf(stderr, "chunks_check: %zu recorded layouts were not computed, the first: %s\n", recorded.size(), recorded.begin()->first.c_str()); return 1; }
  if (!print_mode) printf("chunks ok: %zu layouts\n", ncases);
  return 0;
}

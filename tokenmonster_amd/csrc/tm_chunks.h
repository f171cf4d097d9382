// tm_chunks.h — how tm_tokenize_pipeline cuts a batch into chunks (tm_host.hip, tokenize_pipeline_on).  Plain host C++ with no dependency on the
// device runtime and no look at the environment, so that a stand-alone program can check it by itself (tools/chunks_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace tmh {

// chunks = maximal runs of whole documents of at most `limit` bytes (a longer document is a chunk of its own); `first` gets the first document
// of every chunk and, behind them, ndocs.  offsets[ndocs + 1] is monotone, nv the devices, lanes the lanes of each, `ring` the form.
//
// The steady state of the pipeline runs near the device-resident rate; what it loses it loses at the two ends.
// Lanes' form: W = lanes x nv workers that all begin with full chunks upload W chunks at once and then run their kernels in lock step, so the
// first W chunks grow geometrically - chunk_bytes / 2^W ... chunk_bytes / 2, none below 1 MiB - and the last ones shrink by 1 / W of what is
// left each, none below 2 MiB.
// Ring: a chunk's kernels cannot begin before its upload has ended, and the link is only a fifth faster than the kernels (56 against 46 GB/s):
// behind a chunk of c bytes the next may have c / 100 x ramp_pct (ramp_first 2 MiB and ramp_pct 150 by default: 2, 3, 4.5 ... MiB) or the device
// waits for it; the tail halves per device - 1 / (2 nv) of what is left, none below 4 MiB (... 32, 16, 8, 4 MiB: what the end costs is the
// last chunk's kernels and download with nothing beside them).  No floor is above chunk_bytes.
inline void chunk_layout(const uint64_t* offsets, uint32_t ndocs, uint32_t nv, uint32_t lanes, uint64_t chunk_bytes, bool ring, uint64_t ramp_first,
                         uint64_t ramp_pct, std::vector<uint32_t>& first) {
  const size_t nramp = (size_t)lanes * nv;                          // the lanes' form: workers, if there are chunks enough
  uint64_t ring_limit = ramp_first;
  for (uint32_t d = 0; d < ndocs;) {
    first.push_back(d);
    const size_t ci = first.size() - 1;                              // this chunk's number
    const uint64_t left = offsets[ndocs] - offsets[d];
    uint64_t limit = chunk_bytes;
    if (ring) {
      limit = std::min(chunk_bytes, ring_limit);
      ring_limit = std::min<uint64_t>(chunk_bytes, ring_limit / 100 * ramp_pct);
      if (left < 2 * (uint64_t)nv * chunk_bytes) limit = std::min(limit, std::max<uint64_t>(left / (2 * (uint64_t)nv), std::min<uint64_t>(chunk_bytes, 4u << 20)));
    } else {
      // (the shift count is clamped: 8 lanes on 8 devices - or on the virtual devices of a test - make nramp 64 and more)
      if (ci < nramp) limit = std::max<uint64_t>(chunk_bytes >> std::min<size_t>(nramp - ci, 63), std::min<uint64_t>(chunk_bytes, 1u << 20));
      // (the drain's shape - a floor of 2 / 4 / 8 / 16 MiB, a third or half of what is left instead of a quarter - was swept in round 5: every
      // setting 30 - 37 ms per call, the same as this one: profiles/r05_h2h.txt)
      if (left < (uint64_t)nramp * chunk_bytes) limit = std::min(limit, std::max<uint64_t>(left / nramp, std::min<uint64_t>(chunk_bytes, 2u << 20)));
    }
    // the last document that still ends within `limit` bytes of the chunk's first byte (at least one document)
    const uint64_t* const lo = offsets + d + 1;
    const uint64_t* const hi = std::upper_bound(lo, offsets + ndocs + 1, offsets[d] + limit);
    d = std::max<uint32_t>(d + 1, (uint32_t)(hi - offsets) - 1);
  }
  first.push_back(ndocs);
}

}  // namespace tmh

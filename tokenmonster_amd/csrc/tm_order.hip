// tm_order.hip — tm_batch_length_order: the documents of a run in a stable order of their id counts, ascending or descending, as ABSOLUTE
// document numbers (what tm_batch_collate_select takes as its doc_index).  The rule: include/tokenmonster_hip.h.
//
// A least-significant-digit radix sort of (key, document) pairs with 8-bit digits, written for wavefronts of 64 and LDS.  The key is the id
// count n_d = tok_offsets[d + 1] - tok_offsets[d], under TM_ORDER_DESCENDING its complement - so that equal counts keep ascending document
// numbers in both directions: every pass is stable, and the pairs start in document order.
//   1. k_order_keys: a tile of ORD_TILE documents per workgroup - key and document number of each into plane 0, the largest count of the tile.
//   2. k_order_max: one workgroup folds the tiles' maxima into ONE word.  Every kernel behind it reads that word: pass k has work only if the
//      largest count has a bit at or above 8 k - a byte above it is the same in every key (0, or 0xFF in the complement) and would move nothing.
//      The passes with work are a prefix 0 .. p - 1, so pass k always reads plane k & 1 and writes the other: nothing has to remember which
//      plane is current, only the last kernel asks (p & 1).  The host launches no pass that the run's id TOTAL already rules out.
//   3. per pass: k_order_count - the tile ranked (rank_tile), the tile's count of every digit to hist[digit * ntiles + tile]; scan_u32 over
//      hist, digit-major, so that its exclusive sums are each (digit, tile)'s first place in the output; k_order_scatter - the tile ranked again,
//      its pairs brought into digit order in LDS, then stored: a wavefront's stores to one digit's run are consecutive.
//   4. k_order_out: the document numbers of the final plane to order_out, their counts (the complement undone) to counts_out.
// rank_tile ranks without an atomic per key: a wavefront takes 64 consecutive keys per round, one per lane; eight __ballots, one per bit of the
// digit, leave every lane the mask of the lanes with ITS digit; its rank among them is an mbcnt, and the highest of them adds their number to
// the wavefront's counter of that digit in LDS.  The counters of the four wavefronts are then scanned per digit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tm_pipeline.h"
#include "tm_collate.h"

namespace tmh {

constexpr uint32_t ORD_T = 256, ORD_PER = 8, ORD_TILE = ORD_T * ORD_PER, ORD_WAVES = ORD_T / 64, ORD_DIGITS = 256;
static_assert(ORD_DIGITS == ORD_T, "one work-item per digit where the digits are scanned");

struct OrderArgs {
  const uint64_t* toff;       // tok_offsets + first_doc
  uint32_t n, first, desc, ntiles;
};
// the two planes of pairs, the digit counts and their scan, the tiles' maxima and the word they fold into
struct OrderBuf { uint64_t* bases; uint64_t* sums; uint64_t* total; uint32_t* key[2]; uint32_t* val[2]; uint32_t* hist; uint32_t* tile_max; uint32_t* max; };

// the place inside its tile of the key that lane `lane` of wavefront `wave` holds in round k: a wavefront owns 64 * ORD_PER consecutive keys
__device__ __forceinline__ uint32_t ord_slot(uint32_t wave, uint32_t k, uint32_t lane) { return wave * (64 * ORD_PER) + k * 64 + lane; }
// pass `pass` has work: the largest count has a bit in that digit or above
__device__ __forceinline__ bool ord_live(const uint32_t* __restrict__ max, uint32_t pass) { return (*max >> (8 * pass)) != 0u; }

// ---- rank_tile: the keys of a tile and the rank of each among the keys of its wavefront with the same digit ---------------------------------
// cnt[w][d] afterwards: the keys of wavefront w with digit d.  Stable: ranks rise with the place in the tile (round by round, lane by lane).
__device__ __forceinline__ void rank_tile(const uint32_t* __restrict__ keys, uint32_t base, uint32_t n, uint32_t shift, uint32_t (*cnt)[ORD_DIGITS],
                                          uint32_t* key, uint32_t* rank) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (uint32_t w = 0; w < ORD_WAVES; w++) cnt[w][threadIdx.x] = 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < ORD_PER; k++) {
    const uint32_t i = base + ord_slot(wave, k, lane);
    const bool valid = i < n && i >= base;             // (i >= base: no wrap in the last tile of 2^32 - 1 documents)
    key[k] = valid ? keys[i] : 0u;
    const uint32_t d = (key[k] >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (uint32_t bit = 0; bit < 8; bit++) {
      const unsigned long long m = __ballot((d >> bit) & 1u);
      peers &= ((d >> bit) & 1u) ? m : ~m;
    }
    const uint32_t before = cnt[wave][d];
    rank[k] = before + mbcnt64(peers, 0u);
    __builtin_amdgcn_wave_barrier();                   // (every lane has read the counter before one of them moves it on)
    if (valid && ((peers >> lane) >> 1) == 0ull) cnt[wave][d] = before + (uint32_t)__popcll(peers);      // the highest lane with this digit
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
}

// ---- k_order_keys: the pairs in document order ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ORD_T) void k_order_keys(OrderArgs a, uint32_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ tile_max) {
  __shared__ uint32_t wmax[ORD_WAVES];
  const uint32_t base = blockIdx.x * ORD_TILE;
  uint32_t mx = 0;
  for (uint32_t k = 0; k < ORD_PER; k++) {
    const uint32_t i = base + k * ORD_T + threadIdx.x;
    if (i < a.n && i >= base) {
      const uint32_t c = (uint32_t)std::min<uint64_t>(a.toff[i + 1] - a.toff[i], 0xFFFFFFFFull);
      key[i] = a.desc ? ~c : c;
      val[i] = a.first + i;
      mx = std::max(mx, c);
    }
  }
  for (int off = 32; off > 0; off >>= 1) mx = std::max(mx, __shfl_xor(mx, off));
  if ((threadIdx.x & 63u) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < ORD_WAVES; w++) mx = std::max(mx, wmax[w]);
    tile_max[blockIdx.x] = mx;
  }
}

// ---- k_order_max: the largest count of all -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ORD_T) void k_order_max(const uint32_t* __restrict__ tile_max, uint32_t ntiles, uint32_t* __restrict__ max) {
  __shared__ uint32_t wmax[ORD_WAVES];
  uint32_t mx = 0;
  for (uint32_t i = threadIdx.x; i < ntiles; i += ORD_T) mx = std::max(mx, tile_max[i]);
  for (int off = 32; off > 0; off >>= 1) mx = std::max(mx, __shfl_xor(mx, off));
  if ((threadIdx.x & 63u) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < ORD_WAVES; w++) mx = std::max(mx, wmax[w]);
    *max = mx;
  }
}

// ---- k_order_count: a tile's keys per digit ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ORD_T) void k_order_count(const uint32_t* __restrict__ keys, uint32_t n, uint32_t ntiles, uint32_t pass, const uint32_t* __restrict__ max,
                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[ORD_WAVES][ORD_DIGITS];
  if (!ord_live(max, pass)) return;                    // (the whole grid)
  uint32_t key[ORD_PER], rank[ORD_PER];
  rank_tile(keys, blockIdx.x * ORD_TILE, n, 8 * pass, cnt, key, rank);
  uint32_t c = 0;
  for (uint32_t w = 0; w < ORD_WAVES; w++) c += cnt[w][threadIdx.x];
  hist[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = c;
}

// ---- k_order_scatter: a tile's pairs to their places ----------------------------------------------------------------------------------------
// The digit's first place inside the tile (an exclusive scan of the tile's digit counts: 64 digits per wavefront by shuffles, the four
// wavefronts' sums through LDS) and in the output (bases: the scan of hist); the pairs go to LDS in digit order, and work-item t stores the
// pairs t, t + ORD_T, ... of that order - neighbours in LDS are neighbours in the output wherever they share a digit.
__global__ __launch_bounds__(ORD_T) void k_order_scatter(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n, uint32_t ntiles, uint32_t pass,
                                                         const uint32_t* __restrict__ max, const uint64_t* __restrict__ bases, uint32_t* __restrict__ keys_out,
                                                         uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t cnt[ORD_WAVES][ORD_DIGITS];
  __shared__ uint32_t start[ORD_DIGITS];               // of a digit: its first place inside the tile's digit order
  __shared__ uint32_t gbase[ORD_DIGITS];               // ... and in the output
  __shared__ uint32_t wsum[ORD_WAVES];
  __shared__ uint32_t skey[ORD_TILE], sval[ORD_TILE];
  if (!ord_live(max, pass)) return;                    // (the whole grid)
  const uint32_t base = blockIdx.x * ORD_TILE, shift = 8 * pass, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t key[ORD_PER], rank[ORD_PER];
  rank_tile(keys, base, n, shift, cnt, key, rank);
  // digit threadIdx.x: its keys per wavefront -> the wavefronts' first places inside the digit's run; its total -> scanned over the digits
  uint32_t tot = 0;
  for (uint32_t w = 0; w < ORD_WAVES; w++) { const uint32_t c = cnt[w][threadIdx.x]; cnt[w][threadIdx.x] = tot; tot += c; }
  uint32_t inc = tot;                                  // inclusive scan over the 64 digits of this wavefront
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl(inc, (int)((lane - off) & 63u));
    if (lane >= off) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t w = 0; w < wave; w++) before += wsum[w];
  start[threadIdx.x] = before + inc - tot;
  gbase[threadIdx.x] = (uint32_t)bases[(uint64_t)threadIdx.x * ntiles + blockIdx.x];      // (a place among n < 2^32 pairs)
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < ORD_PER; k++) {
    const uint32_t i = base + ord_slot(wave, k, lane);
    if (i < n && i >= base) {
      const uint32_t d = (key[k] >> shift) & 255u;
      const uint32_t p = start[d] + cnt[wave][d] + rank[k];      // (< the tile's pairs: the three terms count pairs in front of this one)
      skey[p] = key[k];
      sval[p] = vals[i];
    }
  }
  __syncthreads();
  const uint32_t have = (uint32_t)std::min<uint64_t>(ORD_TILE, (uint64_t)n - base);
  for (uint32_t p = threadIdx.x; p < have; p += ORD_T) {
    const uint32_t kk = skey[p], d = (kk >> shift) & 255u;
    const uint32_t to = gbase[d] + (p - start[d]);     // (< n: the scan of hist counts every pair once)
    keys_out[to] = kk;
    vals_out[to] = sval[p];
  }
}

// ---- k_order_out: the final plane to the caller ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_order_out(OrderBuf w, uint32_t n, uint32_t desc, uint32_t launched, uint32_t* __restrict__ order, uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;                                  // (the grid covers n < 2^32 in whole workgroups: no wrap)
  const uint32_t mx = *w.max;
  uint32_t p = 0;                                      // the passes that ran: those launched that the largest count asks for
  while (p < launched && (mx >> (8 * p)) != 0u) p++;
  order[i] = w.val[p & 1u][i];
  if (counts) { const uint32_t k = w.key[p & 1u][i]; counts[i] = desc ? ~k : k; }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
static uint64_t order_tiles(uint64_t nd) { return (nd + ORD_TILE - 1) / ORD_TILE; }
static uint64_t order_scan_blocks(uint64_t cap) { return (order_tiles(cap) * ORD_DIGITS + 1 + SCAN_CH - 1) / SCAN_CH + 2; }
static uint64_t order_bytes(uint64_t cap) {
  return (order_tiles(cap) * ORD_DIGITS + 1 + order_scan_blocks(cap) + 1) * 8 + (4 * cap + order_tiles(cap) * (ORD_DIGITS + 1) + 2) * 4;
}
static OrderBuf order_buf(const tm_batch* b) {
  const uint64_t cap = b->order_cap, nt = order_tiles(cap);
  OrderBuf w;
  w.bases = reinterpret_cast<uint64_t*>(b->d_order);
  w.sums = w.bases + nt * ORD_DIGITS + 1;
  w.total = w.sums + order_scan_blocks(cap);
  w.key[0] = reinterpret_cast<uint32_t*>(w.total + 1);
  w.val[0] = w.key[0] + cap;
  w.key[1] = w.val[0] + cap;
  w.val[1] = w.key[1] + cap;
  w.hist = w.val[1] + cap;
  w.tile_max = w.hist + nt * ORD_DIGITS;
  w.max = w.tile_max + nt;
  return w;
}
static int order_reserve(tm_batch* b, uint32_t nd) {
  return batch_reserve_docs(b, (void**)&b->d_order, &b->order_cap, nd, [](uint32_t cap) { return order_bytes(cap); }, "length order");
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_batch_length_order(tm_batch* b, uint32_t first_doc, uint32_t ndocs, uint32_t flags, void* stream, uint32_t* order_out, uint32_t* counts_out) {
  if (!b) return set_error(TM_E_INVALID, "tm_batch_length_order: null argument");
  if (flags & ~TM_ORDER_DESCENDING) return set_error(TM_E_INVALID, "tm_batch_length_order: unknown flags %#x", flags);
  if (ndocs && !order_out) return set_error(TM_E_INVALID, "tm_batch_length_order: null order_out");
  if (!b->has_output) return set_error(TM_E_INVALID, "tm_batch_length_order: the batch holds no ids (no completed tm_batch_run or tm_batch_load_ids since the last upload)");
  if ((uint64_t)first_doc + ndocs > b->ndocs)
    return set_error(TM_E_INVALID, "tm_batch_length_order: documents %u .. %llu of a run of %u", first_doc, (unsigned long long)first_doc + ndocs, b->ndocs);
  int rc;
  if ((rc = enter_device(b->vocab)) != TM_OK || (rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the run: the offsets are all there)
  if (ndocs == 0) return TM_OK;
  if ((rc = order_reserve(b, ndocs)) != TM_OK) return rc;
  const OrderBuf w = order_buf(b);
  const uint32_t ntiles = (uint32_t)order_tiles(ndocs), desc = (flags & TM_ORDER_DESCENDING) ? 1u : 0u;
  const OrderArgs a{b->d_tok_offsets + first_doc, ndocs, first_doc, desc, ntiles};
  // no document holds more ids than the run: the digits above the total's are launched for no one
  uint32_t passes = 0;
  while (passes < 4 && (b->last_totals[1] >> (8 * passes)) != 0) passes++;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  TM_LAUNCH(k_order_keys, ntiles, ORD_T, 0, st, a, w.key[0], w.val[0], w.tile_max);
  TM_LAUNCH(k_order_max, 1, ORD_T, 0, st, w.tile_max, ntiles, w.max);
  for (uint32_t p = 0; p < passes; p++) {
    const uint32_t from = p & 1u, to = from ^ 1u;
    TM_LAUNCH(k_order_count, ntiles, ORD_T, 0, st, w.key[from], ndocs, ntiles, p, w.max, w.hist);
    scan_u32(w.hist, (uint64_t)ntiles * ORD_DIGITS, w.sums, w.total, w.bases, st);
    TM_LAUNCH(k_order_scatter, ntiles, ORD_T, 0, st, w.key[from], w.val[from], ndocs, ntiles, p, w.max, w.bases, w.key[to], w.val[to]);
  }
  TM_LAUNCH(k_order_out, grid_of(ndocs), 256, 0, st, w, ndocs, desc, passes, order_out, counts_out);
  return launch_check();
}

}  // extern "C"

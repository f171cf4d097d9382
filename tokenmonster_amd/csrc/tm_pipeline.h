// tm_pipeline.h — shared by the HIP translation units of libtokenmonster_hip.so: constants of the segment pipeline,
// the tm_batch workspace behind the opaque handle, and the host-side entry points one unit offers the others.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "tm_device.h"
#include "tm_norm_masks.h"

namespace tmh {

constexpr int SEG = 256;                 // bytes of one document segment (one wavefront); 256 -> 28 wavefronts per CU (LDS)
constexpr int NPOS = SEG + 40;           // positions whose descriptors a segment needs (look-ahead <= 40)
constexpr int NPOS_PAD = (NPOS + 63) / 64 * 64;
constexpr int TEXT_LEN = SEG + 96;       // staged text: position i may read up to i + 40
constexpr int RAW_PIECE = 1024;          // bytes of raw text in one piece of the device normalizer (tm_norm.hip)
constexpr int SLAB_BYTES = 2048;         // the device normalizer's slab for one 1 KiB piece of raw text (tm_norm.hip); K1 can stage the text from there
constexpr int ENT = 80;                  // entry states of a segment: 40 offsets x fd{0,1}
#ifndef TM_K1_WAVES
#define TM_K1_WAVES 4
#endif
constexpr int WAVES = TM_K1_WAVES;                 // wavefronts per workgroup in K1 (8: +14 %, the halo barrier couples more wavefronts)
constexpr uint32_t R_INVALID = 0xFFFFFFFFu;
constexpr uint32_t J_EXIT = 1024;           // jump targets >= J_EXIT: left the segment; J_EXIT + next entry state
constexpr uint32_t J_INVALID = 2047;        // state is not reachable (no forward-delete match there)
constexpr uint32_t ID_NONE = 0xFFFFFFu;
constexpr int NOSCORE = -1000000;
constexpr int SIDE_STRIDE = 16;            // uint2 entries of a segment's side list: [0] = {count or SIDE_DENSE, 0}, then {position, T(p,1)}
constexpr uint32_t SIDE_DENSE = 0xFFFFFFFFu;  // more (p,1) states than the list holds: they are in the dense R1 array instead
constexpr uint32_t LONG_SEGS = 512;        // documents with more segments than this are resolved hierarchically

constexpr int SCAN_T = 256, SCAN_PER = 16, SCAN_CH = SCAN_T * SCAN_PER;   // exclusive scan u32 -> u64: elements per workgroup

// segment groups of long documents (hierarchical resolve, tm_kernels.hip)
constexpr uint32_t GROUP_FAN = 64;         // children per group of the tree over a long document's segments
struct Group { uint32_t first_child, nchildren, doc, level; };   // children: segments (level 0 = leaf groups) or groups of the level below
struct LongDoc { uint32_t doc, first_group, ngroups, pad; };

// per-lane select on a wave-uniform lane mask: bit set -> a, else b (one v_cndmask, the mask stays in scalar registers)
__device__ __forceinline__ uint32_t sel_mask(unsigned long long mask, uint32_t a, uint32_t b) {
#ifdef TM_EMU
  return ((mask >> emu::cur->lane) & 1ull) ? a : b;
#else
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(mask));
  return r;
#endif
}
// bit (n & 31) of x: v_bfe_u32 takes the low five bits of its offset operand by itself, the compiler does not drop the `& 31` of the C form
__device__ __forceinline__ uint32_t bit_of(uint32_t x, uint32_t n) {
#ifdef TM_EMU
  return (x >> (n & 31u)) & 1u;
#else
  return __builtin_amdgcn_ubfe(x, n, 1u);
#endif
}
// a + (bit of the lane in a wave-uniform mask): the mask goes in as the carry of ONE add (v_addc_co), instead of an add and a select
__device__ __forceinline__ uint32_t add_mask_bit(uint32_t a, unsigned long long mask) {
#ifdef TM_EMU
  return a + (uint32_t)((mask >> emu::cur->lane) & 1ull);
#else
  uint32_t r;
  unsigned long long carry_out;
  asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r), "=s"(carry_out) : "v"(a), "s"(mask));
  return r;
#endif
}
// the value a wave-uniform lane holds, as a scalar (v_readlane)
__device__ __forceinline__ uint32_t read_lane(uint32_t v, int l) {
#ifdef TM_EMU
  return __shfl(v, l);
#else
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
#endif
}
// The value another lane holds as an operand of this lane's next instruction (a DPP move: no LDS round trip).  ctrl: 0x110 + n = row_shr:n
// (rows of 16 lanes), 0x138 = wave_shr:1, 0x130 = wave_shl:1, 0x142 / 0x143 = row_bcast:15 / row_bcast:31; rows: which rows of 16 lanes take part.
// A lane without a source - shifted in from outside its row / the wavefront, or in a row that does not take part - keeps `old`.
#ifdef TM_EMU
static inline uint32_t tm_dpp_emu(uint32_t old, uint32_t src, int ctrl, int rows) {
  const int lane = (int)emu::cur->lane, row = lane >> 4;
  int from = lane; bool have = false;
  if (ctrl > 0x110 && ctrl <= 0x11F) { from = lane - (ctrl - 0x110); have = (lane & 15) >= ctrl - 0x110; }
  else if (ctrl == 0x138) { from = lane - 1; have = lane >= 1; }
  else if (ctrl == 0x130) { from = lane + 1; have = lane < 63; }
  else if (ctrl == 0x142) { from = row * 16 - 1; have = row >= 1; }
  else if (ctrl == 0x143) { from = 31; have = row >= 2; }
  const uint32_t v = __shfl(src, from & 63);
  return (have && ((rows >> row) & 1)) ? v : old;
}
#define TM_DPP(old, src, ctrl, rows) tm_dpp_emu(old, src, ctrl, rows)
#define TM_DPP0(src, ctrl) tm_dpp_emu(0u, src, ctrl, 0xF)
#else
#define TM_DPP(old, src, ctrl, rows) ((uint32_t)__builtin_amdgcn_update_dpp((int)(old), (int)(src), ctrl, rows, 0xF, false))
#define TM_DPP0(src, ctrl) ((uint32_t)__builtin_amdgcn_mov_dpp((int)(src), ctrl, 0xF, 0xF, true))      // all rows; a lane without a source gets 0 (bound_ctrl: no `old` to set up)
#endif
// A wavefront's window on global memory: a buffer resource (base and size wave-uniform), so that the range check is the hardware's - a dword
// load outside [base, base + bytes) returns 0 and costs no branch and no 64-bit compare (offsets are unsigned: "before the window" is
// outside too).  `bytes` a multiple of 4 and offsets multiples of 4, so that no dword is partly inside.
#ifdef TM_EMU
struct TmWindow { const uint8_t* base; uint32_t bytes; };
static inline TmWindow tm_window(const void* base, uint32_t bytes) { return TmWindow{(const uint8_t*)base, bytes}; }
static inline uint32_t tm_window_u32(const TmWindow& w, uint32_t off) { uint32_t v = 0; if (off < w.bytes && w.bytes - off >= 4u) __builtin_memcpy(&v, w.base + off, 4); return v; }
static inline uint4 tm_window_u128(const TmWindow& w, uint32_t off) { return uint4{tm_window_u32(w, off), tm_window_u32(w, off + 4), tm_window_u32(w, off + 8), tm_window_u32(w, off + 12)}; }
#else
typedef __amdgpu_buffer_rsrc_t TmWindow;
__device__ __forceinline__ TmWindow tm_window(const void* base, uint32_t bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000); }
__device__ __forceinline__ uint32_t tm_window_u32(TmWindow w, uint32_t off) { return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(w, (int)off, 0, 0); }
__device__ __forceinline__ uint4 tm_window_u128(TmWindow w, uint32_t off) {      // four dwords, each range-checked by itself
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  const v4u v = __builtin_amdgcn_raw_buffer_load_b128(w, (int)off, 0, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}
#endif
__device__ __forceinline__ uint32_t mbcnt64(unsigned long long mask, uint32_t acc) {      // acc + #set bits of mask below the lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, acc));
}

// ---- what the chain walks behind K3 share (K4 and the scoring walks in tm_kernels.hip, the span pass in tm_spans.hip) ----------------------
// narrow T(p,0) rows (vocabularies of at most 65 536 ids): per segment SEG ids (u16), then SEG bytes advance [0..5] | fd' [6] | missing [7]
constexpr uint64_t R0_NARROW = 3 * SEG;
// ... and the two-plane form of the larger vocabularies (round 6): SEG ids (u32: id, 0xFFFFFF = none), then the same SEG flag bytes - so that K4's
// position-staging walk (k_emit_list), which only looks at the flag plane, serves them too.  `narrow` of k_match_branch: 0 = one plane of
// u32 words (id | advance << 24 | fd' << 30 | missing << 31: the id-staging walks k_emit_tiles<false> / k_score_tiles read these), 1 = u16 + u8, 2 = u32 + u8
constexpr uint64_t R0_WIDE = 5 * SEG;
// the position-staging walks (k_emit_list, k_score_list, k_span_list): segments per wavefront, slack in front of a row's flag bytes, bytes per row in LDS
#ifndef TM_K4_TSL
#define TM_K4_TSL 16
#endif
constexpr int TSL = TM_K4_TSL, TSLACK_L = 4, TROW_L = SEG + 16;

struct TileSeg { bool have; uint64_t begin, base; uint32_t seglen, entry; };   // one segment of the tile per lane (lanes >= TS: have == false)
__device__ __forceinline__ TileSeg tile_segment(const uint4* __restrict__ par, uint64_t g, bool lane_ok, uint64_t nseg) {
  TileSeg t{lane_ok && g < nseg, 0, 0, 0, 0};
  if (t.have) {
    const uint4 q = par[g];
    t.begin = (uint64_t)q.x | ((uint64_t)(q.y & 0xFFu) << 32);
    t.seglen = (q.y >> 8) & 0xFFFu;
    t.entry = (q.y >> 20) & 0x7Fu;
    t.base = (uint64_t)q.z | ((uint64_t)q.w << 32);
  }
  return t;
}
// T(p,1) of a segment: from its side list, or from the dense array when the list overflowed
__device__ __forceinline__ uint32_t side_word(const uint2* __restrict__ sl, const uint32_t* __restrict__ R1, uint64_t g, uint32_t p) {
  const uint32_t nside = sl[0].x;
  if (nside == SIDE_DENSE) return R1[g * SEG + p];
  uint32_t w = R_INVALID;
  for (uint32_t k = 1; k <= nside && k < (uint32_t)SIDE_STRIDE; k++) { const uint2 sv = sl[k]; if (sv.x == p) w = sv.y; }
  return w;
}

}  // namespace tmh

struct tm_batch {
  const tm_vocab* vocab = nullptr;
  uint64_t max_bytes = 0;
  uint32_t max_docs = 0;
  uint64_t max_segs = 0;
  uint64_t nbytes = 0, nseg = 0;
  uint32_t ndocs = 0;
  uint64_t device_bytes = 0;
  hipStream_t last_stream = nullptr;
  hipStream_t aux_stream = nullptr;    // fetch of the host-fallback documents, beside the normalizer pass
  // device buffers
  uint8_t* d_text = nullptr;
  bool text_borrowed = false;          // scoring pass: text belongs to a tm_dataset
  uint64_t* d_offsets = nullptr;       // packed batches: doc_begin = d_offsets, doc_end = d_offsets + 1
  const uint64_t* d_doc_begin = nullptr;
  const uint64_t* d_doc_end = nullptr;
  const uint64_t* d_doc_vis = nullptr;   // how far a document may look at the text (null: its end); see k_match_branch
  const uint8_t* d_doc_entry = nullptr;  // entry state of a document's first segment (null: 0); see k_resolve
  uint32_t* d_doc_nseg = nullptr;
  uint64_t* d_doc_seg_start = nullptr;
  uint32_t* d_seg_doc = nullptr;
  uint32_t* d_R0 = nullptr;          // T(p,0): SEG words per segment (position p of segment g at g * SEG + p)
  uint2* d_side = nullptr;           // per segment: its few T(p,1) words (SIDE_STRIDE entries: header + {position, word})
  uint32_t* d_R1 = nullptr;          // T(p,1) per position, written only for segments whose side list overflows
  uint32_t* d_exitmap = nullptr;       // per segment: 80 entries {next entry state | #ids << 8}: written only for a segment with a count that does not fit the 16-bit form
  uint16_t* d_exit16 = nullptr;        // per segment: 80 entries {next entry state | #ids << 7}, 0xFFFF = unreachable (exit_entry, tm_kernels.hip)
  uint8_t* d_seg_entry = nullptr;
  uint32_t* d_seg_tokbase = nullptr;
  uint4* d_seg_par = nullptr;          // per segment: what K1 starts from (k_seg_fill); behind K3: begin | length | entry state | first output index (k_seg_params)
  uint32_t* d_doc_ntok = nullptr;
  uint32_t* d_doc_events = nullptr;
  uint32_t* d_doc_missing = nullptr;
  uint32_t* d_doc_fd = nullptr;        // delete tokens emitted per document (K4)
  uint64_t* d_tok_offsets = nullptr;
  uint64_t* d_scan_tmp = nullptr;   // block sums
  uint64_t* d_totals = nullptr;     // [0] nseg total (device-computed), [1] token total, [2] missing total
  uint32_t* d_error = nullptr;
  // long documents (hierarchical resolve)
  uint32_t ngroups = 0, nlong = 0, cap_groups = 0, cap_long = 0;
  std::vector<uint32_t> level_first;   // groups of level k+1 are d_groups[level_first[k] .. level_first[k+1])
  tmh::Group* d_groups = nullptr;
  tmh::LongDoc* d_longs = nullptr;
  uint2* d_gmap = nullptr;
  uint8_t* d_group_entry = nullptr;
  uint32_t* d_group_base = nullptr;
  // raw (un-normalized) input of tm_batch_upload_raw / tm_batch_normalize
  uint8_t* d_raw = nullptr;
  // the filter pass of a vocabulary with byte-level normalization flags (tm_norm.hip: k_pf_*): the filtered text and its documents
  uint8_t* d_rawf = nullptr; uint64_t rawf_cap = 0;
  uint64_t* d_rawf_off = nullptr; uint64_t rawf_docs_cap = 0;
  uint8_t* d_pf_piece = nullptr; uint64_t pf_piece_cap = 0;      // (bytes of PfPiece)
  void* d_pf_doc = nullptr;
  uint32_t* d_acc = nullptr;             // what `accents` leaves of the two-byte characters
  uint8_t* d_slab = nullptr;            // normalizer: one 2 KiB slab per 1 KiB piece
  uint64_t slab_pieces = 0;             // pieces of the batch that was normalized last (raw_pieces may already count the next upload)
  bool text_in_slabs = false;           // the normalized text of this batch has not been packed into d_text: K1 stages it from the slabs (k_seg_fill)
  uint64_t slab_cap = 0;
  uint64_t* d_raw_off = nullptr;
  uint64_t raw_cap = 0, raw_bytes = 0, raw_pieces = 0, piece_cap = 0;
  uint32_t raw_docs = 0, raw_docs_cap = 0;
  std::vector<uint64_t> h_raw_off;
  uint32_t host_fallback_docs = 0;
  uint32_t* d_doc_npiece = nullptr;     // pieces per raw document, then (scan) first piece of each document
  uint64_t* d_doc_piece_start = nullptr;
  uint32_t* d_piece_doc = nullptr;
  uint32_t* d_piece_sum = nullptr;      // per-piece run summary (pass 1)
  uint8_t* d_piece_carry = nullptr;     // per-piece carries (pass 2)
  uint32_t* d_piece_len = nullptr;      // normalized bytes per piece (pass 3)
  uint64_t* d_piece_off = nullptr;      // their exclusive scan
  tmh::NmTwo* d_two = nullptr;          // the device normalizer's table of the two-byte characters (tm_norm_masks.h)
  uint8_t* d_need_host = nullptr;       // per document: needs the host normalizer
  uint64_t* d_nbegin = nullptr;         // normalized document ranges (GPU documents packed first, fallback documents after)
  uint64_t* d_nend = nullptr;
  uint64_t* d_ninfo = nullptr;          // [0] #fallback docs [1] #long docs [2] #segments (device-computed)
  // grow-only staging for the host fallback
  uint64_t* d_fb_roff = nullptr; uint64_t* d_fb_noff = nullptr; uint32_t* d_fb_ids = nullptr;   // lists of the host-fallback documents
  // small transfers (counters, lists of a few hundred KB) go through a pinned mailbox and a copy kernel on the caller's stream
  // instead of the copy engines, where they would queue behind the bulk transfers of other lanes (small_d2h / small_h2d)
  uint8_t* h_mail = nullptr; uint64_t mail_pos = 0;
  uint8_t* h_groups = nullptr; uint64_t h_groups_cap = 0;   // pinned staging of the group tree of long documents (build_groups)
  struct MailPending { void* dst; const uint8_t* slot; uint64_t n; hipStream_t st; };
  std::vector<MailPending> mail_pending;
  std::vector<hipStream_t> mail_streams;   // streams that have used mailbox slots since it last wrapped
  uint64_t last_totals[3] = {0, 0, 0};   // d_totals as read by ensure_output
  uint8_t* h_fb_raw = nullptr; uint8_t* h_fb_norm = nullptr;     // pinned host staging of the fallback documents (raw in, normalized out)
  uint64_t h_fb_raw_cap = 0, h_fb_norm_cap = 0;
  uint32_t* d_out = nullptr;
  uint64_t out_cap = 0;
  bool has_output = false;              // ids and offsets of a completed run (or of tm_batch_load_ids) lie in d_out / d_tok_offsets: what tm_batch_collate / tm_batch_pack ask for
  int row_form = -1;                    // the form of the T(p,0) rows the last id-emitting run left (k_match_branch's `narrow`: 0 one plane of u32 words, 1 u16 + u8, 2 u32 + u8); -1: the ids did not come from a walk
  uint2* d_spans = nullptr;             // tm_batch_collate_spans / tm_tokenize_batch_spans: the ragged (begin, end) pairs of the ids, grow-only (tm_spans.hip)
  uint64_t spans_cap = 0;
  uint32_t* d_own = nullptr;            // tm_batch_raw_spans: per byte of the normalized text, the raw offset of the unit that owns it, grow-only (origin pass, tm_norm.hip)
  uint64_t own_cap = 0;
  uint8_t* d_own_tmp = nullptr;         // ... and what k_norm_carry writes on the side when the origin pass runs it again
  uint64_t own_tmp_cap = 0;
  uint8_t* d_units[2] = {nullptr, nullptr};   // tm_batch_spans_in: the unit index of the normalized [0] / the raw [1] text, grow-only (tm_units.hip: two planes of UnitPlane)
  uint64_t units_cap[2] = {0, 0};       // ... in 256-byte blocks of text
  uint64_t units_blocks[2] = {0, 0};    // ... and the blocks of the text the planes were made for
  uint32_t units_have[2] = {0, 0};      // which planes hold the current text: bit 0 non-continuation bytes, bit 1 bytes >= 0xF0; 0 again wherever new text arrives (units_forget)
  uint8_t* d_win = nullptr;             // tm_batch_windows: win_off[cap + 1] (u64) | the scan's block sums and total (u64) | windows per document (u32), grow-only (tm_windows.hip)
  uint32_t win_cap = 0;                 // ... in documents
  uint32_t* d_win_rows = nullptr;       // ... and the document of every row of the last window call, grow-only
  uint64_t win_rows_cap = 0;
  uint16_t* d_out16 = nullptr;          // set for the length of a launch: K4 writes two-byte ids here instead (a chunk of the ring, launch_emit)
  uint64_t out16_cap = 0;
  // a chunk of the host-to-host ring (tm_host.hip): what the host would have read back between the stages - the number of segments the normalizer
  // pass left, whether the chunk can be taken on this path at all, the number of ids - stays on the device in these control words, and the
  // kernels behind the pass are launched over a bound and look the counts up (d_ctl != null; k_chunk_ctl / k_chunk_done, tm_kernels.hip)
  uint64_t* d_ctl_store = nullptr;      // 8 words, allocated on first use
  const uint64_t* d_ctl = nullptr;      // = d_ctl_store while the workspace belongs to a slot of the ring
  // tm_batch_decode (tm_decode.hip): the ids of this batch decoded where they lie - two grow-only arenas and what the last call left in them
  uint8_t* d_dec_a = nullptr; uint64_t dec_a_cap = 0;      // lengths, byte offset of every id, scan sums, the documents' offsets and decoded lengths
  uint8_t* d_dec_b = nullptr; uint64_t dec_b_cap = 0;      // the gathered bytes | the same after capcode decoding
  uint64_t dec_total = 0, dec_o_doff = 0, dec_o_declen = 0, dec_o_dec = 0;
  uint32_t dec_ndocs = 0;
  bool dec_raw = false;                                     // decode_raw: the gathered bytes are the result
  bool dec_capcode = false;                                 // the capcode decoder ran on the device (else the gathered bytes are the result, or all the host's)
  hipEvent_t ev[TM_NUM_KERNELS + 1] = {};
  bool have_events = false;
};

// device-resident normalized dataset of the scoring pass (tm_score.hip)
struct tm_dataset {
  uint8_t* d_text = nullptr;
  uint64_t n = 0;
  tm_batch* ws = nullptr;          // workspace, created on first use and reused by every scoring pass
  uint32_t ws_docs = 0;
  uint32_t* d_hist = nullptr;      // scores | 4 token limbs | 256 missing counters
  uint64_t hist_words = 0, hist_cap = 0;
  unsigned long long* d_tokens = nullptr;
  uint32_t* d_missing_bits = nullptr;
  int n_cu = 256;
  int device = 0;
  // byte ranges of a whole-buffer walk (tm_score_begin / tm_score_finish)
  uint64_t* d_vis = nullptr;       // per strip: how far it may look at the text
  uint8_t* d_entry = nullptr;      // per strip: entry state
  uint8_t* d_exits = nullptr;      // per strip: exit state for each of the ENT entry states
  uint32_t strip_cap = 0;
  bool prepared = false;
  // the strips of the last pass, as the workspace holds them on the device (score_prepare: a pass over the same strips does not upload them again)
  std::vector<uint64_t> strips_key; const tm_batch* ws_strips_owner = nullptr; bool strips_valid = false;
  // one scoring pass at a time per dataset (it owns ONE workspace); host threads that build and load the next candidates
  // (tm_build_vocab, tm_vocab_load) run beside the pass of the current one
  std::mutex mu;
  hipStream_t stream = nullptr;    // tm_score's own stream
};

namespace tmh {

// tm_kernels.hip
int make_workspace(const tm_vocab* v, uint64_t max_bytes, uint32_t max_docs, bool own_text, bool with_output, tm_batch** out);
void scan_u32(const uint32_t* in, uint64_t n, uint64_t* block_sums, uint64_t* total, uint64_t* out, hipStream_t st);
void launch_doc_units(const uint64_t* doc_begin, const uint64_t* doc_end, uint32_t ndocs, uint32_t unit, uint32_t* doc_nunits, hipStream_t st);
void launch_unit_owner(const uint64_t* doc_unit_start, uint32_t ndocs, uint64_t nunits, uint32_t* unit_doc, hipStream_t st, const uint64_t* count_dev = nullptr);      // count_dev: nunits is a bound, this the count
// (TM_TRACE: every buffer that is replaced by a larger one after a workspace exists - each is a hipFree, which waits for the whole device)
inline void trace_grow(const char* what, uint64_t bytes) { static const bool on = getenv("TM_TRACE") != nullptr; if (on) fprintf(stderr, "[grow] %s -> %.2f MB\n", what, bytes / 1048576.0); }
int reserve_groups(tm_batch* b, uint32_t ngroups, uint32_t nlong);
int debug_flags();        // the test hooks in force (tm_debug_flags)
bool hooks_armed();       // the process was started with TM_TEST_HOOKS in its environment: only then do tm_debug_flags / TM_VIRTUAL_DEVICES change anything
uint32_t long_segs();    // documents with more segments than this hang under the group tree (LONG_SEGS; 8 under test hook bit 12)
int build_groups(tm_batch* b, const uint64_t* begin, const uint64_t* end, uint32_t ndocs, hipStream_t st);
int run_pipeline(tm_batch* b, hipStream_t st, bool timed, float* ms, bool emit);
int pipeline_match(tm_batch* b, hipStream_t st, hipEvent_t* ev, bool for_score = false);      // for_score: the rows are for the scoring walk (tm_score.hip)
int pipeline_resolve(tm_batch* b, hipStream_t st, hipEvent_t* ev, int mode);
void launch_doc_exits(tm_batch* b, uint8_t* d_exits, hipStream_t st);
// the streaming encoder's step from one pass to the next (k_enc_carry): entry state, missing count and the `keep` bytes of look-ahead, all on the device
void launch_enc_carry(tm_batch* b, const uint8_t* d_exits, uint8_t* d_entry, uint32_t* d_acc, uint64_t own, uint32_t keep, hipStream_t st);
// tm_tokenize_document's step from one slot to the next (k_doc_chain) and the second half of a piece behind it (tm_kernels.hip)
void launch_doc_chain(tm_batch* b, uint32_t* d_cell, const uint8_t* d_exits, uint8_t* d_entry, uint64_t* d_ctl, uint64_t nseg, uint64_t from, uint32_t keep,
                      uint8_t* next_text, hipStream_t st);
int doc_enqueue_resolve(tm_batch* b, hipStream_t st, uint32_t enc, uint64_t* d_ctl, uint8_t* d_bytes, uint64_t d_bytes_cap, uint64_t* h_status, uint64_t* h_scratch,
                        const uint8_t** ids_at);
int doc_redo_emit(tm_batch* b, hipStream_t st, uint64_t* d_ctl);
// scoring variant of the chain kernel: histogram in HBM (scores | 4 limbs | 256 counters), see tm_score.hip
bool raw_upload_replaces_buffers(const tm_batch* b, const uint64_t* raw_offsets, uint32_t ndocs);
void pack_text(tm_batch* b, hipStream_t st);     // tm_norm.hip: the normalizer's slabs packed into d_text (no-op unless text_in_slabs)
void launch_chain_hist(tm_batch* b, uint32_t delete_id, int n_cu, uint32_t* d_hist, unsigned long long* d_tokens, uint32_t* d_missing_bits,
                       uint32_t n_ids, hipStream_t st);
int ensure_output(tm_batch* b);
// HIP events on `st` around the parts of a call that reports times: n events, or none at all (n = 0: the caller wants no times, nothing
// here touches the device).  mark(k) records event k; finish waits for the last one, writes the n - 1 times between neighbouring marks to
// `ms` and returns rc - or, where the work succeeded and an event did not, that failure.
struct EventBracket {
  hipStream_t st;
  int n;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  EventBracket(hipStream_t stream, int count) : st(stream), n(count) { for (int k = 0; k < n && e == hipSuccess; k++) e = hipEventCreate(&ev[k]); }
  void mark(int k) { if (n && e == hipSuccess) e = hipEventRecord(ev[k], st); }
  int finish(float* ms, int rc) {
    if (n && e == hipSuccess) e = hipEventSynchronize(ev[n - 1]);
    for (int k = 0; k + 1 < n && e == hipSuccess; k++) e = hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
    for (int k = 0; k < n; k++) if (ev[k]) (void)hipEventDestroy(ev[k]);
    return rc == TM_OK && e != hipSuccess ? hip_fail(e, "HIP events") : rc;
  }
};
// tm_spans.hip: the byte span of every id of the last run.  batch_spans_on: the pass itself on `st` into `out` (device or page-locked, 8-byte
// aligned, room for `total` pairs) - the caller has waited for the run (ensure_output)
int spans_ready(const tm_batch* b, const char* who);
int batch_spans_on(tm_batch* b, hipStream_t st, void* out, uint64_t total);
// tm_norm.hip: origin_ready - the batch's text came from tm_batch_upload_raw + tm_batch_normalize and every raw document is shorter than 2^32
// bytes; origin_pass_on - the owner of every normalized byte into b->d_own (indexed like the documents' ranges d_doc_begin), *host_docs = the
// documents mapped on the host.  Reads what the normalizer and the run left, changes none of it.
int origin_ready(const tm_batch* b, const char* who);
int origin_pass_on(tm_batch* b, hipStream_t st, uint32_t* host_docs);
int batch_raw_spans_on(tm_batch* b, hipStream_t st, void* out, uint64_t total, uint32_t* host_docs, float* ms);      // tm_spans.hip: batch_spans_on into d_spans, origin_pass_on, k_raw_spans; ms[3] (may be null) as tm_batch_raw_spans_timed states
// tm_units.hip: the pairs counted in code points or UTF-16 units (tokenmonster_hip.h, character offsets).  units_args: `text` and `unit` are known
// (TM_E_INVALID otherwise; the callers ask origin_ready for TM_TEXT_RAW themselves).  batch_spans_in_on: the byte pairs of `text` into `out` and
// their conversion in place (nothing for TM_UNIT_BYTES), ms[4] (may be null) as tm_batch_spans_in states.  units_forget: new text has arrived
// (kinds: bit 0 the normalized text, bit 1 the raw text).
int units_args(uint32_t text, uint32_t unit, const char* who);
int batch_spans_in_on(tm_batch* b, hipStream_t st, uint32_t text, uint32_t unit, void* out, uint64_t total, uint32_t* host_docs, float* ms);
inline void units_forget(tm_batch* b, uint32_t kinds) { if (kinds & 1u) b->units_have[0] = 0; if (kinds & 2u) b->units_have[1] = 0; }
// tm_spans.hip: the bodies the span calls share (text: TM_TEXT_*, unit: TM_UNIT_*; `who` names the entry point).  batch_own_spans_on: the pairs
// of `text` in `unit` into the batch's own buffer d_spans, grown for `total` pairs; ragged_spans_impl: tm_batch_spans, tm_batch_raw_spans(_timed)
// and tm_batch_spans_in; collate_spans_impl: tm_batch_collate_spans, tm_batch_collate_raw_spans and tm_batch_collate_spans_in
int batch_own_spans_on(tm_batch* b, hipStream_t st, uint32_t text, uint32_t unit, uint64_t total);
int ragged_spans_impl(tm_batch* b, void* stream, uint32_t text, uint32_t unit, uint32_t* spans_out, uint64_t spans_cap, uint32_t* host_docs, float* ms, const char* who);
int collate_spans_impl(tm_batch* b, const tm_collate* how, void* stream, uint32_t text, uint32_t unit, void* spans_out, uint32_t span_bytes, const char* who);
// small device <-> host transfers that bypass the copy engines (tm_kernels.hip).  small_d2h's destination is filled by small_sync
// (which synchronizes the stream); small_h2d's source may be reused as soon as the call returns (pageable memory, or at most MAIL_MAX bytes).
constexpr uint64_t MAIL_BYTES = 4ull << 20, MAIL_MAX = 1ull << 20;
int small_d2h(tm_batch* b, void* host_dst, const void* dev_src, uint64_t bytes, hipStream_t st);
int small_h2d(tm_batch* b, void* dev_dst, const void* host_src, uint64_t bytes, hipStream_t st);
int small_sync(tm_batch* b, hipStream_t st);
// Grow-only buffers outside tm_batch::device_bytes (tm_kernels.hip): lanes, ring slots, document slots, the decode arenas, the normalizer's texts and staging.  A buffer of at least `need` bytes
// stays; a smaller one is replaced by one of `alloc` bytes (the caller's headroom), and `what` names it in the [grow] line of TM_TRACE and in the
// error message.  On failure the pointer is null and the capacity 0.
bool is_pinned(const void* p);      // page-locked host memory (hipHostMalloc / hipHostRegister)
int grow_device(uint8_t** buf, uint64_t* cap, uint64_t need, uint64_t alloc, const char* what);
int grow_pinned(uint8_t** buf, uint64_t* cap, uint64_t need, uint64_t alloc, const char* what);
// ... and the same contract for the grow-only buffers a batch owns, which count in tm_batch::device_bytes (ids, spans, origins and their scratch,
// window rows): `cap`, `need` and `alloc` in elements of elem_bytes.  batch_replace is the step behind it for a buffer whose size is no multiple of
// its capacity (windows, the unit index): *p of old_bytes, too small for need_bytes, replaced by one of alloc_bytes; the caller keeps the capacity.
int grow_batch(tm_batch* b, void** p, uint64_t* cap, uint64_t need, uint64_t alloc, uint32_t elem_bytes, const char* what);
int batch_replace(tm_batch* b, void** p, uint64_t old_bytes, uint64_t need_bytes, uint64_t alloc_bytes, const char* what);
// ... and a workspace of `v` for `bytes` of text in `docs` documents: a smaller one (or another vocabulary's) is replaced by one of alloc_bytes and docs + 25 %
int grow_workspace(tm_batch** ws, const tm_vocab* v, uint64_t bytes, uint32_t docs, uint64_t alloc_bytes, const char* what);
int batch_upload_on(tm_batch* b, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, hipStream_t st);
void launch_serialize(const uint32_t* ids, uint64_t n, uint32_t enc, uint8_t* out, hipStream_t st);
// the host-to-host ring: a chunk's stages behind the upload enqueued on `st` without a host round trip (tm_norm.hip / tm_kernels.hip)
constexpr uint32_t RING_HOST_DOCS = 1, RING_LONG_DOCS = 2, RING_UNDECIDED = 4, RING_SLAB = 8, RING_SHORT_PIECE = 16, RING_BYTES = 32, RING_SEGS = 64,
                   RING_ERROR = 128, RING_OUT_CAP = 256;      // status bits of a chunk the ring hands to the exact path instead
bool ring_supported(const tm_vocab* v);
uint64_t raw_piece_count(const tm_vocab* v, const uint64_t* offsets, uint32_t ndocs);      // the 1 KiB pieces of these raw documents, as raw_prepare wants them counted
int raw_prepare(tm_batch* b, uint64_t nbytes, uint32_t ndocs, uint64_t npieces, hipStream_t st);      // the buffers tm_batch_upload_raw fills, grown to size
void raw_free(tm_batch* b);      // ... and freed, with the filter pass's (tm_batch_free)
int ring_enqueue_normalize(tm_batch* b, hipStream_t st, uint64_t seg_bound, const uint64_t* h_raw_off);      // h_raw_off: the chunk's document offsets on the host (ndocs + 1)
void launch_chunk_ctl(tm_batch* b, uint64_t seg_bound, hipStream_t st);
// K0 .. K4, the ids packed to `enc` bytes into d_bytes (16-byte aligned), and the chunk's verdict written to `h_status` (page-locked host memory, 8 words:
// status bits, ids, normalized bytes, segments, device error word)
// *ids_at: where the packed ids lie when the stream gets there - d_bytes, or the workspace's own id buffer (four-byte ids need no packing)
int ring_enqueue_tokenize(tm_batch* b, hipStream_t st, uint32_t enc, uint8_t* d_bytes, uint64_t d_bytes_cap, uint64_t* h_status, const uint8_t** ids_at);
// The wait for such a verdict (a chunk of the ring, a piece of tm_tokenize_document): a word in page-locked memory that the host has set to ~0
// and the last kernel on the stream writes, `done` the event recorded behind that kernel.  The word is WATCHED instead of slept for in
// hipEventSynchronize - on some boxes every other call lost 3.2 ms right there, in the wait for its first chunk (round 6's per-chunk
// trace, tools/r06_probe25.sh: every chunk of a 30.5 ms call lies 3.2 ms behind its place in a 26.9 ms call, from chunk 0 on).  The event is still asked now and then: a stream
// that has failed must not be waited for for ever.  hipSuccess with the word still ~0: the stream ended without writing it.
#if defined(__x86_64__) || defined(__i386__)
#define TM_CPU_RELAX() __builtin_ia32_pause()
#else
#define TM_CPU_RELAX() ((void)0)
#endif
inline hipError_t wait_verdict(const volatile uint64_t* flag, hipEvent_t done) {
  for (uint32_t spin = 1;; spin++) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != ~0ull) return hipSuccess;
    if ((spin & 0xFFFu) == 0) {
      const hipError_t q = hipEventQuery(done);
      if (q == hipSuccess) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == ~0ull ? hipEventSynchronize(done) : hipSuccess;
      if (q != hipErrorNotReady) return q;
    }
    TM_CPU_RELAX();
  }
}
// tm_decode.hip: the stages of a decode on a stream, in buffers of the caller
constexpr uint64_t DEC_HOST = ~0ull;      // k_dec_capcode's length of a document it leaves to the host decoder (scripts beyond Latin, malformed UTF-8)
// the arena of a decode behind `base` bytes of the caller's own: byte counts of the tiles of ids (tm_decode.hip) | first document of a tile | byte offset of a
// tile | scan block sums | total | byte offset of every document | decoded length of every document
struct DecArena { uint64_t ntiles, o_len, o_first, o_off, o_sums, o_total, o_doff, o_declen, bytes; };
constexpr uint32_t DEC_TILE_IDS = 2048;
inline uint64_t dec_up(uint64_t x) { return (x + 255) & ~(uint64_t)255; }      // the parts of the decode's arenas begin on 256-byte boundaries
inline DecArena dec_arena(uint64_t base, uint64_t n, uint32_t ndocs) {
  const auto up = dec_up;
  DecArena a;
  a.ntiles = (n + DEC_TILE_IDS - 1) / DEC_TILE_IDS;
  const uint64_t sblocks = (a.ntiles + 1 + SCAN_CH - 1) / SCAN_CH + 2;
  a.o_len = up(base); a.o_first = a.o_len + up((a.ntiles + 1) * 4); a.o_off = a.o_first + up((a.ntiles + 1) * 4); a.o_sums = a.o_off + up((a.ntiles + 2) * 8);
  a.o_total = a.o_sums + up(sblocks * 8); a.o_doff = a.o_total + 256; a.o_declen = a.o_doff + up(((uint64_t)ndocs + 1) * 8); a.bytes = a.o_declen + up((uint64_t)ndocs * 8 + 8);
  return a;
}
// lengths: the bytes of every tile and their scan (the total at A + a.o_total); copy: the gather itself and the documents' byte offsets (A + a.o_doff)
void launch_decode_lengths(const tm_vocab* v, const uint32_t* d_tok, uint64_t n, const uint64_t* d_toff, uint32_t ndocs, const DecArena& a, uint8_t* A, hipStream_t st);
void launch_decode_copy(const tm_vocab* v, const uint32_t* d_tok, uint64_t n, const uint64_t* d_toff, uint32_t ndocs, const DecArena& a, uint8_t* A, uint8_t* d_out, hipStream_t st);
// d_sums: two words the kernel adds up - bytes the device decoded, documents it left to the host decoder
int launch_decode_capcode(const tm_vocab* v, const uint8_t* d_out, const uint64_t* d_doff, uint32_t ndocs, uint8_t* d_dec, uint64_t* d_declen, uint64_t* d_sums, hipStream_t st);
// The host's part of a decode, once everything is in host memory: doff[ndocs + 1] the documents' offsets in the `total` gathered bytes, `decoded` the
// same after the device's capcode decoder with declen[ndocs] its lengths (both null: the decoder did not run; DEC_HOST: a document it left alone).
// Documents without a device-decoded form go through capcode_decode_batch - none when `raw` or the vocabulary has no capcode: the gathered bytes are
// the text then.  out_offsets[ndocs + 1] is always filled; TM_E_NOSPACE (nothing written to out) if out_cap is too small; TM_E_INTERNAL for offsets
// that are not monotone or reach beyond `total`.  *host_docs (may be null): documents decoded on the host.
int decode_assemble(const tm_vocab* v, bool raw, uint32_t ndocs, const uint64_t* doff, uint64_t total, const uint8_t* gathered, const uint8_t* decoded, const uint64_t* declen,
                    uint8_t* out, uint64_t out_cap, uint64_t* out_offsets, uint32_t* host_docs);
// tm_host.hip: tm_tokenize_pipeline over the lanes of one vocabulary or of its replicas on several devices
int tokenize_pipeline_on(const tm_vocab* const* vs, uint32_t nv, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, int raw, uint32_t encoding_length,
                         uint64_t chunk_bytes, uint32_t lanes, uint8_t* bytes_out, uint64_t bytes_cap, uint64_t* byte_offsets, uint32_t* missing,
                         uint32_t* encoding_length_used, tm_pipeline_stats* stats);
// what the device's error word (tm_batch::d_error) means for the caller: bit 0 = an entry state from which the walk never leaves its segment
// (k_resolve and the group kernels: the text / vocabulary pair does not advance, TM_E_INPUT), bit 1 = K4 met a row that K1 never wrote or a
// chain longer than its segment (an inconsistency of this library, TM_E_INTERNAL).  0 -> TM_OK.
int error_from_flag(uint32_t err);
// tm_score.hip: the error word of the dataset's last pass, once its stream has been synchronized
int score_check(tm_dataset* d);
// ... and the two halves of a byte range's pass with the entry state staying on the device (tm_multi.hip)
int score_begin_device(const tm_vocab* v, tm_dataset* d, uint64_t off, uint64_t len, int continues, hipStream_t st);
const uint8_t* score_exits_device(const tm_dataset* d);
uint8_t* score_entry_device(tm_dataset* d);
uint32_t* score_error_device(tm_dataset* d);
int score_finish_device(const tm_vocab* v, tm_dataset* d, hipStream_t st);
// tm_norm.hip
int batch_upload_raw_on(tm_batch* b, const uint8_t* raw, const uint64_t* raw_offsets, uint32_t ndocs, hipStream_t st);
// the streaming encoder's raw pieces (tm_encoder.hip): a workspace that holds what the normalizer needs and nothing of the tokenizer's
// (make_piece_workspace, tm_kernels.hip: max_bytes bounds the NORMALIZED size of a piece), every buffer a piece of max_raw bytes takes grown once
// (piece_reserve) and counted (piece_device_bytes); then per piece batch_upload_raw_on of ONE document and piece_normalize_on - tm_batch_normalize
// without the group tree, nothing on the NULL stream - after which b->nbytes normalized bytes lie in the slabs or packed in d_text, and
// launch_enc_pack (k_enc_pack) copies a range of them to `dst`, device to device
int make_piece_workspace(const tm_vocab* v, uint64_t max_bytes, hipStream_t st, tm_batch** out);
int piece_reserve(tm_batch* b, uint64_t max_raw, hipStream_t st);
uint64_t piece_device_bytes(tm_batch* b);
int piece_normalize_on(tm_batch* b, hipStream_t st);
void launch_enc_pack(const tm_batch* b, uint64_t from, uint64_t n, uint8_t* dst, hipStream_t st);
// tm_normalize.cpp
bool normalize_supported(uint32_t capcode, uint32_t norm_flag);
bool normalize_on_device(uint32_t capcode, uint32_t norm_flag);
bool normalize_origins(const uint8_t* data, size_t n, uint32_t capcode, uint32_t norm_flag, std::vector<uint8_t>& out, std::vector<uint32_t>& own);      // tm_normalize_origins

}  // namespace tmh

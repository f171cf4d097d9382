// tm_encoder.hip — the streaming encoder behind tm_encoder_* (include/tokenmonster_hip.h): ONE document that arrives in pieces (a file read
// in blocks, a socket, a decompressor) or is larger than a device workspace should be, tokenized exactly as Vocab.tokenize would tokenize
// the whole of it (go/tokenmonster.go:1017-1279).
//
// What makes that possible is the property the whole pipeline rests on (tm_kernels.hip): the walk's state at a token boundary is (offset of
// the next token start, pending forward-delete flag), one of ENT = 80 ENTRY STATES, and what a byte range does to it is an 80-entry map.  The
// scoring pass already cuts one walk into byte ranges that way (tm_score_begin / tm_score_finish, tm_multi.hip); here the ranges follow each
// other in time instead of lying side by side on several devices, and the second half of a pass emits ids (K4) instead of a histogram.
//
// The encoder owns a stream and a workspace whose text buffer holds HALO + max_piece_bytes bytes.  A pass owns the positions [0, have - HALO)
// of the buffer and may LOOK at all `have` bytes (doc_vis of k_match_branch): tokens that begin in the range are emitted by this pass even
// where they end behind it, and the last HALO bytes - the look-ahead tm_score_begin requires of a range that is followed by more text - move
// to the front of the buffer for the next pass.  Behind K4 one small kernel (k_enc_carry) takes the range's exit state out of k_doc_exits'
// map and puts it where the next pass's K3 reads its entry state, adds up the characters without a token, and moves the look-ahead: the
// state never visits the host.  tm_encoder_finish runs what is left as a range the text ENDS with (doc_vis == doc_end: the pad byte 0).
// A range that is followed by more text must be at least MIN_RANGE bytes long (tm_score_begin's rule: the entry states' offsets, < 40,
// lie inside it), so short feeds are kept on the host until HALO + MIN_RANGE bytes are there.
//
// RAW text (tm_encoder_feed_raw).  The normalizer has state of its own across a cut - capcode's inWord / rlast / rlast2 and its rewrite window,
// the order of the marks behind a starter under NFD, the byte before and behind for `collapse` and `unixlines` - but behind a line feed that
// state is the state at the start of a text (javascript/tokenmonster.js:900-1005): normalize(a + b) == normalize(a) + normalize(b) wherever a
// ends in '\n', and in any byte of FALLBACK below (tests/test_safe_cuts.py keeps that claim checked against the host normalizer).  So the encoder
// cuts the raw text itself: right behind the last '\n' of what it has, or - once max_piece_bytes are held without one - behind the last tab or
// ASCII punctuation byte; what lies behind the cut waits on the host (rhold).  A raw piece goes through the batch normalizer as ONE document of
// a normalizer workspace of the encoder's own (created by the first raw feed, sized by max_piece_bytes, on the encoder's stream), and its
// normalized bytes go from there - slabs or packed text - behind the look-ahead in the text buffer, device to device (k_enc_pack, tm_norm.hip),
// in portions of what the buffer has room for; each portion is then a normalized feed like any other.  A piece the device normalizer leaves to
// the host normalizer (full-width Latin, polytonic Greek, malformed UTF-8 ...) takes that path inside the same call (tm_encoder_host_pieces).
// Out of scope, because they need the whole document: the flags quotemarks 8 (the reference's in-place quirk counts the bytes the document has
// lost so far), trim 32 (unbounded look-ahead for trailing blanks) and leadingspace 64 (the document's start); capcode 1.  (A document that
// is in hand as a whole goes through tm_tokenize_document, tm_document.hip: serialized ids, and the pieces overlapped in slots of their own.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "tm_cuts.h"
#include "tm_pipeline.h"

using namespace tmh;

namespace {
constexpr uint64_t HALO = CUT_HALO, MIN_RANGE = CUT_MIN_RANGE;
constexpr uint64_t DEFAULT_PIECE = 32ull << 20, MAX_PIECE = 1ull << 36;
constexpr size_t O_EXITS = 0, O_ENTRY = 128, O_ACC = 192, SMALL_BYTES = 256;      // the encoder's own device words: exit map | entry state | missing, state
}  // namespace

struct tm_encoder {
  const tm_vocab* v = nullptr;
  uint64_t max_piece = 0;
  hipStream_t stream = nullptr;
  tm_batch* ws = nullptr;
  uint8_t* d_small = nullptr;
  uint64_t have = 0;                 // bytes of the document in the device text buffer: the look-ahead of the last pass + what has come since
  std::vector<uint8_t> hold;         // bytes fed since, while they are too few for a pass
  std::vector<uint32_t> pending;     // ids not yet handed to the caller (a call whose buffer was too small)
  bool failed = false;               // a pass failed: the carried state means nothing until tm_encoder_reset
  // raw text (tm_encoder_feed_raw)
  tm_batch* nws = nullptr;           // the normalizer's workspace: one raw piece = one document of it
  std::vector<uint8_t> rhold;        // raw bytes behind the last cut (no '\n' among them)
  int mode = 0;                      // what the current document is fed as: 0 nothing yet, 1 normalized, 2 raw
  uint32_t host_pieces = 0;          // raw pieces of this document (after finish: the last one) that the host normalizer took
  // the range of the last pass as the workspace holds it on the device (offsets, group tree): a stream of equal pieces uploads it once
  uint64_t r_own = ~0ull, r_have = ~0ull;
  uint32_t r_long = 0;
  uint8_t* d_exits() const { return d_small + O_EXITS; }
  uint8_t* d_entry() const { return d_small + O_ENTRY; }
  uint32_t* d_acc() const { return reinterpret_cast<uint32_t*>(d_small + O_ACC); }
};

namespace {

// one pass over the buffer: its ids are in the workspace's id buffer afterwards, *total of them; the stream has been synchronized
int enc_pass(tm_encoder* e, bool last, uint64_t* total) {
  tm_batch* b = e->ws;
  hipStream_t st = e->stream;
  const uint64_t own = last ? e->have : e->have - HALO;
  const uint64_t be[3] = {0, own, e->have};
  if (e->r_own != own || e->r_have != e->have || e->r_long != long_segs()) {
    e->r_own = ~0ull;
    int rc = small_h2d(b, b->d_offsets, be, sizeof be, st);
    if (rc != TM_OK) return rc;
    b->nseg = (own + SEG - 1) / SEG;
    if ((rc = build_groups(b, be, be + 1, 1, st)) != TM_OK) return rc;      // more than LONG_SEGS segments: the group tree (k_group_compose ...)
    e->r_own = own; e->r_have = e->have; e->r_long = long_segs();
  }
  b->vocab = e->v;
  b->d_doc_begin = b->d_offsets;
  b->d_doc_end = b->d_offsets + 1;
  b->d_doc_vis = b->d_offsets + 2;
  b->d_doc_entry = e->d_entry();
  b->text_in_slabs = false;
  units_forget(b, 3u);
  b->ndocs = 1;
  b->nbytes = e->have;
  b->nseg = (own + SEG - 1) / SEG;
  int rc = pipeline_match(b, st, nullptr);
  if (rc != TM_OK) return rc;
  if (!last) launch_doc_exits(b, e->d_exits(), st);
  if ((rc = pipeline_resolve(b, st, nullptr, 2)) != TM_OK) return rc;
  launch_enc_carry(b, last ? nullptr : e->d_exits(), e->d_entry(), e->d_acc(), own, last ? 0u : (uint32_t)HALO, st);
  { hipError_t he = hipGetLastError(); if (he != hipSuccess) return hip_fail(he, "kernel launch"); }
  if ((rc = ensure_output(b)) != TM_OK) return rc;      // (waits for the pass; the walk's dead ends come back here as TM_E_INPUT)
  *total = b->last_totals[1];
  e->have = last ? 0 : HALO;
  return TM_OK;
}

// the ids of the pass that has just run: into the caller's buffer behind what this call has already put there, or - once they no longer
// fit, or while older ids are still waiting - into `pending`
int enc_collect(tm_encoder* e, uint64_t total, uint32_t* out, uint64_t cap, uint64_t* written) {
  if (!total) return TM_OK;
  tm_batch* b = e->ws;
  uint32_t* dst;
  if (e->pending.empty() && out && *written + total <= cap) { dst = out + *written; *written += total; }
  else { const size_t old = e->pending.size(); e->pending.resize(old + total); dst = e->pending.data() + old; }
  int rc = small_d2h(b, dst, b->d_out, total * 4, e->stream);
  if (rc == TM_OK) rc = small_sync(b, e->stream); else (void)small_sync(b, e->stream);
  return rc;
}

// end of a call: everything that is final goes to the caller, or stays (in order) if the buffer is too small
int enc_hand_over(tm_encoder* e, uint32_t* out, uint64_t cap, uint64_t written, uint64_t* n_tokens) {
  const uint64_t need = written + e->pending.size();
  if (n_tokens) *n_tokens = need;
  if (e->pending.empty()) return TM_OK;
  if (need <= cap && out) {
    std::memcpy(out + written, e->pending.data(), e->pending.size() * 4);
    e->pending.clear();
    return TM_OK;
  }
  if (written) e->pending.insert(e->pending.begin(), out, out + written);
  return set_error(TM_E_NOSPACE, "tokens_cap %llu < %llu ids (the text has been consumed: call tm_encoder_feed with no text and a larger buffer)", (unsigned long long)cap, (unsigned long long)need);
}

int enc_usable(tm_encoder* e) {
  if (!e) return set_error(TM_E_INVALID, "null argument");
  if (e->failed) return set_error(TM_E_INVALID, "a pass of this encoder failed: tm_encoder_reset before the next document");
  return enter_device(e->v);
}

// bytes to the end of the device text buffer
int enc_upload(tm_encoder* e, const uint8_t* src, uint64_t n) {
  if (!n) return TM_OK;
  int rc = small_h2d(e->ws, e->ws->d_text + e->have, src, n, e->stream);
  if (rc == TM_OK) e->have += n;
  return rc;
}

// ---- raw text ------------------------------------------------------------------------------------------------------------------------
// (the bytes behind which the normalizer is in its start state, and the search for the last of them: tm_cuts.h)
// TM_OK, or why this vocabulary's raw text cannot be cut (thread-local message set)
int raw_refusal(const tm_vocab* v, bool say) {
  const uint32_t capcode = v->host.capcode, flag = v->host.norm_flag;
  const char* why = nullptr;
  if (capcode != 0 && capcode != 2) why = "capcode 1";
  else if (flag & 8u) why = "the normalization flag quotemarks (8)";
  else if (flag & 32u) why = "the normalization flag trim (32)";
  else if (flag & 64u) why = "the normalization flag leadingspace (64)";
  else if (!normalize_supported(capcode, flag)) why = "normalization flags the normalizer does not implement";
  if (!why) return TM_OK;
  return say ? set_error(TM_E_INVALID, "%s needs the whole document: normalize it first and use tm_encoder_feed", why) : TM_E_INVALID;
}

int enc_make_nws(tm_encoder* e) {
  tm_batch* nb = nullptr;
  int rc = make_piece_workspace(e->v, piece_norm_cap(e->max_piece), e->stream, &nb);
  if (rc == TM_OK) rc = piece_reserve(nb, e->max_piece, e->stream);
  if (rc != TM_OK) { tm_batch_free(nb); return rc; }
  e->nws = nb;
  return TM_OK;
}

// `total` normalized bytes behind the look-ahead in the text buffer, in portions of what the buffer has room for; put(off, take) places a
// portion at d_text + have.  A pass runs as soon as there is enough for a range that is followed by more text.
template <typename Put>
int enc_portions(tm_encoder* e, uint64_t total, uint32_t* out, uint64_t cap, uint64_t* written, Put put) {
  for (uint64_t off = 0; off < total;) {
    const uint64_t take = std::min<uint64_t>(total - off, HALO + e->max_piece - e->have);
    int rc = put(off, take);
    if (rc != TM_OK) return rc;
    e->have += take;
    off += take;
    if (e->have < HALO + MIN_RANGE) continue;           // (then off == total: the next piece goes behind it)
    uint64_t ids = 0;
    if ((rc = enc_pass(e, false, &ids)) != TM_OK || (rc = enc_collect(e, ids, out, cap, written)) != TM_OK) return rc;
  }
  return TM_OK;
}

// one raw piece [p, p + n), n > 0: a document of its own for the normalizer
int enc_raw_piece(tm_encoder* e, const uint8_t* p, uint64_t n, uint32_t* out, uint64_t cap, uint64_t* written) {
  tm_batch* nb = e->nws;
  hipStream_t st = e->stream;
  const uint64_t offs[2] = {0, n};
  int rc = batch_upload_raw_on(nb, p, offs, 1, st);
  if (rc == TM_OK) rc = piece_normalize_on(nb, st);
  if (rc == TM_OK) {
    e->host_pieces += nb->host_fallback_docs ? 1u : 0u;
    return enc_portions(e, nb->nbytes, out, cap, written, [&](uint64_t off, uint64_t take) {
      launch_enc_pack(nb, off, take, e->ws->d_text + e->have, st);
      hipError_t he = hipGetLastError();
      return he == hipSuccess ? TM_OK : hip_fail(he, "kernel launch");
    });
  }
  if (rc != TM_E_LIMIT) return rc;
  // normalized, the piece is larger than the workspace was sized for: the host normalizer, and its text uploaded in portions
  std::vector<uint8_t> norm;
  normalize_bytes(p, n, e->v->host.capcode, e->v->host.norm_flag, norm);
  e->host_pieces++;
  return enc_portions(e, norm.size(), out, cap, written, [&](uint64_t off, uint64_t take) {
    int r2 = small_h2d(e->ws, e->ws->d_text + e->have, norm.data() + off, take, st);
    if (r2 == TM_OK) r2 = small_sync(e->ws, st);       // (`norm` is pageable and goes away)
    return r2;
  });
}

}  // namespace

extern "C" {

int tm_encoder_new(const tm_vocab* v, uint64_t max_piece_bytes, tm_encoder** out) {
  if (!v || !out) return set_error(TM_E_INVALID, "null argument");
  *out = nullptr;
  if (max_piece_bytes == 0) max_piece_bytes = DEFAULT_PIECE;
  if (max_piece_bytes < MIN_RANGE || max_piece_bytes > MAX_PIECE) return set_error(TM_E_INVALID, "max_piece_bytes %llu outside [%llu, %llu]", (unsigned long long)max_piece_bytes, (unsigned long long)MIN_RANGE, (unsigned long long)MAX_PIECE);
  { int rc = enter_device(v); if (rc != TM_OK) return rc; }
  auto* e = new tm_encoder();
  e->v = v;
  e->max_piece = max_piece_bytes;
  hipError_t he;
  if ((he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) { e->stream = nullptr; tm_encoder_free(e); return hip_fail(he, "hipStreamCreate (encoder)"); }
  if ((he = hipMalloc((void**)&e->d_small, SMALL_BYTES)) != hipSuccess) { e->d_small = nullptr; tm_encoder_free(e); return hip_fail(he, "hipMalloc (encoder)"); }
  int rc = make_workspace(v, HALO + max_piece_bytes, 1, true, true, &e->ws);
  if (rc != TM_OK) { tm_encoder_free(e); return rc; }
  if ((he = hipMemsetAsync(e->d_small, 0, SMALL_BYTES, e->stream)) != hipSuccess || (he = hipStreamSynchronize(e->stream)) != hipSuccess) { tm_encoder_free(e); return hip_fail(he, "hipMemset (encoder)"); }
  *out = e;
  return TM_OK;
}

void tm_encoder_free(tm_encoder* e) {
  if (!e) return;
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  tm_batch_free(e->ws);
  tm_batch_free(e->nws);
  (void)hipFree(e->d_small);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

int tm_encoder_feed(tm_encoder* e, const uint8_t* text, uint64_t n, uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* n_tokens) {
  { int rc = enc_usable(e); if (rc != TM_OK) return rc; }
  if (n && !text) return set_error(TM_E_INVALID, "null argument");
  if (n && e->mode == 2) return set_error(TM_E_INVALID, "this document is being fed as raw text (tm_encoder_feed_raw): one document is fed either raw or normalized");
  if (n) e->mode = 1;
  uint64_t written = 0, pos = 0;
  const uint64_t room = HALO + e->max_piece;
  while (pos < n) {
    const uint64_t buffered = e->have + e->hold.size();
    const uint64_t take = std::min<uint64_t>(n - pos, room - buffered);
    if (buffered + take < HALO + MIN_RANGE) {          // too little for a range that is followed by more text (then take == n - pos: the call ends here)
      e->hold.insert(e->hold.end(), text + pos, text + pos + take);
      pos += take;
      continue;
    }
    int rc = enc_upload(e, e->hold.data(), e->hold.size());
    e->hold.clear();
    if (rc == TM_OK) rc = enc_upload(e, text + pos, take);
    pos += take;
    uint64_t total = 0;
    if (rc == TM_OK) rc = enc_pass(e, false, &total);
    if (rc == TM_OK) rc = enc_collect(e, total, tokens_out, tokens_cap, &written);
    if (rc != TM_OK) { e->failed = true; return rc; }
  }
  return enc_hand_over(e, tokens_out, tokens_cap, written, n_tokens);
}

int tm_encoder_finish(tm_encoder* e, uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* n_tokens, uint32_t* missing) {
  { int rc = enc_usable(e); if (rc != TM_OK) return rc; }
  uint64_t written = 0, total = 0;
  int rc = TM_OK;
  if (!e->rhold.empty()) {                               // what lay behind the last cut is the last raw piece
    rc = enc_raw_piece(e, e->rhold.data(), e->rhold.size(), tokens_out, tokens_cap, &written);
    e->rhold.clear();
  }
  if (rc == TM_OK) rc = enc_upload(e, e->hold.data(), e->hold.size());
  e->hold.clear();
  e->mode = 0;
  if (rc == TM_OK && e->have) {
    rc = enc_pass(e, true, &total);
    if (rc == TM_OK) rc = enc_collect(e, total, tokens_out, tokens_cap, &written);
  }
  uint32_t acc[2] = {0, 0};
  if (rc == TM_OK) rc = small_d2h(e->ws, acc, e->d_acc(), sizeof acc, e->stream);
  if (rc == TM_OK) rc = small_sync(e->ws, e->stream);
  // the encoder is ready for the next document: state 0 (k_enc_carry has seen to that), nothing counted
  if (rc == TM_OK) { hipError_t he = hipMemsetAsync(e->d_acc(), 0, 8, e->stream); if (he != hipSuccess) rc = hip_fail(he, "hipMemset (encoder)"); }
  if (rc != TM_OK) { e->failed = true; return rc; }
  if (missing) *missing = acc[0];
  return enc_hand_over(e, tokens_out, tokens_cap, written, n_tokens);
}

int tm_encoder_reset(tm_encoder* e) {
  if (!e) return set_error(TM_E_INVALID, "null argument");
  { int rc = enter_device(e->v); if (rc != TM_OK) return rc; }
  e->have = 0;
  e->hold.clear();
  e->rhold.clear();
  e->mode = 0;
  e->host_pieces = 0;
  e->pending.clear();
  e->r_own = ~0ull;
  hipError_t he;
  if ((he = hipStreamSynchronize(e->stream)) != hipSuccess) (void)hipGetLastError();      // (what a failed pass has left behind is of no interest)
  if ((he = hipMemsetAsync(e->d_small, 0, SMALL_BYTES, e->stream)) != hipSuccess || (he = hipStreamSynchronize(e->stream)) != hipSuccess) return hip_fail(he, "hipMemset (encoder)");
  e->failed = false;
  return TM_OK;
}

uint32_t tm_encoder_state(const tm_encoder* e) {
  if (!e || enter_device(e->v) != TM_OK) return 0;
  uint8_t s = 0;
  if (hipMemcpyAsync(&s, e->d_entry(), 1, hipMemcpyDeviceToHost, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return s;
}

uint64_t tm_encoder_device_bytes(const tm_encoder* e) {
  if (!e) return 0;
  return e->ws->device_bytes + SMALL_BYTES + (e->nws ? e->nws->device_bytes + piece_device_bytes(e->nws) : 0);
}

int tm_encoder_raw_supported(const tm_vocab* v) { return v && raw_refusal(v, false) == TM_OK ? 1 : 0; }

int tm_encoder_feed_raw(tm_encoder* e, const uint8_t* raw, uint64_t n, uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* n_tokens) {
  { int rc = enc_usable(e); if (rc != TM_OK) return rc; }
  { int rc = raw_refusal(e->v, true); if (rc != TM_OK) return rc; }
  if (n && !raw) return set_error(TM_E_INVALID, "null argument");
  if (n && e->mode == 1) return set_error(TM_E_INVALID, "this document is being fed as normalized text (tm_encoder_feed): one document is fed either raw or normalized");
  if (n && !e->nws) { int rc = enc_make_nws(e); if (rc != TM_OK) return rc; }        // (nothing consumed, the encoder stays usable)
  if (n && e->mode == 0) { e->mode = 2; e->host_pieces = 0; }
  uint64_t written = 0, pos = 0;
  while (pos < n) {
    // the text at hand is rhold + raw[pos, n); the cut lies in its first max_piece bytes
    const uint64_t held = e->rhold.size(), window = std::min<uint64_t>(n - pos, e->max_piece - held);
    uint64_t take = cut_behind_line_feed(raw + pos, window);      // bytes of raw[pos ..) in front of the cut
    bool cut = take > 0;
    if (!cut && held + window == e->max_piece) {        // a line of a whole piece: behind its last separator, in the new bytes or in the held ones
      take = cut_behind_fallback(raw + pos, window);
      cut = take > 0;
      if (!cut) {
        const uint64_t h = cut_behind_fallback(e->rhold.data(), held);
        if (h == 0) {
          e->failed = true;
          return set_error(TM_E_LIMIT, "a line of more than max_piece_bytes without a separator: normalize it as a whole");
        }
        // the piece ends inside the held bytes: it goes by itself, the rest stays held
        int rc = enc_raw_piece(e, e->rhold.data(), h, tokens_out, tokens_cap, &written);
        if (rc != TM_OK) { e->failed = true; return rc; }
        e->rhold.erase(e->rhold.begin(), e->rhold.begin() + (ptrdiff_t)h);
        continue;
      }
    }
    if (!cut) {                                          // no cut yet (then window == n - pos): wait for more text
      e->rhold.insert(e->rhold.end(), raw + pos, raw + pos + window);
      pos += window;
      continue;
    }
    int rc;
    if (held) {
      e->rhold.insert(e->rhold.end(), raw + pos, raw + pos + take);
      rc = enc_raw_piece(e, e->rhold.data(), e->rhold.size(), tokens_out, tokens_cap, &written);
      e->rhold.clear();
    } else rc = enc_raw_piece(e, raw + pos, take, tokens_out, tokens_cap, &written);
    pos += take;
    if (rc != TM_OK) { e->failed = true; return rc; }
  }
  return enc_hand_over(e, tokens_out, tokens_cap, written, n_tokens);
}

uint64_t tm_encoder_raw_held(const tm_encoder* e) { return e ? e->rhold.size() : 0; }
uint32_t tm_encoder_host_pieces(const tm_encoder* e) { return e ? e->host_pieces : 0; }

}  // extern "C"

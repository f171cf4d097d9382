// tm_document.hip — tm_tokenize_document (include/tokenmonster_hip.h): ONE large document that is in hand as a whole, host to host, as the
// reference's own benchmark runs it (one Vocab.tokenize of a whole file), with the transfers behind the kernels.
//
// The streaming encoder (tm_encoder.hip) runs the pieces of a document one behind the other in ONE workspace: upload, pass, wait, download.
// Here the pieces go through `slots` workspaces of their own.  What couples two pieces is small: the walk's state at the cut (one of 80 entry
// states) and, for raw text, the 128 bytes of look-ahead.  The match kernel (K1, four fifths of a pass) needs neither the state nor anything of
// the piece before - so K1 of piece k + 1 runs while piece k resolves, emits, packs its ids and downloads them, and while piece k + 2 uploads.
//
//   upload stream        text of piece k -> slot k % slots                                                   (one for the call)
//   slot's own stream    [raw: normalizer pass] | K0 K1, k_doc_exits | wait: chain of k - 1 | k_doc_chain | K3, scan, K4 | pack, verdict
//   download stream      wait: piece k computed | ids -> bytes_out + (ids so far) * enc                      (one for the call)
//
// k_doc_chain (tm_kernels.hip) takes the document's state out of a cell the call owns, puts it where this slot's K3 looks, replaces it by the
// exit state of this piece (k_doc_exits' map), and - raw text - copies the look-ahead to the front of the NEXT slot's text.  The chain kernels
// wait for each other through events, each recorded before the wait on it is enqueued: no stream ever waits for something a later call records.
// The host reads a piece's verdict (status bits, id count, characters without a token) from a page-locked block its last kernel writes, and
// then - in order, so that it knows how many ids lie in front - enqueues the download.  One thread: the caller's.
//
// Normalized text: piece k is text[k * P, (k + 1) * P + 128), straight from the caller's buffer (the look-ahead is uploaded twice).  Raw text is
// cut behind line feeds (tm_cuts.h), every raw piece is normalized on the device as one document of the slot's normalizer workspace, and a
// pass is the look-ahead carried from the slot before + those normalized bytes; the host waits for a piece's normalizer pass only (it needs the
// length for the group tree), which runs beside the walk of the piece before.  A pass that is too short to own anything rolls whole into the next.
// Vocabularies whose normalizer needs the whole document (quotemarks, trim, leadingspace), and a text that has no byte to cut behind, are
// normalized once on the host and take the normalized path.
//
// Slots come from a grow-only pool on the vocabulary, in sets shaped by (piece_bytes, raw): a second call of the same shape allocates nothing,
// concurrent calls take different sets (at most MAX_SETS, an idle one of another shape making room for a new shape; further callers wait).  Nothing runs on the NULL stream.
// On a failure - a HIP error, the walk's dead end (TM_E_INPUT) - nothing more is issued and every stream the call touched is drained before
// the set goes back; later pieces that were already enqueued behind a dead end emit nothing (k_doc_chain zeroes their control words).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "tm_cuts.h"
#include "tm_pipeline.h"

using namespace tmh;

namespace {
constexpr uint64_t HALO = CUT_HALO, MIN_RANGE = CUT_MIN_RANGE;
constexpr uint64_t DEFAULT_PIECE = 32ull << 20, MAX_PIECE = 1ull << 36;
constexpr uint32_t DEFAULT_SLOTS = 3, MIN_SLOTS = 2, MAX_SLOTS = 8;
constexpr size_t MAX_SETS = 4;
constexpr size_t O_EXITS = 0, O_ENTRY = 128, O_CTL = 192, SMALL_BYTES = 256;      // a slot's own device words: exit map | entry state | control words
constexpr size_t CELL_BYTES = 64;                                                 // the call's cell: entry state, -, error word

struct DocSlot {
  tm_batch* ws = nullptr;            // the tokenizer's workspace: text of HALO + piece bytes (raw: look-ahead + the normalized size of a piece)
  tm_batch* nws = nullptr;           // raw text: the normalizer's workspace, one raw piece = one document of it
  hipStream_t comp = nullptr;
  uint8_t* d_small = nullptr;
  uint8_t* d_bytes = nullptr; uint64_t d_bytes_cap = 0;      // the packed ids (two or three bytes each; four-byte ids are the workspace's own)
  uint8_t* h_pin = nullptr;                                  // page-locked: the verdict (8 words) | 8 words nobody reads
  uint8_t* h_in = nullptr; uint64_t h_in_cap = 0;            // page-locked staging of pageable input / output, made by the first call that needs it
  uint8_t* h_out = nullptr; uint64_t h_out_cap = 0;
  hipEvent_t up_done = nullptr, chain_done = nullptr, comp_done = nullptr, free_ev = nullptr;
  // the range of the last pass as the workspace holds it (offsets, group tree): equal pieces upload it once
  uint64_t r_own = ~0ull, r_have = ~0ull;
  uint32_t r_long = 0;
  // the pass in flight
  bool active = false, computes = false, harvested = false, staged = false;
  uint64_t base = 0, ntok = 0;
  const uint8_t* ids_at = nullptr;
  uint8_t* d_exits() const { return d_small + O_EXITS; }
  uint8_t* d_entry() const { return d_small + O_ENTRY; }
  uint64_t* d_ctl() const { return reinterpret_cast<uint64_t*>(d_small + O_CTL); }
  uint64_t* h_status() const { return reinterpret_cast<uint64_t*>(h_pin); }
  uint64_t* h_scratch() const { return reinterpret_cast<uint64_t*>(h_pin + 64); }
};

struct DocSet {
  uint64_t piece = 0;
  bool raw = false, busy = false;
  hipStream_t up = nullptr, down = nullptr;
  uint32_t* d_cell = nullptr;
  std::vector<DocSlot> slots;
};

void slot_destroy(DocSlot& s) {
  if (s.comp) (void)hipStreamSynchronize(s.comp);
  tm_batch_free(s.ws);
  tm_batch_free(s.nws);
  (void)hipFree(s.d_small);
  (void)hipFree(s.d_bytes);
  (void)hipHostFree(s.h_pin); (void)hipHostFree(s.h_in); (void)hipHostFree(s.h_out);
  for (hipEvent_t ev : {s.up_done, s.chain_done, s.comp_done, s.free_ev}) if (ev) (void)hipEventDestroy(ev);
  if (s.comp) (void)hipStreamDestroy(s.comp);
  s = DocSlot();
}
void set_destroy(DocSet* d) {
  if (!d) return;
  for (DocSlot& s : d->slots) slot_destroy(s);
  (void)hipFree(d->d_cell);
  if (d->up) (void)hipStreamDestroy(d->up);
  if (d->down) (void)hipStreamDestroy(d->down);
  delete d;
}

// the most text a slot's tokenizer workspace holds
uint64_t slot_text_bytes(uint64_t piece, bool raw) { return raw ? HALO + MIN_RANGE + piece_norm_cap(piece) : HALO + piece; }

int slot_create(DocSlot& s, const tm_vocab* v, uint64_t piece, bool raw) {
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&s.comp, hipStreamNonBlocking)) != hipSuccess) { s.comp = nullptr; return hip_fail(e, "hipStreamCreate (document slot)"); }
  for (hipEvent_t* ev : {&s.up_done, &s.chain_done, &s.comp_done, &s.free_ev})
    if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) { *ev = nullptr; return hip_fail(e, "hipEventCreate (document slot)"); }
  if ((e = hipMalloc((void**)&s.d_small, SMALL_BYTES)) != hipSuccess) { s.d_small = nullptr; return hip_fail(e, "hipMalloc (document slot)"); }
  if ((e = hipHostMalloc((void**)&s.h_pin, 128, hipHostMallocDefault)) != hipSuccess) { s.h_pin = nullptr; return hip_fail(e, "hipHostMalloc (document slot)"); }
  std::memset(s.h_pin, 0, 128);
  int rc = make_workspace(v, slot_text_bytes(piece, raw), 1, true, true, &s.ws);
  if (rc != TM_OK) return rc;
  s.d_bytes_cap = s.ws->out_cap * 3 + 64;
  if ((e = hipMalloc((void**)&s.d_bytes, s.d_bytes_cap)) != hipSuccess) { s.d_bytes = nullptr; s.d_bytes_cap = 0; return hip_fail(e, "hipMalloc (document ids)"); }
  if ((e = hipMemsetAsync(s.d_small, 0, SMALL_BYTES, s.comp)) != hipSuccess) return hip_fail(e, "hipMemset (document slot)");
  if (raw) {
    if ((rc = make_piece_workspace(v, piece_norm_cap(piece), s.comp, &s.nws)) != TM_OK) return rc;
    if ((rc = piece_reserve(s.nws, piece, s.comp)) != TM_OK) return rc;
  }
  if ((e = hipStreamSynchronize(s.comp)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize (document slot)");
  return TM_OK;
}

uint64_t slot_device_bytes(const DocSlot& s) {
  return s.ws->device_bytes + SMALL_BYTES + s.d_bytes_cap + (s.nws ? s.nws->device_bytes + piece_device_bytes(s.nws) : 0);
}

// (exact sizes: a slot's buffers are sized for its piece once)
int stage_grow(uint8_t** buf, uint64_t* cap, uint64_t bytes) { return grow_pinned(buf, cap, bytes, bytes, "document staging (pinned)"); }

}  // namespace

namespace tmh {
struct DocPool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<DocSet*> sets;
};
void doc_pool_destroy(DocPool* p) {
  if (!p) return;
  for (DocSet* d : p->sets) set_destroy(d);
  delete p;
}
}  // namespace tmh

namespace {

DocPool* doc_pool_of(const tm_vocab* v) {
  static std::mutex create_mu;
  std::lock_guard<std::mutex> g(create_mu);
  if (!v->doc_pool) v->doc_pool = new DocPool();
  return v->doc_pool;
}

// borrow a set of this shape with at least `nslots` slots (blocks while MAX_SETS calls are running); idle sets of another shape make room
int set_acquire(const tm_vocab* v, uint64_t piece, bool raw, uint32_t nslots, DocSet** out) {
  DocPool* p = doc_pool_of(v);
  DocSet* d = nullptr;
  {
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
      for (DocSet* q : p->sets) if (!q->busy && q->piece == piece && q->raw == raw) { d = q; break; }
      if (d) break;
      if (p->sets.size() >= MAX_SETS)      // (full: an idle set of another shape makes room)
        for (size_t i = 0; i < p->sets.size(); i++)
          if (!p->sets[i]->busy) { trace_grow("document slots (another shape)", 0); set_destroy(p->sets[i]); p->sets.erase(p->sets.begin() + (ptrdiff_t)i); break; }
      if (p->sets.size() < MAX_SETS) { d = new DocSet(); d->piece = piece; d->raw = raw; p->sets.push_back(d); break; }
      p->cv.wait(lk);
    }
    d->busy = true;
  }
  // (the set is this call's alone from here on: what it lacks is made outside the lock)
  int rc = TM_OK;
  hipError_t e = hipSuccess;
  if (!d->up && (e = hipStreamCreateWithFlags(&d->up, hipStreamNonBlocking)) != hipSuccess) { d->up = nullptr; rc = hip_fail(e, "hipStreamCreate (document)"); }
  if (rc == TM_OK && !d->down && (e = hipStreamCreateWithFlags(&d->down, hipStreamNonBlocking)) != hipSuccess) { d->down = nullptr; rc = hip_fail(e, "hipStreamCreate (document)"); }
  if (rc == TM_OK && !d->d_cell && (e = hipMalloc((void**)&d->d_cell, CELL_BYTES)) != hipSuccess) { d->d_cell = nullptr; rc = hip_fail(e, "hipMalloc (document)"); }
  while (rc == TM_OK && d->slots.size() < nslots) {
    DocSlot s;
    rc = slot_create(s, v, piece, raw);
    if (rc != TM_OK) { const std::string msg = last_error(); slot_destroy(s); set_error(rc, "%s", msg.c_str()); break; }
    d->slots.push_back(s);
  }
  if (rc != TM_OK) {
    { std::lock_guard<std::mutex> g(p->mu); d->busy = false; }
    p->cv.notify_one();
    return rc;
  }
  *out = d;
  return TM_OK;
}
void set_release(const tm_vocab* v, DocSet* d) {
  DocPool* p = v->doc_pool;
  { std::lock_guard<std::mutex> g(p->mu); d->busy = false; }
  p->cv.notify_one();
}

struct DocCall {
  const tm_vocab* v;
  DocSet* set;
  uint32_t nslots, enc;
  uint8_t* bytes_out;
  uint64_t bytes_cap;
  bool in_pinned, out_pinned;
  uint64_t ids = 0, missing = 0, passes = 0, issued = 0;      // ids of the passes harvested so far; passes issued
  bool fits = true;                                           // the ids harvested so far have all gone to bytes_out
  DocSlot& slot(uint64_t pass) const { return set->slots[pass % nslots]; }
};

int hip_rc(hipError_t e, const char* what) { return e == hipSuccess ? TM_OK : hip_fail(e, what); }

// the verdict of the pass in the slot, and its download enqueued behind those of the passes before it
int harvest(DocCall& c, DocSlot& s) {
  if (!s.active || s.harvested) return TM_OK;
  s.harvested = true;
  if (!s.computes) return TM_OK;
  tm_batch* b = s.ws;
  hipError_t e = wait_verdict(s.h_status(), s.comp_done);      // (the word that the pass's last kernel writes, watched as the ring's finisher watches its chunks')
  if (e != hipSuccess) return hip_fail(e, "document piece");
  const uint64_t st = s.h_status()[0];
  if (st == ~0ull) return set_error(TM_E_INTERNAL, "a piece of the document ended without its verdict");
  uint64_t ntok = s.h_status()[1], missing = s.h_status()[2];
  if (st & RING_ERROR) { const int rc = error_from_flag((uint32_t)s.h_status()[4]); return rc != TM_OK ? rc : set_error(TM_E_INTERNAL, "a piece of the document failed without an error word"); }
  if (st & RING_OUT_CAP) {
    // more ids than the slot's buffers hold (over half an id per byte): the emit stage again into a larger id buffer, the ids packed behind it
    int rc = doc_redo_emit(b, s.comp, s.d_ctl());
    if (rc != TM_OK) return rc;
    ntok = b->last_totals[1];
    if (c.enc != 4) {
      if ((rc = grow_device(&s.d_bytes, &s.d_bytes_cap, ntok * 3 + 64, b->out_cap * 3 + 64, "document ids")) != TM_OK) return rc;
      launch_serialize(b->d_out, ntok, c.enc, s.d_bytes, s.comp);
      s.ids_at = s.d_bytes;
    } else s.ids_at = reinterpret_cast<const uint8_t*>(b->d_out);
    uint32_t m = 0;
    if ((rc = small_d2h(b, &m, b->d_doc_missing, 4, s.comp)) != TM_OK || (rc = small_sync(b, s.comp)) != TM_OK) return rc;
    missing = m;
    if ((e = hipEventRecord(s.comp_done, s.comp)) != hipSuccess) return hip_fail(e, "hipEventRecord");
  } else if (st != 0) return set_error(TM_E_INTERNAL, "a piece of the document ended with status %llu", (unsigned long long)st);
  s.base = c.ids;
  s.ntok = ntok;
  c.ids += ntok;
  c.missing += missing;
  const uint64_t nb = ntok * c.enc;
  if (c.fits && c.bytes_out && (s.base + ntok) * c.enc <= c.bytes_cap) {
    if (nb) {
      uint8_t* dst = c.bytes_out + s.base * c.enc;
      if (!c.out_pinned) {
        const int rc = stage_grow(&s.h_out, &s.h_out_cap, std::max<uint64_t>(nb, b->out_cap * 4));
        if (rc != TM_OK) return rc;
        dst = s.h_out;
        s.staged = true;
      }
      if ((e = hipStreamWaitEvent(c.set->down, s.comp_done, 0)) != hipSuccess || (e = hipMemcpyAsync(dst, s.ids_at, nb, hipMemcpyDeviceToHost, c.set->down)) != hipSuccess ||
          (e = hipEventRecord(s.free_ev, c.set->down)) != hipSuccess)
        return hip_fail(e, "document download");
    }
  } else c.fits = false;
  return TM_OK;
}

// the slot's pass is over: its ids are in the caller's buffer, the slot may take the next pass
int retire(DocCall& c, DocSlot& s) {
  if (!s.active) return TM_OK;
  int rc = harvest(c, s);
  if (rc != TM_OK) return rc;
  const hipError_t e = hipEventSynchronize(s.free_ev);
  if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize (document piece)");
  if (s.staged) std::memcpy(c.bytes_out + s.base * c.enc, s.h_out, s.ntok * c.enc);
  s.active = s.staged = false;
  return TM_OK;
}

// A pass over the `have` bytes in the slot's text buffer, of which it owns the first `own` (own == 0: too short to own anything, the bytes
// roll into the next pass).  keep: the bytes from own on (own == 0: all) go to the front of the next slot's text.  On the slot's own stream,
// behind whatever has put the text there.
int enqueue_pass(DocCall& c, uint64_t pass, uint64_t own, uint64_t have, uint32_t keep, bool wait_upload) {
  DocSlot& s = c.slot(pass);
  DocSlot* prev = pass > 0 ? &c.slot(pass - 1) : nullptr;
  uint8_t* next_text = keep ? c.slot(pass + 1).ws->d_text : nullptr;
  tm_batch* b = s.ws;
  hipStream_t st = s.comp;
  hipError_t e = hipSuccess;
  s.active = true; s.harvested = s.staged = false; s.computes = own > 0;
  s.base = s.ntok = 0;
  c.issued = pass + 1;
  if (!s.computes) {
    if (prev && (e = hipStreamWaitEvent(st, prev->chain_done, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    launch_doc_chain(b, c.set->d_cell, nullptr, s.d_entry(), s.d_ctl(), 0, 0, keep, next_text, st);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(s.chain_done, st)) != hipSuccess || (e = hipEventRecord(s.free_ev, st)) != hipSuccess) return hip_fail(e, "document chain");
    return TM_OK;
  }
  const uint64_t be[3] = {0, own, have};
  int rc;
  if (s.r_own != own || s.r_have != have || s.r_long != long_segs()) {
    s.r_own = ~0ull;
    if ((rc = small_h2d(b, b->d_offsets, be, sizeof be, st)) != TM_OK) return rc;
    b->nseg = (own + SEG - 1) / SEG;
    if ((rc = build_groups(b, be, be + 1, 1, st)) != TM_OK) return rc;      // more than LONG_SEGS segments: the group tree
    s.r_own = own; s.r_have = have; s.r_long = long_segs();
  }
  // (behind the group tree, which waits for the stream where it has to be built anew: not for the upload as well)
  if (wait_upload && (e = hipStreamWaitEvent(st, s.up_done, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
  b->vocab = c.v;
  b->d_doc_begin = b->d_offsets;
  b->d_doc_end = b->d_offsets + 1;
  b->d_doc_vis = b->d_offsets + 2;
  b->d_doc_entry = s.d_entry();
  b->d_ctl = nullptr;
  b->text_in_slabs = false;
  b->has_output = false;
  units_forget(b, 3u);
  b->ndocs = 1;
  b->nbytes = have;
  b->nseg = (own + SEG - 1) / SEG;
  // (raw text: the front of this slot's text is the look-ahead the chain kernel of the pass before puts there - K1 waits for it; normalized
  // text has all of its bytes from the upload, and only the chain kernel waits)
  if (prev && c.set->raw && (e = hipStreamWaitEvent(st, prev->chain_done, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
  if ((rc = pipeline_match(b, st, nullptr)) != TM_OK) return rc;
  launch_doc_exits(b, s.d_exits(), st);
  if (prev && !c.set->raw && (e = hipStreamWaitEvent(st, prev->chain_done, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
  launch_doc_chain(b, c.set->d_cell, s.d_exits(), s.d_entry(), s.d_ctl(), b->nseg, own, keep, next_text, st);
  if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(s.chain_done, st)) != hipSuccess) return hip_fail(e, "document chain");
  __atomic_store_n(s.h_status(), ~0ull, __ATOMIC_RELEASE);
  if ((rc = doc_enqueue_resolve(b, st, c.enc, s.d_ctl(), s.d_bytes, s.d_bytes_cap, s.h_status(), s.h_scratch(), &s.ids_at)) != TM_OK) return rc;
  // (free_ev: re-recorded behind the download when there is one; a pass whose ids go nowhere is over when it is computed)
  if ((e = hipEventRecord(s.comp_done, st)) != hipSuccess || (e = hipEventRecord(s.free_ev, st)) != hipSuccess) return hip_fail(e, "hipEventRecord");
  return TM_OK;
}

// behind the pass that has just been issued: the verdict of the oldest pass that may still be running beside it
int harvest_behind(DocCall& c, uint64_t pass) {
  return pass + 1 >= c.nslots ? harvest(c, c.slot(pass + 1 - c.nslots)) : TM_OK;
}

int run_normalized(DocCall& c, const uint8_t* text, uint64_t n, uint64_t piece) {
  const uint64_t count = norm_piece_count(n, piece);
  hipError_t e;
  int rc;
  for (uint64_t k = 0; k < count; k++) {
    DocSlot& s = c.slot(k);
    if ((rc = retire(c, s)) != TM_OK) return rc;
    const PieceRange r = norm_piece(n, piece, count, k);
    const uint64_t have = r.vis_end - r.begin, own = r.own_end - r.begin;
    const uint8_t* src = text + r.begin;
    if (!c.in_pinned) {
      if ((rc = stage_grow(&s.h_in, &s.h_in_cap, std::max<uint64_t>(have, std::min<uint64_t>(n, piece + HALO)))) != TM_OK) return rc;
      std::memcpy(s.h_in, src, have);
      src = s.h_in;
    }
    c.issued = k + 1;      // (from here on the call has work on the device for this pass)
    s.active = true; s.computes = false; s.harvested = true; s.staged = false;
    if ((e = hipMemcpyAsync(s.ws->d_text, src, have, hipMemcpyHostToDevice, c.set->up)) != hipSuccess || (e = hipEventRecord(s.up_done, c.set->up)) != hipSuccess ||
        (e = hipEventRecord(s.free_ev, c.set->up)) != hipSuccess)
      return hip_fail(e, "document upload");
    if ((rc = enqueue_pass(c, k, own, have, 0, true)) != TM_OK) return rc;
    if ((rc = harvest_behind(c, k)) != TM_OK) return rc;
  }
  c.passes = count;
  return TM_OK;
}

int run_raw(DocCall& c, const uint8_t* raw, const std::vector<uint64_t>& cuts, tm_document_stats* stats) {
  const uint64_t room = c.set->slots[0].ws->max_bytes;
  uint64_t pass = 0, carry = 0, norm_total = 0;
  uint32_t host_pieces = 0;
  hipError_t e;
  int rc;
  std::vector<uint8_t> norm;
  for (size_t r = 0; r + 1 < cuts.size(); r++) {
    const bool last_piece = r + 2 == cuts.size();
    const uint8_t* p = raw + cuts[r];
    const uint64_t len = cuts[r + 1] - cuts[r];
    DocSlot* s = &c.slot(pass);
    if ((rc = retire(c, *s)) != TM_OK) return rc;
    // the raw piece: one document of the slot's normalizer workspace, uploaded on the upload stream, normalized on the slot's own
    tm_batch* nb = s->nws;
    const uint8_t* src = p;
    if (!c.in_pinned) {
      if ((rc = stage_grow(&s->h_in, &s->h_in_cap, std::max<uint64_t>(len, c.set->piece))) != TM_OK) return rc;
      std::memcpy(s->h_in, p, len);
      src = s->h_in;
    }
    const uint64_t offs[2] = {0, len};
    c.issued = pass + 1;
    s->active = true; s->computes = false; s->harvested = true; s->staged = false;
    if ((rc = batch_upload_raw_on(nb, src, offs, 1, c.set->up)) != TM_OK) return rc;
    if ((e = hipEventRecord(s->up_done, c.set->up)) != hipSuccess || (e = hipEventRecord(s->free_ev, c.set->up)) != hipSuccess ||
        (e = hipStreamWaitEvent(s->comp, s->up_done, 0)) != hipSuccess)
      return hip_fail(e, "document upload");
    rc = piece_normalize_on(nb, s->comp);      // (waits for this piece's normalizer pass - the walk of the piece before runs on its own stream)
    bool on_host = false;
    uint64_t total = 0;
    if (rc == TM_OK) { total = nb->nbytes; host_pieces += nb->host_fallback_docs ? 1u : 0u; }
    else if (rc == TM_E_LIMIT) {
      // normalized, the piece is larger than the workspace was sized for: the host normalizer, and its text uploaded in portions
      normalize_bytes(p, len, c.v->host.capcode, c.v->host.norm_flag, norm);
      total = norm.size();
      host_pieces++;
      on_host = true;
    } else return rc;
    norm_total += total;
    uint64_t off = 0;
    do {
      if (off > 0) { s = &c.slot(pass); if ((rc = retire(c, *s)) != TM_OK) return rc; }
      const uint64_t take = std::min<uint64_t>(total - off, room - carry);
      if (take && !on_host) launch_enc_pack(nb, off, take, s->ws->d_text + carry, s->comp);
      else if (take) {
        // (`norm` is pageable and is written again by a later piece: the copy is waited for)
        if ((e = hipMemcpyAsync(s->ws->d_text + carry, norm.data() + off, take, hipMemcpyHostToDevice, s->comp)) != hipSuccess || (e = hipStreamSynchronize(s->comp)) != hipSuccess)
          return hip_fail(e, "document upload (host normalizer)");
      }
      if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "kernel launch");
      off += take;
      const uint64_t have = carry + take;
      const bool last = last_piece && off == total;
      if (last) {
        if (have) { if ((rc = enqueue_pass(c, pass, have, have, 0, false)) != TM_OK) return rc; }
        else { s->active = false; break; }      // (nothing is left: the piece before has carried nothing over)
        carry = 0;
      } else if (have < HALO + MIN_RANGE) {
        if ((rc = enqueue_pass(c, pass, 0, have, (uint32_t)have, false)) != TM_OK) return rc;
        carry = have;
      } else {
        if ((rc = enqueue_pass(c, pass, have - HALO, have, (uint32_t)HALO, false)) != TM_OK) return rc;
        carry = HALO;
      }
      if ((rc = harvest_behind(c, pass)) != TM_OK) return rc;
      pass++;
    } while (off < total);
  }
  c.passes = pass;
  stats->host_pieces = host_pieces;
  stats->normalized_bytes = norm_total;
  return TM_OK;
}

}  // namespace

extern "C" {

int tm_tokenize_document(const tm_vocab* v, const uint8_t* text, uint64_t n, int raw, uint32_t encoding_length, uint64_t piece_bytes, uint32_t slots,
                         uint8_t* bytes_out, uint64_t bytes_cap, uint64_t* bytes_needed, uint32_t* missing, uint32_t* encoding_length_used, tm_document_stats* stats) {
  if (!v || (n && !text) || !bytes_needed) return set_error(TM_E_INVALID, "null argument");
  *bytes_needed = 0;
  if (encoding_length == 0) encoding_length = v->host.n_ids <= 65536 ? 2 : 3;
  if (encoding_length < 2 || encoding_length > 4) return set_error(TM_E_INVALID, "Invalid encoding length");
  if (piece_bytes == 0) piece_bytes = DEFAULT_PIECE;
  if (piece_bytes < MIN_RANGE || piece_bytes > MAX_PIECE)
    return set_error(TM_E_INVALID, "piece_bytes %llu outside [%llu, %llu]", (unsigned long long)piece_bytes, (unsigned long long)MIN_RANGE, (unsigned long long)MAX_PIECE);
  if (slots == 0) slots = DEFAULT_SLOTS;
  if (slots < MIN_SLOTS || slots > MAX_SLOTS) return set_error(TM_E_INVALID, "slots %u outside [%u, %u]", slots, MIN_SLOTS, MAX_SLOTS);
  const uint32_t capcode = v->host.capcode, flag = v->host.norm_flag;
  if (raw && capcode != 0 && capcode != 2) return set_error(TM_E_INVALID, "raw text of a capcode 1 vocabulary: no normalizer for it, normalize the text first");
  if (raw && !normalize_supported(capcode, flag)) return set_error(TM_E_INVALID, "raw text: normalization flags the normalizer does not implement");
  if (encoding_length_used) *encoding_length_used = encoding_length;
  if (missing) *missing = 0;
  tm_document_stats local{};
  tm_document_stats& stt = stats ? *stats : local;
  stt = tm_document_stats{};
  stt.slots = slots;
  { int rc = enter_device(v); if (rc != TM_OK) return rc; }
  stt.input_pinned = is_pinned(text);
  stt.output_pinned = is_pinned(bytes_out);
  if (!raw) stt.normalized_bytes = n;

  // raw text: where it is cut - or, where it cannot be (flags that need the whole document, a stretch without a byte to cut behind), the whole
  // of it through the host normalizer once
  std::vector<uint64_t> cuts;
  std::vector<uint8_t> whole;
  bool run_as_raw = raw != 0;
  if (raw) {
    bool cut_ok = !(flag & (8u | 32u | 64u));
    if (cut_ok) {
      cuts.push_back(0);
      for (uint64_t pos = 0; pos < n;) {
        const uint64_t take = raw_piece_length(text + pos, n - pos, piece_bytes);
        if (!take) { cut_ok = false; break; }
        pos += take;
        cuts.push_back(pos);
      }
    }
    if (!cut_ok) {
      normalize_bytes(text, n, capcode, flag, whole);
      text = whole.data();
      n = whole.size();
      run_as_raw = false;
      stt.host_normalized = 1;
      stt.normalized_bytes = n;
    }
  }
  const bool in_pinned = stt.host_normalized ? false : stt.input_pinned != 0;

  DocSet* set = nullptr;
  { int rc = set_acquire(v, piece_bytes, run_as_raw, slots, &set); if (rc != TM_OK) return rc; }
  DocCall c{v, set, slots, encoding_length, bytes_out, bytes_cap, in_pinned, stt.output_pinned != 0};
  for (uint32_t i = 0; i < slots; i++) stt.device_bytes += slot_device_bytes(set->slots[i]);
  stt.device_bytes += CELL_BYTES;

  int rc = TM_OK;
  if (n) {
    // the document starts in state 0 with nothing wrong: on the first slot's stream, in front of the first chain kernel
    rc = hip_rc(hipMemsetAsync(set->d_cell, 0, CELL_BYTES, set->slots[0].comp), "hipMemset (document)");
    if (rc == TM_OK) rc = run_as_raw ? run_raw(c, text, cuts, &stt) : run_normalized(c, text, n, piece_bytes);
    // what is still in flight, oldest first
    for (uint64_t k = c.issued > slots ? c.issued - slots : 0; rc == TM_OK && k < c.issued; k++) rc = harvest(c, c.slot(k));
    for (uint64_t k = c.issued > slots ? c.issued - slots : 0; rc == TM_OK && k < c.issued; k++) rc = retire(c, c.slot(k));
    if (rc != TM_OK) {
      // nothing more is issued; whatever is in flight - uploads that read the caller's text, kernels in the slots, downloads into the caller's
      // buffer - ends before the call returns and the set goes back
      const std::string msg = last_error();
      (void)hipStreamSynchronize(set->up);
      for (uint32_t i = 0; i < slots; i++) {
        DocSlot& s = set->slots[i];
        if (s.ws) (void)small_sync(s.ws, s.comp); else (void)hipStreamSynchronize(s.comp);
        s.r_own = ~0ull;
      }
      (void)hipStreamSynchronize(set->down);
      (void)hipGetLastError();
      set_error(rc, "%s", msg.c_str());
    }
    for (uint32_t i = 0; i < slots; i++) { DocSlot& s = set->slots[i]; s.active = s.staged = false; }
  }
  set_release(v, set);
  if (rc != TM_OK) return rc;
  stt.pieces = (uint32_t)std::min<uint64_t>(c.passes, 0xFFFFFFFFull);
  *bytes_needed = c.ids * encoding_length;
  if (missing) *missing = (uint32_t)std::min<uint64_t>(c.missing, 0xFFFFFFFFull);
  if (!c.fits || (c.ids && !bytes_out) || *bytes_needed > bytes_cap)
    return set_error(TM_E_NOSPACE, "bytes_cap %llu < %llu required", (unsigned long long)bytes_cap, (unsigned long long)*bytes_needed);
  return TM_OK;
}

}  // extern "C"

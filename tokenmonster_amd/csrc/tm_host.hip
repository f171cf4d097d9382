// tm_host.hip — the host-buffer entry points of the C ABI (include/tokenmonster_hip.h): what a Go caller binds.
//
// The reference fans documents out over goroutines, each calling Vocab.tokenize (training/tokenmonsterserver.go:363-378,
// :773-787), and is reentrant: many callers tokenize at once on one read-only Vocab.  Here every call borrows a LANE of the
// vocabulary: a HIP stream + a grow-only device workspace (tm_batch) + grow-only pinned staging.  Steady state does no
// hipMalloc / hipFree and never touches the NULL stream; concurrent callers (cgo calls run on distinct OS threads) take
// different lanes and overlap on the device.  tm_tokenize_pipeline is the large-batch form: the corpus is cut into chunks that
// run H2D | normalize + tokenize (+ serialize) | D2H on several lanes at once, so that PCIe moves chunk k+1 in and chunk k-1 out
// while chunk k computes — the host-to-host number of bench.py.
//
// How the file is laid out.  A lane goes back to the pool with nothing in flight on its stream and nothing pending in its workspace's mailbox
// (small_d2h's destinations are the caller's buffers and stack locals); that rule is kept in three places, once each:
//   one_shot       the body of tm_tokenize_batch, _spans, _raw_spans and _serialized: lane, run, offsets and missing counts, the span pass, the
//                  ids, small_sync on every path, lane back (tm_count_batch reads other arrays and keeps its own few lines);
//   chunk_deliver  the second half of a chunk of tm_tokenize_pipeline on a lane - its place in the chain of counts, offsets, packed ids out,
//                  one wait - for the lanes' worker loop (pipeline_lanes) and for the ring's exact path (chunk_exact), each of which waits
//                  for the lane's stream itself when it fails;
//   tm_decode_batch, whose host part (which documents the device left to the host decoder, the two sources interleaved) is decode_assemble
//                  of tm_decode.hip, shared with tm_batch_decoded_download.
// PipeCall::chunk(k) is the one place that turns a chunk number into documents, bytes and chunk-relative offsets.  Buffers grow through
// grow_device / grow_pinned / grow_workspace (tm_pipeline.h); this file only says how much headroom a lane or a ring slot takes.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "tm_chunks.h"
#include "tm_pipeline.h"

#ifndef TM_EMU
// The HIP runtime spreads the streams of a process over GPU_MAX_HW_QUEUES hardware queues - four unless the environment says otherwise - and
// two streams that share one run their commands in the order they were submitted in: a copy stream's 32 MiB transfer in front of a compute
// stream's kernels holds those back for its 0.6 ms.  The ring (below) has four streams of its own beside the lanes' and the caller's; with
// four queues it ran 1 GiB in 36.2 ms, with eight in 28.1 (profiles/r06_h2h.txt; the lanes' form 34.3 -> 31.9 with sixteen).  So the library
// asks for eight when it is loaded - before the runtime reads the variable at its first call - unless the environment has set it already.
__attribute__((constructor)) static void tm_runtime_defaults() { (void)setenv("GPU_MAX_HW_QUEUES", "8", 0); }
#endif

namespace tmh {

// a tuning variable of the environment: its value where it lies in [lo, hi], the default where it does not or is not set (a call site that
// reads it once keeps it in a static)
static int env_int(const char* name, int lo, int hi, int dflt) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  return e && v >= lo && v <= hi ? v : dflt;
}

struct Lane {
  hipStream_t stream = nullptr;
  tm_batch* ws = nullptr;
  uint8_t* h_stage = nullptr;     // pinned staging (pageable input of a one-shot call, pageable output), grow-only
  uint64_t h_cap = 0;
  uint8_t* h_stage_in = nullptr;  // pinned staging of the pipeline's pageable input (filled for the next chunk while h_stage still holds output)
  uint64_t h_in_cap = 0;
  hipStream_t up_stream = nullptr;   // tm_tokenize_pipeline: the next chunk's raw text is uploaded here while the current chunk computes
  hipEvent_t up_done = nullptr;
  uint8_t* d_bytes = nullptr;     // serialized ids on the device, grow-only
  uint64_t d_bytes_cap = 0;
  uint8_t* d_dec_a = nullptr;     // tm_decode_batch: ids, lengths, offsets (grow-only) ...
  uint64_t d_dec_a_cap = 0;
  uint8_t* d_dec_b = nullptr;     // ... and the decoded bytes, before and after capcode decoding (grow-only)
  uint64_t d_dec_b_cap = 0;
  bool busy = false;
};

// ---- the host-to-host ring (tm_tokenize_pipeline on page-locked buffers) ---------------------------------------------------------------------
// A slot = one chunk in flight: a workspace, the packed ids on the device, and a page-locked block for what goes to and comes from the host
// beside the bulk data (the chunk's verdict, raw offsets in, id offsets and missing counts out).
struct RingSlot {
  tm_batch* ws = nullptr;
  uint8_t* d_bytes = nullptr;
  uint64_t d_bytes_cap = 0;
  uint8_t* h_pin = nullptr;
  uint64_t h_pin_cap = 0, docs_cap = 0;
  hipEvent_t up_done = nullptr, comp_done = nullptr, dl_done = nullptr;
  const uint8_t* ids_at = nullptr;   // where the packed ids of the chunk in the slot lie (d_bytes, or the workspace's id buffer)
  uint64_t* h_status() const { return reinterpret_cast<uint64_t*>(h_pin); }
  uint64_t* h_roff() const { return reinterpret_cast<uint64_t*>(h_pin + 64); }
  uint64_t* h_toff() const { return reinterpret_cast<uint64_t*>(h_pin + 64 + (docs_cap + 2) * 8); }
  uint32_t* h_missing() const { return reinterpret_cast<uint32_t*>(h_pin + 64 + 2 * (docs_cap + 2) * 8); }
};
struct Ring {
  hipStream_t up = nullptr, down = nullptr;
  std::vector<hipStream_t> comp;
  std::vector<RingSlot> slots;
  bool busy = false;                 // one call at a time drives the ring (LanePool::mu); a second caller takes the lanes
};

struct LanePool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Lane*> lanes;
  size_t max_lanes = 8;
  Ring ring;
};

static void lane_destroy(Lane* l) {
  if (!l) return;
  tm_batch_free(l->ws);
  if (l->stream) (void)hipStreamDestroy(l->stream);
  if (l->up_stream) (void)hipStreamDestroy(l->up_stream);
  if (l->up_done) (void)hipEventDestroy(l->up_done);
  (void)hipHostFree(l->h_stage);
  (void)hipHostFree(l->h_stage_in);
  (void)hipFree(l->d_bytes);
  (void)hipFree(l->d_dec_a);
  (void)hipFree(l->d_dec_b);
  delete l;
}

void pool_destroy(LanePool* p) {
  if (!p) return;
  for (Lane* l : p->lanes) lane_destroy(l);
  Ring& r = p->ring;
  for (RingSlot& s : r.slots) {
    tm_batch_free(s.ws);
    (void)hipFree(s.d_bytes);
    (void)hipHostFree(s.h_pin);
    for (hipEvent_t ev : {s.up_done, s.comp_done, s.dl_done}) if (ev) (void)hipEventDestroy(ev);
  }
  for (hipStream_t st : r.comp) if (st) (void)hipStreamDestroy(st);
  if (r.up) (void)hipStreamDestroy(r.up);
  if (r.down) (void)hipStreamDestroy(r.down);
  delete p;
}

static LanePool* pool_of(const tm_vocab* v) {
  static std::mutex create_mu;
  std::lock_guard<std::mutex> g(create_mu);
  if (!v->pool) {
    v->pool = new LanePool();
    v->pool->max_lanes = (size_t)env_int("TM_LANES", 1, 64, (int)v->pool->max_lanes);
  }
  return v->pool;
}

// borrow a lane (blocks while all max_lanes are busy); *out is returned with busy == true
static int lane_acquire(const tm_vocab* v, Lane** out) {
  int rc = enter_device(v);
  if (rc != TM_OK) return rc;
  LanePool* p = pool_of(v);
  std::unique_lock<std::mutex> lk(p->mu);
  for (;;) {
    for (Lane* l : p->lanes) if (!l->busy) { l->busy = true; *out = l; return TM_OK; }
    if (p->lanes.size() < p->max_lanes) {
      Lane* l = new Lane();
      hipError_t e = hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking);
      if (e != hipSuccess) { delete l; return hip_fail(e, "hipStreamCreate (lane)"); }
      l->busy = true;
      p->lanes.push_back(l);
      *out = l;
      return TM_OK;
    }
    p->cv.wait(lk);
  }
}

// ---- the GPU's NUMA node ------------------------------------------------------------------------------------------------------------------
// A two-socket host has the GPU's PCIe root under ONE of its sockets.  Page-locked memory from hipHostMalloc already comes from the NUMA node
// nearest to the current device (the runtime's default; hipHostMallocNumaUser would switch that off), but the THREADS that feed a lane -
// command submission, the memcpy through pinned staging for pageable buffers, the waits - run wherever the scheduler put them, and from the
// far socket every doorbell and every completion crosses the inter-socket link: the box-to-box spread of the host-to-host rate in rounds
// 3 and 4 (27 - 34 GB/s for one library).  The workers of tm_tokenize_pipeline therefore run on the CPUs of the device's node for the length
// of the call (the calling thread gets its own mask back); TM_NUMA=0 in the environment switches that off.
struct NumaNear { int node = -1; cpu_set_t cpus; bool pin = false; };      // cpus: the node's own list, as the kernel gives it; pin: TM_NUMA has not switched the moving of threads off
static const NumaNear& numa_near(int device) {
  static std::mutex mu;
  static NumaNear table[64];
  static bool done[64] = {};
  std::lock_guard<std::mutex> g(mu);
  NumaNear& n = table[device < 0 || device >= 64 ? 0 : device];
  if (device < 0 || device >= 64 || done[device]) return n;
  done[device] = true;
  CPU_ZERO(&n.cpus);
  // (the node is read whatever TM_NUMA says: tm_device_numa_node reports it to callers that pin their own feeding threads; TM_NUMA=0 only
  // keeps THIS library from moving threads)
  const char* off = getenv("TM_NUMA");
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) { (void)hipGetLastError(); return n; }
  for (char* c = bdf; *c; c++) *c = (char)tolower((unsigned char)*c);
  char path[160];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
  FILE* f = fopen(path, "r");
  if (!f) return n;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  if (node < 0) return n;                        // (a one-node host, or a kernel that does not say)
  n.node = node;
  snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
  if (!(f = fopen(path, "r"))) return n;
  char list[4096] = {0};
  const bool got = fgets(list, sizeof list, f) != nullptr;
  fclose(f);
  if (!got) return n;
  int count = 0;
  for (char* p = list; *p && *p != '\n';) {       // "0-63,128-191"
    char* end = nullptr;
    const long a = strtol(p, &end, 10);
    if (end == p) break;
    long b = a;
    if (*end == '-') { p = end + 1; b = strtol(p, &end, 10); }
    for (long c = a; c <= b && c < CPU_SETSIZE; c++) { CPU_SET((int)c, &n.cpus); count++; }
    p = *end == ',' ? end + 1 : end;
  }
  n.pin = count > 0 && !(off && atoi(off) == 0);
  return n;
}
// the calling thread on the CPUs near `device` while the object lives - those of them the thread may use at all: the node's list is
// intersected with the thread's OWN mask at every call (a container's cpuset, a caller's pinning of this thread: what one thread was
// allowed at the first call says nothing about the next), and a thread that already runs on the node only (a caller's pinned feeder
// thread) is left exactly where it is
struct NearDevice {
  cpu_set_t before;
  bool changed = false;
  explicit NearDevice(int device) {
    const NumaNear& n = numa_near(device);
    if (!n.pin || sched_getaffinity(0, sizeof before, &before) != 0) return;
    cpu_set_t want;
    CPU_AND(&want, &n.cpus, &before);
    if (CPU_COUNT(&want) == 0 || CPU_EQUAL(&want, &before)) return;       // nothing of the node is allowed / the thread is on the node already
    changed = sched_setaffinity(0, sizeof want, &want) == 0;
  }
  ~NearDevice() { if (changed) (void)sched_setaffinity(0, sizeof before, &before); }
  NearDevice(const NearDevice&) = delete;
  NearDevice& operator=(const NearDevice&) = delete;
};

static void lane_release(const tm_vocab* v, Lane* l) {
  LanePool* p = v->pool;
  { std::lock_guard<std::mutex> g(p->mu); l->busy = false; }
  p->cv.notify_one();
}

// grow-only, with the lanes' headroom, so that a server converges to zero allocations (grow_workspace / grow_pinned / grow_device, tm_pipeline.h)
static uint64_t lane_room(uint64_t bytes) { return bytes + bytes / 4 + 4096; }
static int lane_workspace(Lane* l, const tm_vocab* v, uint64_t bytes, uint32_t docs) {
  return grow_workspace(&l->ws, v, bytes, docs, bytes + bytes / 4 + (1u << 20), "lane workspace");
}
static int lane_pinned(uint8_t** buf, uint64_t* cap, uint64_t bytes) { return grow_pinned(buf, cap, bytes, lane_room(bytes), "lane staging (pinned)"); }
static int lane_device(uint8_t** buf, uint64_t* cap, uint64_t bytes, const char* what) { return grow_device(buf, cap, bytes, lane_room(bytes), what); }
static int lane_dbytes(Lane* l, uint64_t bytes) { return lane_device(&l->d_bytes, &l->d_bytes_cap, bytes, "lane serialized ids"); }

struct RunOut { uint64_t total_tokens = 0; };

// upload + run one batch on a lane; the ids stay on the device (l->ws->d_out)
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// raw text grows under capcode (about 1.1x; worst case every byte a capital: "DC x" = 4x)
static uint64_t lane_need(bool raw, uint64_t nbytes) { return raw ? nbytes + nbytes / 2 + 4096 : nbytes; }
// H2D of one batch into the lane's workspace on stream `st` (the workspace must be idle, or — raw text only — past its normalizer pass)
static int lane_upload(Lane* l, const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, bool raw, hipStream_t st) {
  const uint64_t nbytes = ndocs ? offsets[ndocs] : 0;
  int rc = lane_workspace(l, v, lane_need(raw, nbytes), ndocs);
  if (rc != TM_OK) return rc;
  return raw ? batch_upload_raw_on(l->ws, text, offsets, ndocs, st) : batch_upload_on(l->ws, text, offsets, ndocs, st);
}
// normalize (raw text) + the tokenizer pipeline on what lane_upload has put into the workspace; the ids stay on the device (l->ws->d_out)
static int lane_compute(Lane* l, const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, bool raw, bool emit, RunOut* ro,
                        const std::function<int()>& after_normalize = nullptr) {
  static const bool trace = getenv("TM_TRACE") != nullptr;
  const double t0 = trace ? now_ms() : 0;
  double t1 = 0, t2 = 0;
  const uint64_t nbytes = ndocs ? offsets[ndocs] : 0;
  int rc = TM_OK;
  tm_batch* b = l->ws;
  if (raw) {
    rc = tm_batch_normalize(b, l->stream);
    if (rc == TM_E_LIMIT) {      // capital-heavy text: retry once with the worst-case workspace
      if ((rc = lane_workspace(l, v, 4 * nbytes + 4096, ndocs)) != TM_OK) return rc;
      b = l->ws;
      if ((rc = batch_upload_raw_on(b, text, offsets, ndocs, l->stream)) != TM_OK) return rc;
      rc = tm_batch_normalize(b, l->stream);
    }
  }
  if (rc != TM_OK) return rc;
  if (after_normalize && (rc = after_normalize()) != TM_OK) return rc;     // (the raw text buffer is free from here on)
  if (trace) t1 = now_ms();
  if ((rc = run_pipeline(b, l->stream, false, nullptr, emit)) != TM_OK) return rc;
  if (trace) t2 = now_ms();
  if (emit) {
    if ((rc = ensure_output(b)) != TM_OK) return rc;
  } else {
    hipError_t e = hipStreamSynchronize(l->stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
  }
  if (ro) {
    if (!emit) {                       // (ensure_output has read them already otherwise)
      if ((rc = small_d2h(b, b->last_totals, b->d_totals, sizeof b->last_totals, l->stream)) != TM_OK || (rc = small_sync(b, l->stream)) != TM_OK) return rc;
    }
    ro->total_tokens = ndocs ? b->last_totals[1] : 0;
  }
  if (trace) fprintf(stderr, "[lane %p] %llu bytes: %s %.2f ms, launch %.2f ms, wait %.2f ms\n", (void*)l, (unsigned long long)nbytes, raw ? "normalize" : "-", t1 - t0, t2 - t1, now_ms() - t2);
  return TM_OK;
}
static int lane_run(Lane* l, const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, bool raw, bool emit, RunOut* ro) {
  int rc = lane_upload(l, v, text, offsets, ndocs, raw, l->stream);
  return rc == TM_OK ? lane_compute(l, v, text, offsets, ndocs, raw, emit, ro) : rc;
}

static int d2h(void* dst, const void* src, uint64_t bytes, hipStream_t st, const char* what) {
  if (!bytes) return TM_OK;
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  return e == hipSuccess ? TM_OK : hip_fail(e, what);
}

}  // namespace tmh

using namespace tmh;

extern "C" {

int tm_device_numa_node(int device) {
  int have = 0;
  if (hipGetDeviceCount(&have) != hipSuccess || device < 0 || device >= have) { (void)hipGetLastError(); return -1; }
  return numa_near(device).node;
}

void* tm_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void tm_host_free(void* p) { if (p) (void)hipHostFree(p); }
int tm_host_register(void* p, size_t bytes) {
  hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
  return e == hipSuccess ? TM_OK : hip_fail(e, "hipHostRegister");
}
int tm_host_unregister(void* p) {
  hipError_t e = hipHostUnregister(p);
  return e == hipSuccess ? TM_OK : hip_fail(e, "hipHostUnregister");
}

// The one body of the one-shot calls: a lane, the run, the documents' id offsets and missing counts, the span pass where one is asked for,
// the ids - as u32, or packed to `enc` bytes -, and the lane back with nothing in flight and nothing pending in the mailbox.  small_sync runs
// on every path behind a completed run: it is what fills tok_offsets and missing, also for a call that is refused.
enum class SpanStep { none, normalized, raw };
struct OneShot {
  bool raw;                 // the text is raw: the normalizer runs in front
  SpanStep spans;
  uint32_t unit;            // TM_UNIT_*: what the pairs count (tm_units.hip)
  uint32_t enc;             // 0: ids_out takes u32 ids and `cap` counts ids; 2 .. 4: the serialized form, `cap` counts bytes and offsets_out takes byte offsets
  const char* who;
  void* ids_out; uint64_t cap; uint64_t* offsets_out; uint32_t* spans_out; uint32_t* missing;
};
static int one_shot(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, const OneShot& o) {
  if (!v || (ndocs && !offsets)) return set_error(TM_E_INVALID, "null argument");
  Lane* l = nullptr;
  int rc = lane_acquire(v, &l);
  if (rc != TM_OK) return rc;
  RunOut ro;
  rc = lane_run(l, v, text, offsets, ndocs, o.raw, true, &ro);
  if (rc == TM_OK) {
    tm_batch* b = l->ws;
    const uint64_t total = ro.total_tokens, need = o.enc ? total * o.enc : total;
    const bool fits = need <= o.cap;
    // the serialized form reads the id offsets into an array of its own: the caller's array takes BYTE offsets, made from them behind the wait
    std::vector<uint64_t> id_offs(o.enc ? (size_t)ndocs + 1 : 0, 0);
    uint64_t* const toff = o.enc ? id_offs.data() : o.offsets_out;
    if (toff && ndocs) rc = small_d2h(b, toff, b->d_tok_offsets, ((uint64_t)ndocs + 1) * 8, l->stream);
    if (rc == TM_OK && o.missing && ndocs) rc = small_d2h(b, o.missing, b->d_doc_missing, (uint64_t)ndocs * 4, l->stream);
    if (rc == TM_OK && fits && o.spans != SpanStep::none) {
      if (total && (!o.ids_out || !o.spans_out)) rc = set_error(TM_E_INVALID, "null argument");
      // the pairs behind the run on the lane's stream, into the workspace's own grow-only buffer (lane_run has waited for the run: ensure_output)
      if (rc == TM_OK) rc = spans_ready(b, o.who);
      if (rc == TM_OK && o.spans == SpanStep::raw) rc = origin_ready(b, o.who);
      if (rc == TM_OK) rc = batch_own_spans_on(b, l->stream, o.spans == SpanStep::raw ? TM_TEXT_RAW : TM_TEXT_NORMALIZED, o.unit, total);
    }
    if (rc == TM_OK && fits && total) {
      if (!o.enc) rc = small_d2h(b, o.ids_out, b->d_out, total * 4, l->stream);
      else if ((rc = lane_dbytes(l, need)) == TM_OK) {
        launch_serialize(b->d_out, total, o.enc, l->d_bytes, l->stream);
        rc = small_d2h(b, o.ids_out, l->d_bytes, need, l->stream);
      }
    }
    if (rc == TM_OK && fits && o.spans != SpanStep::none) rc = small_d2h(b, o.spans_out, b->d_spans, total * 8, l->stream);
    { const int rs = small_sync(b, l->stream); if (rc == TM_OK) rc = rs; }
    if (ndocs == 0 && toff) toff[0] = 0;
    if (rc == TM_OK && o.enc && o.offsets_out) for (size_t d = 0; d <= ndocs; d++) o.offsets_out[d] = id_offs[d] * o.enc;
    // TM_E_NOSPACE is answered last on every form: tok_offsets is complete once small_sync has run, byte_offsets once the line above has - and
    // both say what capacity the call needs
    if (rc == TM_OK && !fits) {
      rc = o.enc ? set_error(TM_E_NOSPACE, "bytes_cap too small")
                 : set_error(TM_E_NOSPACE, "tokens_cap %llu < %llu required", (unsigned long long)o.cap, (unsigned long long)total);
    }
  }
  lane_release(v, l);
  return rc;
}

int tm_tokenize_batch(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, uint32_t* tokens_out,
                      uint64_t tokens_cap, uint64_t* tok_offsets, uint32_t* missing) {
  return one_shot(v, text, offsets, ndocs, OneShot{false, SpanStep::none, TM_UNIT_BYTES, 0, "tm_tokenize_batch", tokens_out, tokens_cap, tok_offsets, nullptr, missing});
}

int tm_tokenize_batch_spans(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, uint32_t* tokens_out,
                            uint64_t tokens_cap, uint64_t* tok_offsets, uint32_t* spans_out, uint32_t* missing) {
  return one_shot(v, text, offsets, ndocs, OneShot{false, SpanStep::normalized, TM_UNIT_BYTES, 0, "tm_tokenize_batch_spans", tokens_out, tokens_cap, tok_offsets, spans_out, missing});
}

int tm_tokenize_batch_raw_spans(const tm_vocab* v, const uint8_t* raw, const uint64_t* offsets, uint32_t ndocs, uint32_t* tokens_out,
                                uint64_t tokens_cap, uint64_t* tok_offsets, uint32_t* spans_out, uint32_t* missing) {
  return one_shot(v, raw, offsets, ndocs, OneShot{true, SpanStep::raw, TM_UNIT_BYTES, 0, "tm_tokenize_batch_raw_spans", tokens_out, tokens_cap, tok_offsets, spans_out, missing});
}

int tm_tokenize_batch_spans_in(const tm_vocab* v, const uint8_t* docs, const uint64_t* offsets, uint32_t ndocs, uint32_t text, uint32_t unit,
                               uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* tok_offsets, uint32_t* spans_out, uint32_t* missing) {
  const int rc = units_args(text, unit, "tm_tokenize_batch_spans_in");
  if (rc != TM_OK) return rc;
  const bool raw = text == TM_TEXT_RAW;
  return one_shot(v, docs, offsets, ndocs, OneShot{raw, raw ? SpanStep::raw : SpanStep::normalized, unit, 0, "tm_tokenize_batch_spans_in", tokens_out, tokens_cap, tok_offsets, spans_out, missing});
}

static int count_batch(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, bool raw, uint64_t* counts, uint32_t* missing) {
  if (!v || (ndocs && !offsets)) return set_error(TM_E_INVALID, "null argument");
  Lane* l = nullptr;
  int rc = lane_acquire(v, &l);
  if (rc != TM_OK) return rc;
  rc = lane_run(l, v, text, offsets, ndocs, raw, false, nullptr);
  if (rc == TM_OK && ndocs) {
    tm_batch* b = l->ws;
    std::vector<uint32_t> ev(ndocs);
    uint32_t err = 0;
    rc = small_d2h(b, &err, b->d_error, 4, l->stream);
    if (rc == TM_OK) rc = small_d2h(b, ev.data(), b->d_doc_events, (uint64_t)ndocs * 4, l->stream);
    if (rc == TM_OK && missing) rc = small_d2h(b, missing, b->d_doc_missing, (uint64_t)ndocs * 4, l->stream);
    if (rc == TM_OK) rc = small_sync(b, l->stream); else (void)small_sync(b, l->stream);
    if (rc == TM_OK && err) rc = error_from_flag(err);
    if (rc == TM_OK && counts) for (uint32_t d = 0; d < ndocs; d++) counts[d] = ev[d];
  }
  lane_release(v, l);
  return rc;
}

int tm_count_batch(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, uint64_t* counts, uint32_t* missing) {
  return count_batch(v, text, offsets, ndocs, false, counts, missing);
}
int tm_count_batch_raw(const tm_vocab* v, const uint8_t* raw, const uint64_t* offsets, uint32_t ndocs, uint64_t* counts, uint32_t* missing) {
  return count_batch(v, raw, offsets, ndocs, true, counts, missing);
}

int tm_tokenize_batch_serialized(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, uint32_t encoding_length,
                                 uint8_t* bytes_out, uint64_t bytes_cap, uint64_t* byte_offsets, uint32_t* missing, uint32_t* encoding_length_used) {
  if (!v || (ndocs && !offsets)) return set_error(TM_E_INVALID, "null argument");
  if (encoding_length <= 1) encoding_length = v->host.n_ids <= 65536 ? 2 : 3;          // go :990-996
  if (encoding_length < 2 || encoding_length > 4) return set_error(TM_E_INVALID, "Invalid encoding length");   // go :1012
  if (encoding_length_used) *encoding_length_used = encoding_length;
  return one_shot(v, text, offsets, ndocs, OneShot{false, SpanStep::none, TM_UNIT_BYTES, encoding_length, "tm_tokenize_batch_serialized", bytes_out, bytes_cap, byte_offsets, nullptr, missing});
}

// ---- large batches, host to host -------------------------------------------------------------------------------------------------
int tm_tokenize_pipeline(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, int raw, uint32_t encoding_length,
                         uint64_t chunk_bytes, uint32_t lanes, uint8_t* bytes_out, uint64_t bytes_cap, uint64_t* byte_offsets, uint32_t* missing,
                         uint32_t* encoding_length_used, tm_pipeline_stats* stats) {
  return tmh::tokenize_pipeline_on(&v, 1, text, offsets, ndocs, raw, encoding_length, chunk_bytes, lanes, bytes_out, bytes_cap, byte_offsets, missing,
                                   encoding_length_used, stats);
}

}  // extern "C"
namespace tmh {
// ---- tm_tokenize_pipeline ------------------------------------------------------------------------------------------------------------------
// What both forms of the pipeline share: the call's arguments, the chunk list, and the chain of id counts - chunk k's ids go behind those of
// chunks 0..k-1 wherever and whenever they were computed.
struct PipeCall {
  const tm_vocab* const* vs; uint32_t nv;
  const uint8_t* text; const uint64_t* offsets; uint32_t ndocs; int raw; uint32_t enc;
  uint64_t chunk_bytes; uint32_t lanes;
  uint8_t* bytes_out; uint64_t bytes_cap; uint64_t* byte_offsets; uint32_t* missing; tm_pipeline_stats* stats;
  bool in_pinned = false, out_pinned = false;
  std::vector<uint32_t> first;     // first document of every chunk, + ndocs
  size_t nchunks = 0;
  std::vector<uint64_t> tok_base;  // ids before chunk k
  std::vector<char> known;
  std::mutex mu;
  std::condition_variable cv;
  int first_error = TM_OK;
  std::string first_msg;
  std::atomic<size_t> next{0};
  double t0 = 0;
  // chunk k: its documents [d0, d0 + nd) and its bytes [b0, b0 + nb) of the call's text
  struct Chunk {
    const uint64_t* off;      // = offsets + d0
    uint32_t d0, nd; uint64_t b0, nb;
    void local_offsets(uint64_t* lo) const { for (uint32_t d = 0; d <= nd; d++) lo[d] = off[d] - b0; }      // lo[nd + 1]: the documents' offsets counted from the chunk's first byte
  };
  Chunk chunk(size_t k) const { const uint32_t d0 = first[k], nd = first[k + 1] - d0; return Chunk{offsets + d0, d0, nd, offsets[d0], offsets[d0 + nd] - offsets[d0]}; }
  // A chunk's place in the output, once the chain of counts has said that `base` ids lie before its `ntok`: the bytes of bytes_out that take its
  // packed ids - none (bytes == 0) when it has no ids, or when they do not fit and the call ends with TM_E_NOSPACE - and its documents' byte
  // offsets from their id offsets toff[nd + 1] within the chunk.  How the bytes get there is the caller's business (a lane's, the ring's).
  struct Place { uint8_t* at; uint64_t bytes; };
  Place place(uint64_t base, uint64_t ntok) const {
    const bool fits = (base + ntok) * enc <= bytes_cap && bytes_out;
    return fits ? Place{bytes_out + base * enc, ntok * enc} : Place{nullptr, 0};
  }
  void place_offsets(const Chunk& ch, uint64_t base, const uint64_t* toff) const { for (uint32_t d = 1; d <= ch.nd; d++) byte_offsets[ch.d0 + d] = (base + toff[d]) * enc; }
  // test hook 24 (tm_debug_flags, TM_TEST_FAIL="<place>:<chunk>[:<chunks>]"): ONE chunk of this call fails with TM_E_INPUT at a place of the
  // host code - an error return like any other, nothing on the device differs.  hook_place stays 0 in every call of a process without the hook.
  enum { HOOK_FINISHER = 1, HOOK_EXACT, HOOK_ISSUER, HOOK_DOWNLOAD };
  int hook_place = 0;
  size_t hook_chunk = 0;
  bool hook(int place, size_t k) const { return hook_place == place && hook_chunk == k; }
  void hook_arm() {
    static const char* const names[] = {"", "finisher", "exact", "issuer", "download"};
    const char* e = getenv("TM_TEST_FAIL");
    const char* colon = e ? strchr(e, ':') : nullptr;
    if (!colon) return;
    char* end = nullptr;
    const unsigned long long k = strtoull(colon + 1, &end, 10);
    if (end == colon + 1) return;
    if (*end == ':' && strtoull(end + 1, nullptr, 10) != nchunks) return;      // (a call of another shape: a second caller beside the one under test)
    for (int p = HOOK_FINISHER; p <= HOOK_DOWNLOAD; p++)
      if (strlen(names[p]) == (size_t)(colon - e) && !strncmp(e, names[p], (size_t)(colon - e))) { hook_place = p; hook_chunk = (size_t)k; }
  }
  static int hook_fail(const char* place, size_t k) { return set_error(TM_E_INPUT, "test hook 24: chunk %zu fails at the place '%s' of the pipeline", k, place); }
  void fail(int rc) {
    { std::lock_guard<std::mutex> g(mu); if (first_error == TM_OK) { first_error = rc; first_msg = last_error(); } }
    cv.notify_all();
  }
  bool failed() { std::lock_guard<std::mutex> g(mu); return first_error != TM_OK; }
  // publish chunk k's count, learn where its ids go; false: another chunk has failed
  bool order(size_t k, uint64_t ntok, uint64_t* base) {
    { std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return known[k] || first_error != TM_OK; });
      if (first_error != TM_OK) return false;
      tok_base[k + 1] = tok_base[k] + ntok;
      known[k + 1] = 1;
      *base = tok_base[k]; }
    cv.notify_all();
    return true;
  }
};

// The second half of a chunk on a lane: its ids lie in l->ws and their number is known.  The chunk takes its place in the chain of counts; id
// offsets and missing counts come through the mailbox, the packed ids through l->d_bytes into the caller's buffer (directly, or through
// h_stage when that buffer is pageable); one wait; offsets and statistics.  *delivered stays false with TM_OK when another chunk has failed.
// `toff` is the caller's scratch: a failure may leave a small transfer into it pending, which the caller's clean-up waits for.
// download_hook: test hook place HOOK_DOWNLOAD lies between the enqueued download and the wait (the lanes' form; the ring has its own).
static int chunk_deliver(PipeCall& c, Lane* l, size_t k, uint64_t ntok, bool download_hook, std::vector<uint64_t>& toff, bool* delivered, double* t_ordered = nullptr) {
  *delivered = false;
  const PipeCall::Chunk ch = c.chunk(k);
  uint64_t base = 0;
  if (!c.order(k, ntok, &base)) return TM_OK;          // publish this chunk's count, learn where its ids go
  if (t_ordered) *t_ordered = now_ms();
  tm_batch* b = l->ws;
  const PipeCall::Place out = c.place(base, ntok);
  int rc = TM_OK;
  toff.resize((size_t)ch.nd + 1);
  if ((rc = small_d2h(b, toff.data(), b->d_tok_offsets, toff.size() * 8, l->stream)) != TM_OK) return rc;
  if (c.missing && ch.nd && (rc = small_d2h(b, c.missing + ch.d0, b->d_doc_missing, (uint64_t)ch.nd * 4, l->stream)) != TM_OK) return rc;
  if (out.bytes) {
    // (Writing the ids straight into the caller's page-locked buffer from the serialize kernel - no device staging, no copy command - was
    // built and timed in round 5: 42 - 45 ms per GiB call against 32 - 36 with the copy engine, profiles/r05_h2h.txt: stores of a kernel to
    // fine-grained host memory cross PCIe far below the engine's rate.  Removed.)
    if ((rc = lane_dbytes(l, out.bytes)) != TM_OK) return rc;
    launch_serialize(b->d_out, ntok, c.enc, l->d_bytes, l->stream);
    if (c.out_pinned) rc = d2h(out.at, l->d_bytes, out.bytes, l->stream, "D2H ids");
    else if ((rc = lane_pinned(&l->h_stage, &l->h_cap, out.bytes)) == TM_OK) rc = d2h(l->h_stage, l->d_bytes, out.bytes, l->stream, "D2H ids");
    if (rc != TM_OK) return rc;
  }
  if (download_hook && c.hook(PipeCall::HOOK_DOWNLOAD, k)) return PipeCall::hook_fail("download", k);
  if ((rc = small_sync(b, l->stream)) != TM_OK) return rc;
  if (out.bytes && !c.out_pinned) std::memcpy(out.at, l->h_stage, out.bytes);
  c.place_offsets(ch, base, toff.data());
  if (c.stats) { std::lock_guard<std::mutex> g(c.mu); c.stats->host_fallback_docs += c.raw ? b->host_fallback_docs : 0; c.stats->normalized_bytes += b->nbytes; }
  *delivered = true;
  return TM_OK;
}

// Where an upload reads the chunk's text from: the caller's buffer when that is page-locked, else the lane's pinned input staging with the text
// copied into it, so that the H2D runs at link speed
static int chunk_text(const PipeCall& c, Lane* l, const PipeCall::Chunk& ch, const uint8_t** src) {
  *src = c.text + ch.b0;
  if (c.in_pinned) return TM_OK;
  const int rc = lane_pinned(&l->h_stage_in, &l->h_in_cap, ch.nb);
  if (rc != TM_OK) return rc;
  std::memcpy(l->h_stage_in, *src, ch.nb);
  *src = l->h_stage_in;
  return TM_OK;
}
// A lane on its way back after the failure `rc`: nothing of the chunk is in flight when it gets there - no download into the caller's buffer, no
// small transfer that would land in the failed thread's own arrays during a later call.  The failure's message outlives the wait.
static void lane_quiet(Lane* l, int rc) {
  const std::string msg = last_error();
  if (l->ws) (void)small_sync(l->ws, l->stream); else (void)hipStreamSynchronize(l->stream);
  set_error(rc, "%s", msg.c_str());
}

// One chunk through the exact path on a borrowed lane, start to finish (the ring's way out for a chunk its one-pass form does not take; no
// prefetching, every wait in line)
static int chunk_exact(PipeCall& c, const tm_vocab* v, size_t k) {
  const PipeCall::Chunk ch = c.chunk(k);
  Lane* l = nullptr;
  int rc = lane_acquire(v, &l);
  if (rc != TM_OK) return rc;
  std::vector<uint64_t> lo((size_t)ch.nd + 1), toff;
  ch.local_offsets(lo.data());
  const uint8_t* src = nullptr;
  RunOut ro;
  bool delivered = false;
  if ((rc = chunk_text(c, l, ch, &src)) == TM_OK && (rc = lane_run(l, v, src, lo.data(), ch.nd, c.raw != 0, true, &ro)) == TM_OK)
    rc = c.hook(PipeCall::HOOK_EXACT, k) ? PipeCall::hook_fail("exact", k) : chunk_deliver(c, l, k, ro.total_tokens, false, toff, &delivered);
  if (rc != TM_OK) lane_quiet(l, rc);
  lane_release(v, l);
  return rc;
}

// ---- the ring --------------------------------------------------------------------------------------------------------------------------------
// Raw text in page-locked memory -> packed ids in page-locked memory, with NO host round trip inside a chunk.  The lanes' form below waits
// for the device three times per chunk (the normalizer's counts, the id count, the end of the download), and every wait drains the lane's
// stream: four lanes' streams on the runtime's four hardware queues kept the device 85 % busy at best (profiles/r06_h2h.txt).  Here ONE
// thread per device (the issuer) enqueues chunk after chunk - upload on the copy stream `up`, the normalizer pass and K0 .. K4 + the packing
// of the ids on one of two compute streams, alternating, so that the thin kernels of one chunk run beside the wide ones of the next - and never
// waits for the device: grids behind the normalizer pass are launched over a bound and the kernels look the counts up (tm_batch::d_ctl).
// A second thread (the finisher) waits for a chunk's end, reads its verdict and id count from the slot's page-locked block, takes the chunk's
// place in the output from the chain of counts, and enqueues the download on the copy stream `down`.  A chunk the one-pass form does not
// take (documents for the host normalizer, a long document, a piece whose margins could not tell ...) costs its kernels nothing behind the
// normalizer pass (ctl[0] == 0) and is run through the exact path by the finisher (chunk_exact).
static int ring_slot_size(RingSlot& s, const tm_vocab* v, uint64_t need_bytes, uint32_t need_docs) {
  int rc = grow_workspace(&s.ws, v, need_bytes, need_docs, need_bytes + need_bytes / 8 + (1u << 20), "ring workspace");
  if (rc != TM_OK) return rc;
  const uint64_t nb = s.ws->out_cap * 4;          // (room for the widest form: the slot outlives the call)
  if ((rc = grow_device(&s.d_bytes, &s.d_bytes_cap, nb, nb, "ring ids")) != TM_OK) return rc;
  // (the block's layout hangs on the workspace's document count, which only grows - and the block's size with it)
  const uint64_t dc = s.ws->max_docs;
  if ((rc = grow_pinned(&s.h_pin, &s.h_pin_cap, 64 + 2 * (dc + 2) * 8 + (dc + 2) * 4, 64 + 2 * (dc + 2) * 8 + (dc + 2) * 4, "ring slot (pinned)")) != TM_OK) return rc;
  s.docs_cap = dc;
  hipError_t e;
  for (hipEvent_t* ev : {&s.up_done, &s.comp_done, &s.dl_done})
    if (!*ev && (e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return hip_fail(e, "hipEventCreate (ring)");
  return TM_OK;
}

static int pipeline_ring(PipeCall& c, const std::vector<Ring*>& rings) {
  static const bool trace = getenv("TM_TRACE") != nullptr;
  static const uint32_t slack_pct = (uint32_t)env_int("TM_RING_SLACK", 100, 400, 125);
  // per device: a queue of issued chunks for the finisher, and the slots' states
  struct Dev {
    const tm_vocab* v; Ring* r;
    std::mutex mu; std::condition_variable cv;
    std::vector<std::pair<size_t, int>> queue;       // (chunk, slot) in issue order; slot -1: a chunk for the exact path as it is
    size_t qhead = 0;
    bool issuer_done = false;
    std::vector<char> slot_free;
  };
  // A slot in the finisher's hands.  The issuer may be waiting for it, so it goes back on EVERY way out: the lease's end gives it back, and the
  // lease ends when its holder lets go of it (the chunk is complete, or runs on through the exact path, which needs no slot) or goes out of scope
  // (the chunk failed, or is drained behind a failure).  A chunk whose download is enqueued takes its lease along into Pending.  A chunk issued
  // for the exact path has no slot and no lease.
  struct Lease {
    Dev& dv; const int si;
    Lease(Dev& d, int slot) : dv(d), si(slot) {}
    Lease(const Lease&) = delete;
    ~Lease() {
      { std::lock_guard<std::mutex> g(dv.mu); dv.slot_free[si] = 1; }
      dv.cv.notify_all();
    }
  };
  typedef std::unique_ptr<Lease> Held;
  std::vector<std::unique_ptr<Dev>> devs;
  for (uint32_t i = 0; i < c.nv; i++) { auto d = std::make_unique<Dev>(); d->v = c.vs[i]; d->r = rings[i]; d->slot_free.assign(rings[i]->slots.size(), 1); devs.push_back(std::move(d)); }

  // A failure is every pair's business: the first one is recorded, and every issuer that waits for a slot - on this device or another - hears of
  // it (the lock is taken and dropped so that the news cannot fall between a waiter's look at the predicate and its sleep).
  auto fail_all = [&](int rc) {
    c.fail(rc);
    for (auto& d : devs) { { std::lock_guard<std::mutex> g(d->mu); } d->cv.notify_all(); }
  };

  auto issuer = [&](Dev& dv) {
    const tm_vocab* const v = dv.v;
    Ring& r = *dv.r;
    NearDevice near_gpu(v->device);
    int rc = enter_device(v);
    size_t issued = 0;
    bool enqueued = false;
    while (rc == TM_OK && !c.failed()) {
      const size_t k = c.next.fetch_add(1);
      if (k >= c.nchunks) break;
      const PipeCall::Chunk ch = c.chunk(k);
      int si = -1;
      if (ch.nb > 0) {
        // a free slot (the finisher hands them back in order)
        std::unique_lock<std::mutex> lk(dv.mu);
        dv.cv.wait(lk, [&] { for (char f : dv.slot_free) if (f) return true; return c.failed(); });
        if (c.failed()) break;          // (nothing more is issued behind a failure; the finisher drains what is in flight)
        for (size_t j = 0; j < dv.slot_free.size(); j++) { const size_t q = (issued + j) % dv.slot_free.size(); if (dv.slot_free[q]) { si = (int)q; break; } }
        dv.slot_free[si] = 0;
      }
      if (si >= 0) {
        RingSlot& s = r.slots[si];
        tm_batch* b = s.ws;
        uint64_t* lo = s.h_roff();
        ch.local_offsets(lo);
        hipStream_t cs = r.comp[issued % r.comp.size()];
        hipError_t e = hipSuccess;
        const double ti0 = trace ? now_ms() : 0;
        enqueued = true;
        if ((rc = raw_prepare(b, ch.nb, ch.nd, raw_piece_count(v, lo, ch.nd), cs)) != TM_OK) break;
        if ((e = hipMemcpyAsync(b->d_raw, c.text + ch.b0, ch.nb, hipMemcpyHostToDevice, r.up)) != hipSuccess ||
            (e = hipMemcpyAsync(b->d_raw_off, lo, ((uint64_t)ch.nd + 1) * 8, hipMemcpyHostToDevice, r.up)) != hipSuccess ||
            (e = hipEventRecord(s.up_done, r.up)) != hipSuccess || (e = hipStreamWaitEvent(cs, s.up_done, 0)) != hipSuccess) { rc = hip_fail(e, "ring upload"); break; }
        if (c.hook(PipeCall::HOOK_ISSUER, k)) { rc = PipeCall::hook_fail("issuer", k); break; }
        const uint64_t seg_bound = (ch.nb / 100 * slack_pct + 99) / SEG + ch.nd + 1;
        s.h_status()[0] = ~0ull;
        if ((rc = ring_enqueue_normalize(b, cs, seg_bound, lo)) != TM_OK) break;
        if ((rc = ring_enqueue_tokenize(b, cs, c.enc, s.d_bytes, s.d_bytes_cap, s.h_status(), &s.ids_at)) != TM_OK) break;
        if ((e = hipEventRecord(s.comp_done, cs)) != hipSuccess) { rc = hip_fail(e, "hipEventRecord"); break; }
        if (trace) fprintf(stderr, "[ring] issue chunk %3zu (%5.1f MiB, %u docs) slot %d at %7.2f ms, %.3f ms of launches\n", k, ch.nb / 1048576.0, ch.nd, si, ti0 - c.t0, now_ms() - ti0);
        issued++;
      }
      { std::lock_guard<std::mutex> g(dv.mu); dv.queue.emplace_back(k, si); }
      dv.cv.notify_all();
    }
    if (rc != TM_OK) {
      // the chunk this thread was enqueuing never reaches the finisher: its upload reads the caller's text and its kernels write a slot's
      // workspace, and neither may outlive the call
      if (enqueued) { (void)hipStreamSynchronize(r.up); for (hipStream_t st : r.comp) (void)hipStreamSynchronize(st); }
      fail_all(rc);
    }
    { std::lock_guard<std::mutex> g(dv.mu); dv.issuer_done = true; }
    dv.cv.notify_all();
  };

  auto finisher = [&](Dev& dv) {
    const tm_vocab* const v = dv.v;
    Ring& r = *dv.r;
    NearDevice near_gpu(v->device);
    int rc = enter_device(v);
    struct Pending { size_t k; uint64_t base; Held slot; };      // the chunk whose download is enqueued, with its slot
    Pending prev{0, 0, nullptr};
    // the downloads of a chunk are through: its offsets and counts to the caller, the slot back to the issuer (a failure leaves the slot with
    // `p`: the issuers hear of the failure first)
    auto complete = [&](Pending& p) -> int {
      RingSlot& s = r.slots[p.slot->si];
      hipError_t e = hipEventSynchronize(s.dl_done);
      if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize (ring download)");
      const PipeCall::Chunk ch = c.chunk(p.k);
      c.place_offsets(ch, p.base, s.h_toff());
      if (c.missing && ch.nd) std::memcpy(c.missing + ch.d0, s.h_missing(), (size_t)ch.nd * 4);
      if (c.stats) { std::lock_guard<std::mutex> g(c.mu); c.stats->normalized_bytes += s.h_status()[2]; }
      p.slot.reset();
      if (trace) fprintf(stderr, "[ring] chunk %3zu complete at %7.2f ms\n", p.k, now_ms() - c.t0);
      return TM_OK;
    };
    // One issued chunk from its verdict to its enqueued download (or through the exact path); `slot` is the caller's, and stays the caller's on
    // every way out but the last line, where the download owns it.  TM_OK without a download: another chunk has failed.
    auto finish = [&](size_t k, Held& slot) -> int {
      bool exact = !slot;
      uint64_t ntok = 0;
      if (slot) {
        RingSlot& s = r.slots[slot->si];
        // (the chunk's verdict: the issuer has set the word to ~0, the chunk's last kernel writes it, and the download stream waits for the
        // event on the device)
        const hipError_t e = wait_verdict(s.h_status(), s.comp_done);
        if (e != hipSuccess) return hip_fail(e, "ring chunk");
        if (c.hook(PipeCall::HOOK_FINISHER, k)) return PipeCall::hook_fail("finisher", k);
        const uint64_t st = s.h_status()[0];
        if (st == ~0ull) return set_error(TM_E_INTERNAL, "a chunk of the ring ended without its verdict");
        if (trace) fprintf(stderr, "[ring] chunk %3zu computed at %7.2f ms: status %llu, %llu ids, %llu segments\n", k, now_ms() - c.t0, (unsigned long long)st,
                           (unsigned long long)s.h_status()[1], (unsigned long long)s.h_status()[3]);
        if (st != 0 || c.hook(PipeCall::HOOK_EXACT, k)) exact = true; else ntok = s.h_status()[1];
      }
      if (exact) {          // (on a borrowed lane: the slot is the issuer's again while the chunk runs there)
        if (c.stats && slot) { std::lock_guard<std::mutex> g(c.mu); c.stats->ring_exact_chunks++; }
        slot.reset();
        return chunk_exact(c, v, k);
      }
      RingSlot& s = r.slots[slot->si];
      uint64_t base = 0;
      if (!c.order(k, ntok, &base)) return TM_OK;
      const uint32_t nd = c.chunk(k).nd;
      const PipeCall::Place out = c.place(base, ntok);
      hipError_t e = hipStreamWaitEvent(r.down, s.comp_done, 0);
      if (e == hipSuccess && out.bytes) e = hipMemcpyAsync(out.at, s.ids_at, out.bytes, hipMemcpyDeviceToHost, r.down);
      if (e == hipSuccess) e = hipMemcpyAsync(s.h_toff(), s.ws->d_tok_offsets, ((uint64_t)nd + 1) * 8, hipMemcpyDeviceToHost, r.down);
      if (e == hipSuccess && c.missing) e = hipMemcpyAsync(s.h_missing(), s.ws->d_doc_missing, (uint64_t)nd * 4, hipMemcpyDeviceToHost, r.down);
      if (e == hipSuccess) e = hipEventRecord(s.dl_done, r.down);
      if (e != hipSuccess) return hip_fail(e, "ring download");
      // (a failure behind the enqueued download: r.down is waited for before the finisher leaves)
      if (c.hook(PipeCall::HOOK_DOWNLOAD, k)) return PipeCall::hook_fail("download", k);
      if (prev.slot) { const int rc = complete(prev); if (rc != TM_OK) return rc; }
      prev = Pending{k, base, std::move(slot)};
      return TM_OK;
    };
    for (;;) {
      std::pair<size_t, int> item;
      { std::unique_lock<std::mutex> lk(dv.mu);
        dv.cv.wait(lk, [&] { return dv.qhead < dv.queue.size() || dv.issuer_done; });
        if (dv.qhead >= dv.queue.size()) break;
        item = dv.queue[dv.qhead++]; }
      Held slot(item.second >= 0 ? new Lease(dv, item.second) : nullptr);
      if (rc != TM_OK || c.failed()) {              // (drain: whatever is in flight ends before the call returns)
        if (slot) (void)hipEventSynchronize(r.slots[slot->si].comp_done);
        continue;
      }
      if ((rc = finish(item.first, slot)) != TM_OK) fail_all(rc);      // (everybody hears of it; then `slot` goes back, and the chunks behind this one are drained)
    }
    if (prev.slot) { if (rc == TM_OK && !c.failed()) { if ((rc = complete(prev)) != TM_OK) fail_all(rc); } else (void)hipEventSynchronize(r.slots[prev.slot->si].dl_done); }
    (void)hipStreamSynchronize(r.down);
  };

  std::vector<std::thread> th;
  for (uint32_t i = 0; i < c.nv; i++) {
    th.emplace_back(finisher, std::ref(*devs[i]));
    if (i > 0) th.emplace_back(issuer, std::ref(*devs[i]));
  }
  issuer(*devs[0]);
  for (auto& t : th) t.join();
  return c.first_error;
}

// borrow the rings of the replicas (all or none) and size their slots for this call; false: somebody else drives one of them
static int rings_acquire(PipeCall& c, uint32_t nslots, uint32_t nstreams, std::vector<Ring*>& rings, bool* got) {
  *got = false;
  uint64_t max_nb = 0; uint32_t max_nd = 0;
  for (size_t k = 0; k < c.nchunks; k++) {
    max_nb = std::max<uint64_t>(max_nb, c.offsets[c.first[k + 1]] - c.offsets[c.first[k]]);
    max_nd = std::max<uint32_t>(max_nd, c.first[k + 1] - c.first[k]);
  }
  for (uint32_t i = 0; i < c.nv; i++) {
    LanePool* p = pool_of(c.vs[i]);
    std::lock_guard<std::mutex> g(p->mu);
    if (p->ring.busy) { for (Ring* r : rings) r->busy = false; rings.clear(); return TM_OK; }      // (a ring's busy flag is only read under its pool's lock; clearing ours without it is safe: nobody else sets it while true)
    p->ring.busy = true;
    rings.push_back(&p->ring);
  }
  int rc = TM_OK;
  for (uint32_t i = 0; i < c.nv && rc == TM_OK; i++) {
    Ring& r = *rings[i];
    if ((rc = enter_device(c.vs[i])) != TM_OK) break;
    hipError_t e = hipSuccess;
    if (!r.up && (e = hipStreamCreateWithFlags(&r.up, hipStreamNonBlocking)) != hipSuccess) { rc = hip_fail(e, "hipStreamCreate (ring)"); break; }
    if (!r.down && (e = hipStreamCreateWithFlags(&r.down, hipStreamNonBlocking)) != hipSuccess) { rc = hip_fail(e, "hipStreamCreate (ring)"); break; }
    while (r.comp.size() < nstreams) {
      hipStream_t st = nullptr;
      if ((e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) { rc = hip_fail(e, "hipStreamCreate (ring)"); break; }
      r.comp.push_back(st);
    }
    if (rc != TM_OK) break;
    if (r.slots.size() < nslots) r.slots.resize(nslots);
    for (RingSlot& s : r.slots) if ((rc = ring_slot_size(s, c.vs[i], lane_need(true, max_nb), max_nd)) != TM_OK) break;
  }
  if (rc != TM_OK) { for (Ring* r : rings) r->busy = false; rings.clear(); return rc; }
  *got = true;
  return TM_OK;
}

static int pipeline_lanes(PipeCall& c);

// The pipeline over the lanes of ONE vocabulary or of its replicas on several devices (tm_tokenize_pipeline_multi, tm_multi.hip): worker w
// borrows a lane of replica w % nv, so the chunks — handed out from one counter — go to whichever lane of whichever device is free, and the
// ids of chunk k land behind those of chunks 0..k-1 wherever they were computed.  `lanes` = lanes per replica.
int tokenize_pipeline_on(const tm_vocab* const* vs, uint32_t nv, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, int raw, uint32_t encoding_length,
                         uint64_t chunk_bytes, uint32_t lanes, uint8_t* bytes_out, uint64_t bytes_cap, uint64_t* byte_offsets, uint32_t* missing,
                         uint32_t* encoding_length_used, tm_pipeline_stats* stats) {
  if (!vs || nv == 0 || !vs[0] || (ndocs && (!offsets || !text)) || !byte_offsets) return set_error(TM_E_INVALID, "null argument");
  const tm_vocab* const v = vs[0];          // (what the replicas have in common: id width)
  if (encoding_length <= 1) encoding_length = v->host.n_ids <= 65536 ? 2 : 3;
  if (encoding_length < 2 || encoding_length > 4) return set_error(TM_E_INVALID, "Invalid encoding length");
  if (encoding_length_used) *encoding_length_used = encoding_length;
  if (ndocs && offsets[0] != 0) return set_error(TM_E_INVALID, "offsets[0] must be 0");
  const bool chunk_default = chunk_bytes == 0;
  if (chunk_default) chunk_bytes = 32ull << 20;
  if (lanes == 0) lanes = 4;
  lanes = std::min<uint32_t>(lanes, 8);
  PipeCall c{vs, nv, text, offsets, ndocs, raw, encoding_length, chunk_bytes, lanes, bytes_out, bytes_cap, byte_offsets, missing, stats};
  c.in_pinned = is_pinned(text); c.out_pinned = is_pinned(bytes_out);
  // the ring: raw text, page-locked buffers on both sides, and a normalizer pass in the one-pass form
  static const int ring_env = env_int("TM_RING", INT_MIN, INT_MAX, 1);
  static const uint32_t ring_slots = (uint32_t)env_int("TM_RING_SLOTS", 2, 16, 4), ring_streams = (uint32_t)env_int("TM_RING_STREAMS", 1, 4, 2);
  static const uint64_t ramp_pct = (uint64_t)env_int("TM_RING_RAMP", 110, 400, 150), ramp_first = (uint64_t)env_int("TM_RING_FIRST_KIB", 64, 1 << 20, 2048) << 10;
  bool use_ring = ring_env != 0 && raw && c.in_pinned && c.out_pinned && ndocs > 0;
  for (uint32_t i = 0; i < nv && use_ring; i++) use_ring = ring_supported(vs[i]);
  // (the ring's chunks: 48 MiB unless the caller says otherwise - every launch of the match kernel has a ramp and a tail of its own, 1 GiB in
  // 27.0 ms against 27.6 with 32 MiB chunks and 28.9 with 24; beyond 48 the first results come later for nothing, profiles/r06_h2h.txt)
  if (use_ring && chunk_default) c.chunk_bytes = chunk_bytes = 48ull << 20;
  for (uint32_t d = 0; d < ndocs; d++) if (offsets[d + 1] < offsets[d]) return set_error(TM_E_INVALID, "offsets not monotone at document %u", d);
  const double t_entry = now_ms();
  chunk_layout(offsets, ndocs, nv, lanes, chunk_bytes, use_ring, ramp_first, ramp_pct, c.first);      // (tm_chunks.h: the ramp and the tail of every call)
  c.nchunks = c.first.size() - 1;
  byte_offsets[0] = 0;
  if (stats) *stats = tm_pipeline_stats{};
  if (c.nchunks == 0) return TM_OK;
  c.tok_base.assign(c.nchunks + 1, 0);
  c.known.assign(c.nchunks + 1, 0);
  c.known[0] = 1;
  c.t0 = now_ms();
  if (debug_flags() & 16777216) c.hook_arm();
  { static const bool trace = getenv("TM_TRACE") != nullptr; if (trace) fprintf(stderr, "[pipe] %zu chunks laid out in %.3f ms (%s)\n", c.nchunks, c.t0 - t_entry, use_ring ? "ring" : "lanes"); }
  if (c.nchunks < 2) use_ring = false;          // (one chunk: the lanes' form is the shorter way)
  int rc = TM_OK;
  uint32_t workers = 0;
  if (use_ring) {
    std::vector<Ring*> rings;
    bool got = false;
    if ((rc = rings_acquire(c, ring_slots, ring_streams, rings, &got)) != TM_OK) return rc;
    if (got) {
      rc = pipeline_ring(c, rings);
      for (uint32_t i = 0; i < nv; i++) { LanePool* p = pool_of(vs[i]); std::lock_guard<std::mutex> g(p->mu); p->ring.busy = false; }
      workers = nv;
      if (stats) stats->ring = 1;
    } else use_ring = false;
  }
  if (!use_ring) { rc = pipeline_lanes(c); workers = (uint32_t)std::min<size_t>((size_t)lanes * nv, c.nchunks); }
  if (rc != TM_OK || c.first_error != TM_OK) return set_error(c.first_error != TM_OK ? c.first_error : rc, "%s", c.first_msg.c_str());
  if (stats) { stats->chunks = (uint32_t)c.nchunks; stats->lanes = workers; stats->input_pinned = c.in_pinned; stats->output_pinned = c.out_pinned; }
  if (byte_offsets[ndocs] > bytes_cap || !bytes_out) return set_error(TM_E_NOSPACE, "bytes_cap %llu < %llu required", (unsigned long long)bytes_cap, (unsigned long long)byte_offsets[ndocs]);
  return TM_OK;
}

// The lanes' form: every worker thread borrows a lane and takes chunk after chunk through it - upload, tm_batch_normalize (one wait), the
// tokenizer (one wait for the id count), the download (one wait).  For pageable buffers, already-normalized text, vocabularies whose
// normalizer is not the one-pass form, and callers that find the ring taken.
static int pipeline_lanes(PipeCall& c) {
  const uint32_t nworkers = (uint32_t)std::min<size_t>((size_t)c.lanes * c.nv, c.nchunks);
  const bool raw = c.raw != 0;
  // A lane works on one chunk at a time, but the raw text of its NEXT chunk is uploaded (on the lane's second stream) as soon as the
  // normalizer pass of the current one is through with the raw buffer: the H2D of chunk k+1 hides behind the tokenizer kernels of chunk k.
  static const bool trace = getenv("TM_TRACE") != nullptr;
  auto worker = [&](uint32_t wi) {
    const tm_vocab* const v = c.vs[wi % c.nv];
    NearDevice near_gpu(v->device);             // (worker 0 is the calling thread: it gets its affinity back when the call returns)
    Lane* l = nullptr;
    int rc = lane_acquire(v, &l);
    std::vector<uint64_t> loc, loc_next, toff;
    if (rc == TM_OK && !l->up_stream) {
      hipError_t e = hipStreamCreateWithFlags(&l->up_stream, hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&l->up_done, hipEventDisableTiming);
      if (e != hipSuccess) rc = hip_fail(e, "hipStreamCreate (lane upload)");
    }
    // the chunk with its offsets `lo` uploaded on `st`; *srcp = where the text was read from (chunk_text; for a retry)
    auto upload = [&](const PipeCall::Chunk& ch, const std::vector<uint64_t>& lo, hipStream_t st, const uint8_t** srcp) -> int {
      const int r = chunk_text(c, l, ch, srcp);
      return r != TM_OK ? r : lane_upload(l, v, *srcp, lo.data(), ch.nd, raw, st);
    };
    size_t k = rc == TM_OK ? c.next.fetch_add(1) : c.nchunks;
    bool prefetched = false;
    const uint8_t* src = nullptr;
    while (rc == TM_OK && k < c.nchunks) {
      if (c.failed()) break;
      const PipeCall::Chunk ch = c.chunk(k);
      const double tr0 = trace ? now_ms() : 0;
      double tr1 = 0, tr2 = 0, tr3 = 0;
      if (prefetched) {
        hipError_t e = hipStreamWaitEvent(l->stream, l->up_done, 0);
        if (e != hipSuccess) { rc = hip_fail(e, "hipStreamWaitEvent"); break; }
      } else {
        loc.resize((size_t)ch.nd + 1);
        ch.local_offsets(loc.data());
        if ((rc = upload(ch, loc, l->stream, &src)) != TM_OK) break;
      }
      size_t k_next = c.nchunks;
      bool next_up = false;
      const uint8_t* src_next = nullptr;
      auto prefetch = [&]() -> int {
        k_next = c.next.fetch_add(1);
        if (k_next >= c.nchunks || !raw) return TM_OK;
        const PipeCall::Chunk nx = c.chunk(k_next);
        // (a chunk that would replace the workspace, or the per-document arrays the current chunk still reads, is uploaded later)
        if (!l->ws || l->ws->max_bytes < lane_need(true, nx.nb) || l->ws->max_docs < nx.nd || (uint64_t)nx.nd + 2 > l->ws->raw_docs_cap) return TM_OK;
        loc_next.resize((size_t)nx.nd + 1);
        nx.local_offsets(loc_next.data());
        if (raw_upload_replaces_buffers(l->ws, loc_next.data(), nx.nd)) return TM_OK;       // (the slabs and piece offsets of the current chunk are read by its match kernel)
        int r = upload(nx, loc_next, l->up_stream, &src_next);
        if (r != TM_OK) return r;
        hipError_t e = hipEventRecord(l->up_done, l->up_stream);
        if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
        next_up = true;
        return TM_OK;
      };
      RunOut ro;
      if (trace) tr1 = now_ms();
      if ((rc = lane_compute(l, v, src, loc.data(), ch.nd, raw, true, &ro, prefetch)) != TM_OK) break;
      if (c.hook(PipeCall::HOOK_EXACT, k)) { rc = PipeCall::hook_fail("exact", k); break; }
      if (trace) tr2 = now_ms();
      if (k_next == c.nchunks && !next_up) k_next = c.next.fetch_add(1);          // (already-normalized input: nothing was prefetched)
      bool delivered = false;
      if ((rc = chunk_deliver(c, l, k, ro.total_tokens, true, toff, &delivered, trace ? &tr3 : nullptr)) != TM_OK || !delivered) break;
      if (trace) fprintf(stderr, "[pipe] worker %u chunk %3zu (%5.1f MiB): start %7.2f  upload/wait %5.2f  compute %5.2f  order-wait %5.2f  download %5.2f  -> end %7.2f ms\n", wi, k,
                         ch.nb / 1048576.0, tr0 - c.t0, tr1 - tr0, tr2 - tr1, tr3 - tr2, now_ms() - tr3, now_ms() - c.t0);
      k = k_next;
      prefetched = next_up;
      if (next_up) { loc.swap(loc_next); src = src_next; }
    }
    if (l && l->up_stream) (void)hipStreamSynchronize(l->up_stream);          // (an error may leave an upload in flight)
    if (rc != TM_OK) c.fail(rc);
    if (rc != TM_OK && l) lane_quiet(l, rc);          // (... or a download, or small transfers into this thread's own arrays)
    if (l) lane_release(v, l);
  };
  std::vector<std::thread> th;
  for (uint32_t t = 1; t < nworkers; t++) th.emplace_back(worker, t);
  worker(0);
  for (auto& t : th) t.join();
  return c.first_error;
}
}  // namespace tmh
extern "C" {

// Decode / decode_raw (go/tokenmonster.go:445-550; tokenmonster.cpp:1404-1425) on a lane like the tokenize entry points: the lane's
// stream, grow-only device arenas and pinned staging — steady state allocates nothing and stays off the NULL stream, so decode jobs of a
// server (tokenmonsterserver jobs 2-9) do not stall the tokenize jobs running beside them (a hipFree synchronizes the whole device).
static thread_local uint32_t g_decode_host_docs = 0;
uint32_t tm_decode_host_docs(void) { return g_decode_host_docs; }

int tm_decode_batch(const tm_vocab* v, const uint32_t* tokens, const uint64_t* tok_offsets, uint32_t ndocs, int raw,
                    uint8_t* out, uint64_t out_cap, uint64_t* out_offsets) {
  g_decode_host_docs = 0;
  if (!v || !tok_offsets || !out_offsets) return set_error(TM_E_INVALID, "null argument");
  const uint64_t n = tok_offsets[ndocs];
  if (n && !tokens) return set_error(TM_E_INVALID, "null argument");
  if (tok_offsets[0] != 0) return set_error(TM_E_INVALID, "tok_offsets[0] must be 0");
  for (uint32_t d = 0; d < ndocs; d++) if (tok_offsets[d + 1] < tok_offsets[d]) return set_error(TM_E_INVALID, "tok_offsets not monotone");
  Lane* l = nullptr;
  int rc = lane_acquire(v, &l);
  if (rc != TM_OK) return rc;
  hipStream_t st = l->stream;
  hipError_t e = hipSuccess;
  const bool dev_capcode = !raw && v->host.capcode == 2 && v->host.charset == 1 && ndocs > 0;
  // arena A: ids | document offsets | the decode's own words (dec_arena: tiles of ids, byte offset / decoded length of every document)
  const auto up = dec_up;
  const uint64_t o_tok = 0, o_toff = o_tok + up((n + 1) * 4);
  const DecArena a = dec_arena(o_toff + up(((uint64_t)ndocs + 1) * 8), n, ndocs);
  const uint64_t a_bytes = a.bytes;
  std::vector<uint64_t> doff((size_t)ndocs + 1, 0), declen;
  uint64_t total = 0;
  bool need_raw = !dev_capcode;
  const uint8_t *h_dec = nullptr, *h_raw = nullptr;          // decoded / raw bytes in the lane's pinned staging
  do {
    if ((rc = lane_device(&l->d_dec_a, &l->d_dec_a_cap, a_bytes, "hipMalloc (decode)")) != TM_OK) break;
    uint8_t* A = l->d_dec_a;
    uint32_t* d_tok = (uint32_t*)(A + o_tok); uint64_t* d_toff = (uint64_t*)(A + o_toff);
    uint64_t* d_total = (uint64_t*)(A + a.o_total); uint64_t* d_doff = (uint64_t*)(A + a.o_doff); uint64_t* d_declen = (uint64_t*)(A + a.o_declen);
    // ids and offsets through pinned staging (the caller's buffers are pageable Go / Python memory)
    const uint64_t in_bytes = n * 4 + ((uint64_t)ndocs + 1) * 8;
    if ((rc = lane_pinned(&l->h_stage_in, &l->h_in_cap, in_bytes)) != TM_OK) break;
    std::memcpy(l->h_stage_in, tok_offsets, ((uint64_t)ndocs + 1) * 8);
    if (n) std::memcpy(l->h_stage_in + ((uint64_t)ndocs + 1) * 8, tokens, n * 4);
    if ((e = hipMemcpyAsync(d_toff, l->h_stage_in, ((uint64_t)ndocs + 1) * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (n && (e = hipMemcpyAsync(d_tok, l->h_stage_in + ((uint64_t)ndocs + 1) * 8, n * 4, hipMemcpyHostToDevice, st)) != hipSuccess)) { rc = hip_fail(e, "H2D tokens"); break; }
    launch_decode_lengths(v, d_tok, n, d_toff, ndocs, a, A, st);
    if ((rc = lane_pinned(&l->h_stage, &l->h_cap, 8)) != TM_OK) break;
    if ((rc = d2h(l->h_stage, d_total, 8, st, "decode lengths")) != TM_OK) break;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) { rc = hip_fail(e, "hipStreamSynchronize"); break; }
    std::memcpy(&total, l->h_stage, 8);
    // arena B: the gathered bytes | the same after capcode decoding (out of place: the host decoder needs the others as they were)
    const uint64_t o_dec = up(total + 16);
    if ((rc = lane_device(&l->d_dec_b, &l->d_dec_b_cap, o_dec + up(total + 16), "hipMalloc (decode output)")) != TM_OK) break;
    uint8_t* d_out = l->d_dec_b; uint8_t* d_dec = l->d_dec_b + o_dec;
    launch_decode_copy(v, d_tok, n, d_toff, ndocs, a, A, d_out, st);
    if (dev_capcode) {
      if ((rc = launch_decode_capcode(v, d_out, d_doff, ndocs, d_dec, d_declen, d_total + 8, st)) != TM_OK) break;
      declen.resize(ndocs);
    }
    // staging: the documents' byte offsets (they come out of the gather) | decoded lengths | decoded text | gathered bytes
    const uint64_t s_doff = 0, s_declen = up(((uint64_t)ndocs + 1) * 8), s_text = s_declen + up((uint64_t)ndocs * 8 + 8), s_raw = s_text + up(total + 16);
    if ((rc = lane_pinned(&l->h_stage, &l->h_cap, s_raw + up(total + 16))) != TM_OK) break;
    if ((rc = d2h(l->h_stage + s_doff, d_doff, ((uint64_t)ndocs + 1) * 8, st, "decode offsets")) != TM_OK) break;
    if (dev_capcode) {
      uint8_t* hp = l->h_stage + s_text;
      if ((rc = d2h(l->h_stage + s_declen, d_declen, (uint64_t)ndocs * 8, st, "D2H decoded text")) != TM_OK || (rc = d2h(hp, d_dec, total, st, "D2H decoded text")) != TM_OK) break;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) { rc = hip_fail(e, "hipStreamSynchronize"); break; }
      std::memcpy(declen.data(), l->h_stage + s_declen, (uint64_t)ndocs * 8);
      h_dec = hp;
      for (uint32_t d = 0; d < ndocs && !need_raw; d++) need_raw = declen[d] == DEC_HOST;
      if (need_raw) {
        uint8_t* hr = l->h_stage + s_raw;
        if ((rc = d2h(hr, d_out, total, st, "D2H decoded bytes")) != TM_OK) break;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) { rc = hip_fail(e, "hipStreamSynchronize"); break; }
        h_raw = hr;
      }
    } else {
      if ((rc = d2h(l->h_stage + s_raw, d_out, total, st, "D2H decoded bytes")) != TM_OK) break;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) { rc = hip_fail(e, "hipStreamSynchronize"); break; }
      h_raw = l->h_stage + s_raw;
    }
    std::memcpy(doff.data(), l->h_stage + s_doff, doff.size() * 8);
  } while (false);
  if (rc != TM_OK) (void)hipStreamSynchronize(st);      // nothing of this call may still be in flight when the lane goes back
  // (the documents the device left alone - anything it does not decode; every document of a capcode-1 or UTF-16 vocabulary - go through the host decoder there)
  if (rc == TM_OK) rc = decode_assemble(v, raw != 0, ndocs, doff.data(), total, h_raw, h_dec, dev_capcode ? declen.data() : nullptr, out, out_cap, out_offsets, &g_decode_host_docs);
  lane_release(v, l);
  return rc;
}

}  // extern "C"

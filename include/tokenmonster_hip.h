/* tokenmonster_hip.h — C ABI of libtokenmonster_hip.so: MI355X (gfx950) batch tokenizer for
 * TokenMonster vocabularies.  This is the drop-in boundary for ONE path of the reference:
 * the 6-branch ungreedy longest-match loop, go/tokenmonster.go:1017-1279 (Vocab.tokenize) and its
 * copies (:1281 count, :1545/:1817/:2089 serialized, training/trainvocab.go:925-1176 scoring).
 *
 * The reference has no FFI of its own; the seams this library replaces are
 *   (*Vocab).Tokenize / Count / TokenizeToSerialized      go/tokenmonster.go:959, :971, :986
 *   tokenmonsterserver job 1 / job 20 goroutine fan-out   training/tokenmonsterserver.go:363-378, :773-787
 *   trainvocab worker inner loop                          training/trainvocab.go:925-1176
 *   Load (table upload; .vocab layout)                    go/tokenmonster.go:2656-2736
 * INTEGRATION.md shows the cgo stub a maintainer adds on the Go side for each entry point.
 *
 * Conventions: extern "C", plain pointers and sizes.  Every host pointer is borrowed for the
 * duration of the call only (cgo pointer-passing rule).  Every function returns TM_OK (0) or a
 * negative TM_E_* code; tm_last_error() gives a thread-local message.  There is NO CPU fallback
 * inside this library: if no gfx950 device is usable the call fails (TM_E_NODEVICE) and the Go
 * side keeps using its own vocab.tokenize.
 *
 * Input text is ALREADY NORMALIZED bytes (what go/tokenmonster.go:963 `normalize` returns), unless
 * stated otherwise.  The look-ahead pad byte is 0 (tokenmonster-cpp/src/tokenmonster.cpp:1724-1726).
 */
#ifndef TOKENMONSTER_HIP_H
#define TOKENMONSTER_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TM_OK 0
#define TM_E_INVALID (-1)   /* bad argument / malformed .vocab */
#define TM_E_NODEVICE (-2)  /* no usable gfx950 device */
#define TM_E_HIP (-3)       /* a HIP runtime call failed */
#define TM_E_NOSPACE (-4)   /* caller buffer too small; required size reported via out-params */
#define TM_E_LIMIT (-5)     /* input exceeds a documented limit (batch bytes, trie nodes) */
#define TM_E_INPUT (-6)     /* the walk cannot advance on this text with this vocabulary (the reference loops forever on it: a UTF-16
                               vocabulary with one-byte keys beside the delete token); nothing is wrong with the device */

#define TM_E_INTERNAL (-7)  /* the pipeline's stages disagree with each other (the emit stage met a transition the match stage never wrote): a fault
                               of this library, never of the input.  Callers that fall back to the CPU path on errors may do so here; on TM_E_INPUT they
                               must NOT (the reference's own walk does not terminate on that input) */

#define TM_NONE 0xFFFFFFu   /* go/tokenmonster.go:32 DOES_NOT_EXIST */

typedef struct tm_vocab tm_vocab;     /* immutable device-resident vocabulary tables */
typedef struct tm_batch tm_batch;     /* reusable device workspace for one batch of documents */
typedef struct tm_dataset tm_dataset; /* device-resident normalized dataset for the scoring pass */
typedef struct tm_decoder tm_decoder; /* streaming Decoder: per-connection host state */
typedef struct tm_encoder tm_encoder; /* streaming encoder: one document piece by piece; a stream and a device workspace of its own */

const char* tm_last_error(void);
int tm_device_count(void);
/* Select the HIP device used by the calling thread's subsequent calls. */
int tm_set_device(int device);

/* ---- vocabulary: replaces Load's table construction (go/tokenmonster.go:2656-2736) ------------ */
/* Parses the bytes of a .vocab file (layout: SURVEY.md Appendix A), builds the longest-match
 * index and per-record rows, uploads them to the current device's HBM. */
int tm_vocab_load(const uint8_t* vocab_file, size_t n, tm_vocab** out);
/* The same on a named device: tm_set_device's "current device" belongs to the calling OS thread, which a goroutine under cgo does not own. */
int tm_vocab_load_on(const uint8_t* vocab_file, size_t n, int device, tm_vocab** out);
/* Batches, decoders and lanes of the vocabulary must not be used afterwards.  Kernels that an asynchronous entry point (tm_batch_run on a
 * caller's stream, tm_score_device, tm_score_finish ...) has already launched may still be in flight: tm_vocab_free waits for them (an
 * event per stream the tables were used on - this vocabulary's work only, not the device as hipFree would) and then parks the device
 * memory for the next tm_vocab_load.  A caller's stream on which this vocabulary's kernels were launched must still exist at this point. */
void tm_vocab_free(tm_vocab* v);
/* OPTIONAL, for large vocabularies (tables of 10 MB and more against the 4 MB of L2 an XCD has): lays the tables out by USE.  The match
 * kernel's table walk is replayed on the host over `normalized_sample` (text as tm_normalize writes it; a few MiB of what the vocabulary
 * will be used on), the trie's nodes are renumbered - most used first, so that the rows, space-prefix links and suffix links that are
 * gathered most share cache lines - and the tables are written again into the device block they lie in.  Token ids and every result are
 * unchanged (only internal node numbers move); nothing else of this vocabulary may run meanwhile, and the call waits for what already does.
 * Not for vocabularies made by tm_vocab_block_import (no records).  Cost: about as long as loading the vocabulary + 0.2 s per MiB of sample. */
int tm_vocab_tune(tm_vocab* v, const uint8_t* normalized_sample, uint64_t n);
/* tm_vocab_load + tm_vocab_tune in one: the caller hands a sample of normalized text with the file and the tables are built for the device once,
 * laid out by use from the start (current device; sample_n == 0: plain tm_vocab_load).  Measured on one MI355X, 1 GiB (profiles/r06_tuned_tables.txt):
 * match kernel -1 % with 32 000 ids (6 MB of tables), -5 % with 100 256 ids (16 MB) and on the 65 536-id scoring pass. */
int tm_vocab_load_sample(const uint8_t* vocab_file, size_t n, const uint8_t* normalized_sample, uint64_t sample_n, tm_vocab** out);
/* The device block of a vocabulary from process to process (the data-parallel scoring mode: ONE rank builds a candidate's tables, the others
 * take the finished block - e.g. as the destination of an RCCL broadcast - instead of repeating tm_build_vocab + tm_vocab_load).
 * tm_vocab_block_export describes the block of `v` (plain data: send it as bytes) and returns its device pointer; tm_vocab_block_import makes
 * an empty vocabulary of that shape on `device` and returns the device pointer the caller has to fill with the exporter's `bytes` bytes
 * before the first use.  An imported vocabulary tokenizes, counts, scores and decodes on the device; it has no host tables (tm_vocab_image /
 * tm_vocab_save and the streaming decoder fail). */
typedef struct tm_vocab_block {
  uint64_t bytes;            /* bytes the tables occupy from the block's start (what has to be sent) */
  uint64_t part_bytes[8];    /* root, walk tables, rows, space-prefix links, node values, reverse offsets, reverse bytes, begin_byte */
  uint32_t idle_off, n_da, n_info, max_len, off, bstart, spl_hint, link_off, direct_off, delete_id, unk_id;
  uint32_t n_ids, vocab_size, capcode, charset, norm_flag, level, reserve, n_nodes, pad;   /* pad: TM_VOCAB_BLOCK_FORMAT of the exporting build */
} tm_vocab_block;
#define TM_VOCAB_BLOCK_FORMAT 6u   /* layout of the device tables inside a block (tm_tables.h); an importer refuses any other */
int tm_vocab_block_export(const tm_vocab* v, tm_vocab_block* meta, void** device_ptr);
int tm_vocab_block_import(const tm_vocab_block* meta, int device, tm_vocab** out, void** device_ptr);
/* Synchronous device-to-device copy (also between two devices of the node with peer access), for callers that have no HIP binding of
 * their own: e.g. to fill an imported block from the exporter's pointer inside one process. */
int tm_device_copy(void* dst_device, const void* src_device, uint64_t bytes);
uint32_t tm_vocab_size(const tm_vocab* v);             /* go :2477 Len()              */
uint32_t tm_vocab_n_info(const tm_vocab* v);           /* index records incl. "D " duplicates */
uint32_t tm_vocab_n_ids(const tm_vocab* v);            /* len(reverse) = highest ID + 1 */
uint32_t tm_vocab_max_token_length(const tm_vocab* v); /* go :2498                    */
uint32_t tm_vocab_capcode(const tm_vocab* v);          /* go :2390                    */
uint32_t tm_vocab_charset(const tm_vocab* v);
uint32_t tm_vocab_normalization(const tm_vocab* v);    /* normalizer flag byte        */
uint32_t tm_vocab_unk(const tm_vocab* v);              /* unk id or TM_NONE           */
uint32_t tm_vocab_delete_token(const tm_vocab* v);     /* deleteToken id or TM_NONE   */
uint64_t tm_vocab_device_bytes(const tm_vocab* v);     /* HBM held by the tables      */

/* ---- batch tokenize, host buffers: drop-in for the goroutine fan-out ------------------------- */
/* Tokenizes `ndocs` independent documents.  Document d is text[offsets[d] .. offsets[d+1]).
 * tokens_out receives all IDs, document after document; tok_offsets[ndocs+1] the prefix sums;
 * missing[d] the count go/tokenmonster.go:1274 returns.  If tokens_cap is too small nothing is
 * written to tokens_out, tok_offsets IS filled (so tok_offsets[ndocs] is the required capacity)
 * and TM_E_NOSPACE is returned.  Equivalent of calling Vocab.tokenize on each document. */
int tm_tokenize_batch(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs,
                      uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* tok_offsets, uint32_t* missing);

/* Same walk, counts only: go/tokenmonster.go:1281 tokenizeCount semantics (b-branches count 1,
 * quirk Q2).  counts[ndocs], missing[ndocs]. */
int tm_count_batch(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs,
                   uint64_t* counts, uint32_t* missing);

/* Vocab.Count on RAW text (go :971: normalize, then tokenizeCount): what tokenmonsterserver job 20 calls per document
 * (training/tokenmonsterserver.go:753-800).  The normalization runs on the device. */
int tm_count_batch_raw(const tm_vocab* v, const uint8_t* raw, const uint64_t* offsets, uint32_t ndocs,
                       uint64_t* counts, uint32_t* missing);

/* TokenizeToSerialized (go/tokenmonster.go:986): encoding_length 2, 3 or 4 bytes little-endian per
 * ID (0 = auto: 2 if n_ids <= 65536 else 3, go :990-996).  bytes_out/byte_offsets as above. */
int tm_tokenize_batch_serialized(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs,
                                 uint32_t encoding_length, uint8_t* bytes_out, uint64_t bytes_cap,
                                 uint64_t* byte_offsets, uint32_t* missing, uint32_t* encoding_length_used);

/* ---- large batches, host to host --------------------------------------------------------------------------------- */
/* The three calls above borrow one LANE of the vocabulary (a HIP stream + a grow-only device workspace): steady state does
 * no allocation and never touches the NULL stream, and concurrent callers (cgo calls run on distinct OS threads) take
 * different lanes and overlap on the device; at most TM_LANES (environment, default 8) calls run at once, further callers wait.
 *
 * tm_tokenize_pipeline is the large-batch form of Vocab.TokenizeToSerialized over many documents: the corpus is cut into
 * chunks of whole documents (about chunk_bytes, 0 = 32 MiB; the first two are smaller) that run H2D | normalize + tokenize + serialize | D2H on `lanes`
 * lanes at once (0 = 4): a lane uploads its next chunk while the current one computes, so that PCIe moves text in and ids out behind the kernels.  raw != 0: text is
 * RAW UTF-8 and is normalized on the device (go/tokenmonster.go:242-253); raw == 0: already normalized.  Output: ids of all
 * documents back to back, encoding_length bytes each, little-endian (0 = automatic, go :990-996); byte_offsets[ndocs+1] is
 * always filled, so on TM_E_NOSPACE byte_offsets[ndocs] is the capacity required.  Buffers from tm_host_alloc (or registered
 * with tm_host_register) are DMA'd directly; pageable buffers go through pinned staging at memcpy speed. */
typedef struct tm_pipeline_stats {
  uint32_t chunks, lanes;
  int input_pinned, output_pinned;
  uint64_t normalized_bytes;
  uint32_t host_fallback_docs;
  uint32_t ring;              /* 1: the call ran on the ring (raw text, page-locked buffers on both sides: no host round trip inside a chunk) */
  uint32_t ring_exact_chunks; /* chunks the ring handed to the exact path (documents for the host normalizer, a long document ...) */
} tm_pipeline_stats;
int tm_tokenize_pipeline(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, int raw,
                         uint32_t encoding_length, uint64_t chunk_bytes, uint32_t lanes, uint8_t* bytes_out, uint64_t bytes_cap,
                         uint64_t* byte_offsets, uint32_t* missing, uint32_t* encoding_length_used, tm_pipeline_stats* stats);
/* Page-locked host memory for the buffers of tm_tokenize_pipeline (hipHostMalloc / hipHostRegister).  hipHostMalloc places it on the NUMA
 * node nearest to the current device; the pipeline's worker threads (the calling thread included, for the length of the call) run on that
 * node's CPUs (TM_NUMA=0 in the environment: leave the threads where they are).  tm_device_numa_node: the node of a device's PCIe root as
 * /sys/bus/pci/devices/<bdf>/numa_node gives it, -1 if the host does not say - what a caller pins its own feeding threads to. */
int tm_device_numa_node(int device);
void* tm_host_alloc(size_t bytes);
void tm_host_free(void* p);
int tm_host_register(void* p, size_t bytes);
int tm_host_unregister(void* p);

/* ---- batch tokenize, device-resident: what bench.py times ------------------------------------ */
/* A tm_batch owns device buffers sized for up to max_bytes of text in up to max_docs documents. */
int tm_batch_create(const tm_vocab* v, uint64_t max_bytes, uint32_t max_docs, tm_batch** out);
void tm_batch_free(tm_batch* b);
/* H2D of packed text + offsets (synchronous). */
int tm_batch_upload(tm_batch* b, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs);
/* Raw (un-normalized) input: H2D of packed raw UTF-8 documents, then tm_batch_normalize runs the pre-step of
 * Tokenize (go/tokenmonster.go:242-253: norm.Normalize + capcode.Encode) ON THE DEVICE into the batch's text buffer
 * (max_bytes of tm_batch_create must cover the normalized size, about 1.1x raw with capcode 2).  The device pass handles ASCII, every
 * two-byte script (U+0080..U+07FF: accented Latin, Greek, Cyrillic, Armenian, Hebrew, Arabic ...: NFD, case and capcode from a table the
 * host normalizer fills), Latin Extended Additional under NFD (U+1E00..U+1EFF, what Vietnamese adds: a letter and one or two marks each), the
 * three-byte characters the normalizer leaves alone (General Punctuation, CJK ideographs, kana, symbols), the voiced kana under NFD (a kana and
 * U+3099 / U+309A each: Japanese text), Hangul syllables (decomposed by arithmetic) and the four-byte characters of caseless, NFD-stable blocks
 * (emoji, symbols, plane-2 ideographs), the three-byte combining marks of U+0800..U+1FFF where they stand in canonical order (virama, nukta, the
 * Thai tone marks ...: Hindi, Thai) and the three-byte decimal digits and lower-case letters (Georgian); documents with anything else (cased scripts beyond the BMP, a capital
 * without a lower-case form - U+03D2..U+03D4 -, a character of three bytes that NFD splits in three, marks out of canonical order or behind a character that
 * ends in one of its own, malformed UTF-8) are normalized by the host normalizer inside the same call, from their original
 * bytes; tm_batch_host_fallback_docs reports how many.  (TM_NORM_WG_PER_CU in the environment: the grid of the pass, workgroups per compute
 * unit, default 64 - a tuning knob, profiles/r05_issue_model.txt.)
 * Supported: capcode 0 and 2 (level 1 has no statement in the reference tree and is refused) and every normalization flag
 * (training/README.md:110-123) ON THE DEVICE: NFD and lowercase in the pass itself; quotemarks, collapse, trim, leadingspace and unixlines -
 * and what accents does to the two-byte characters - in a filter pass in front of it that states the reference's in-place loops
 * (tokenmonster.cpp:245-425) per byte, their quirks included (tm_norm.hip: k_pf_*: a wavefront per document, one sweep; one more trip to the
 * host, for the count of the filtered documents' pieces; ~1.7 ms per GiB on top of the pass).  tm_batch_normalize synchronizes `stream`; afterwards tm_batch_run tokenizes the normalized
 * documents.  (Where the normalized text lies between the two calls is the library's business: when every document was normalized on the
 * device it stays in the normalizer's per-piece slabs and the match kernel reads it from there - no packing pass; tm_batch_download_text
 * packs it on request and returns it in document order either way.) */
int tm_batch_upload_raw(tm_batch* b, const uint8_t* raw, const uint64_t* raw_offsets, uint32_t ndocs);
int tm_batch_normalize(tm_batch* b, void* stream);
uint64_t tm_batch_normalized_bytes(const tm_batch* b);
uint32_t tm_batch_host_fallback_docs(const tm_batch* b);
int tm_batch_download_text(tm_batch* b, uint8_t* text_out, uint64_t text_cap, uint64_t* offsets_out);
/* Runs the whole device pipeline (segments, match+branch+link, resolve, scan, emit) on `stream` (a hipStream_t, NULL =
 * default stream).  Inputs and outputs stay in HBM.  Asynchronous with respect to the host. */
int tm_batch_run(tm_batch* b, void* stream);
/* As tm_batch_run but brackets every kernel with HIP events on `stream` and returns per-kernel
 * milliseconds in ms[TM_NUM_KERNELS] (synchronizes). */
#define TM_NUM_KERNELS 5
int tm_batch_run_timed(tm_batch* b, void* stream, float* ms);
const char* tm_kernel_name(int k);
/* Test hooks: sets the switches and returns the previous value; flags < 0 only queries.  Every bit forces a rarely taken path of
 * the product with the SAME results, so that the tests can cover it: 6 = dense T(p,1) array for every segment, 8 = per-lane
 * normalizer kernel instead of k_norm_emit2, 10 = K4 tile walk that stores every id directly (its overflow path), 11 = the device normalizer packs its text
 * (the path of a batch with host-normalized documents) instead of leaving it in its slabs for the match kernel, 12 = group tree of
 * long documents with fan-out 4 from 9 segments on, 13 = 64 KiB mailbox for the small host <-> device transfers, 14 = the last member of tm_score_multi gives up
 * after the members' first meeting (an error path: the call must return that member's error), 15 = the id-staging form of the K4 walk (what vocabularies
 * of more than 65 536 ids use) for the two-plane rows too, instead of the position-staging form, 16 = accepted, without effect (it split the segment kernel of a chunk of the
 * host-to-host ring in two while the batch path had two; there is one launch for every caller now), 24 = ONE chunk of a
 * tm_tokenize_pipeline / tm_tokenize_pipeline_multi call fails with TM_E_INPUT at a place of the host code (an error path: the call must
 * return that error, with nothing of it left in flight and the handle as good as before).  Which one is read from the environment when such a
 * call begins, and only while the bit is set: TM_TEST_FAIL="<place>:<chunk>" or "<place>:<chunk>:<chunks>" (the latter: only a call that
 * has that many chunks, so that a second caller beside it is left alone), place = finisher (the ring's finisher takes the chunk's verdict
 * for a failure), exact (the exact path fails for the chunk - the ring sends it there first; the lanes' form: its compute step), issuer (the
 * ring's issuer fails behind the chunk's enqueued upload) or download (behind the enqueued download of the chunk's ids).  Nothing on the device
 * differs.  Other bits are
 * ignored (a -DTM_DEVEL build, tools/ only, adds profiling bits that switch phases of the match kernel off).  The switches are process-wide,
 * so they are armed only in a process started with TM_TEST_HOOKS in its environment (the test suite, bench.py --also-flags): anywhere
 * else the call changes nothing and returns 0 - one caller of a server cannot change the code path under the others. */
int tm_debug_flags(int flags);
/* Totals of the last run (synchronizes the stream used by the last run). */
int tm_batch_totals(tm_batch* b, uint64_t* total_tokens, uint64_t* total_missing);
/* D2H of results of the last run. */
int tm_batch_download(tm_batch* b, uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* tok_offsets,
                      uint32_t* missing);
/* Raw device pointers of the last run's results (valid until the next run/free).  The id buffer starts at max_bytes / 2 + 2 * max_docs
 * + 1024 ids and grows on demand: call tm_batch_totals (or tm_batch_download) after tm_batch_run and BEFORE fetching these pointers —
 * it synchronizes, and if the run produced more ids than the buffer held it reallocates the buffer and repeats the emit stage, so a
 * pointer fetched earlier may dangle and ids beyond the old capacity were not written. */
const uint32_t* tm_batch_device_tokens(const tm_batch* b);
const uint64_t* tm_batch_device_tok_offsets(const tm_batch* b);
uint64_t tm_batch_device_bytes(const tm_batch* b);

/* ---- decode: Decode / decode_raw (go/tokenmonster.go:445-550; tokenmonster.cpp:1404-1425) ------------------------ */
/* ids of document d = tokens[tok_offsets[d] .. tok_offsets[d+1]).  The gather of reverse[id] (byte counts of tiles of 2048 ids -> scan -> gather
 * through LDS) runs on the device; ids >= tm_vocab_n_ids are skipped.  raw != 0: the concatenated token bytes as they are
 * (decode_raw); raw == 0: capcode decoding (javascript/tokenmonster.js:1007-1065) follows — on the device for the documents of a capcode-2
 * UTF-8 vocabulary made of ASCII, the two-byte scripts (U+0080..U+07FF), the three-byte characters without case (punctuation, CJK, kana,
 * Hangul, symbols) and the four-byte characters of blocks that are caseless throughout (emoji, symbols, the ideographs of plane 2); on the
 * host for documents with a letter whose upper-case form has another length, a three- or four-byte letter with case or malformed UTF-8, and
 * for capcode 1.  tm_decode_host_docs(): how many documents of the calling thread's last tm_decode_batch went to the host decoder.
 * out_offsets[ndocs+1] is always filled; TM_E_NOSPACE if out_cap is too small (required size in out_offsets[ndocs]).
 * Like the tokenize entry points the call borrows a lane of the vocabulary (its stream, grow-only device arenas and pinned
 * staging): callable concurrently, no allocation in steady state, nothing on the NULL stream. */
int tm_decode_batch(const tm_vocab* v, const uint32_t* tokens, const uint64_t* tok_offsets, uint32_t ndocs, int raw,
                    uint8_t* out, uint64_t out_cap, uint64_t* out_offsets);
uint32_t tm_decode_host_docs(void);
/* The same on the ids a batch HOLDS after tm_batch_run, device-resident: ids in HBM -> text in HBM, in grow-only buffers of the batch (what
 * bench.py --workload decode times; a service that detokenizes what it has just tokenized never moves the ids over the host link).
 * Synchronizes `stream`.  *decoded_bytes: bytes of the documents the device decoded; *host_docs: documents it left to the host decoder
 * (those are decoded by tm_batch_decoded_download, which returns every document's text in document order - out_offsets[ndocs+1] always
 * filled, TM_E_NOSPACE with the size required in out_offsets[ndocs] if out_cap is too small). */
int tm_batch_decode(tm_batch* b, int raw, void* stream, uint64_t* decoded_bytes, uint32_t* host_docs);
/* ... with HIP events on `stream` around its stages: ms[0] byte counts of the tiles + scan, ms[1] the gather of the tokens' bytes and the documents'
 * offsets (k_dec_gather), ms[2] capcode decoding (k_dec_capcode; 0 when that is not the device's) - what bench.py's decode line prices its roofline on */
int tm_batch_decode_timed(tm_batch* b, int raw, void* stream, uint64_t* decoded_bytes, uint32_t* host_docs, float* ms);
int tm_batch_decoded_download(tm_batch* b, uint8_t* out, uint64_t out_cap, uint64_t* out_offsets);

/* ---- fixed-shape id tensors on the device: collate, pack, and ids back in ------------------------------------------------------------- */
/* What a model beside this library in the same process wants of a batch: [rows, L] integer tensors in HBM instead of the ragged ids, and
 * the way back from a [rows, L] tensor of generated ids to text - without an id crossing the host link.  No counterpart in the reference
 * (its callers collate on the host).  Output pointers are device pointers (the storage of a torch tensor, a slice of one: any alignment
 * that is a multiple of the element size gets 16-byte stores between an unaligned head and tail) or page-locked host pointers from
 * tm_host_alloc.  EVERY element of every output row is written: the caller passes uninitialized memory.  The calls are asynchronous on
 * `stream` unless stated otherwise; tm_batch_collate and tm_batch_pack first wait for the batch's last run as tm_batch_decode does (the
 * ids are all there, the emit stage repeated if its buffer was too small) and fail with TM_E_INVALID on a batch that holds no ids (no
 * completed tm_batch_run or tm_batch_load_ids since its last upload).
 * tm_collate: the documents first_doc .. first_doc + ndocs - 1 of the last run (beyond the run: TM_E_INVALID), rows of row_len ids of
 * id_bytes 2, 4 or 8 bytes each, little-endian (8: int64 as torch wants it; 2 with a vocabulary of more than 65 536 ids or a special id
 * >= 65 536: TM_E_INVALID).  pad_id must be given; bos_id / eos_id: TM_NONE = no such special.  Every argument error is TM_E_INVALID. */
#define TM_COLLATE_PAD_LEFT 1u
#define TM_COLLATE_KEEP_TAIL 2u
typedef struct tm_collate {
  uint32_t first_doc, ndocs;   /* documents of the last run to lay out (ndocs == rows in row mode) */
  uint32_t row_len, id_bytes;  /* L; 2, 4 or 8 */
  uint32_t pad_id, bos_id, eos_id;   /* TM_NONE: no such special (pad_id must be given) */
  uint32_t flags;
} tm_collate;
/* One document per row: row r = [bos] content [eos], then pad_id up to row_len - on the left under TM_COLLATE_PAD_LEFT.  content: the
 * document's ids cut to row_len - (number of specials given): its head, under TM_COLLATE_KEEP_TAIL its tail; the specials are always
 * there (row_len smaller than their number: TM_E_INVALID).  ids_out[ndocs * row_len] elements of id_bytes; mask_out (may be NULL)
 * [ndocs * row_len] bytes, 1 on an entry and 0 on padding; lengths_out (may be NULL) [ndocs]: entries of a row, specials included. */
int tm_batch_collate(tm_batch* b, const tm_collate* how, void* stream,
                     void* ids_out, uint8_t* mask_out, uint32_t* lengths_out);
/* The pre-training form: the stream ids(first_doc) [eos] ids(first_doc + 1) [eos] ... (no separator with eos_id == TM_NONE: an empty
 * document then leaves no trace; bos_id and flags are not used) cut into rows of row_len, the last one filled up with pad_id.
 * tm_batch_pack_rows: the rows that takes, ceil(stream length / row_len) (synchronizes like tm_batch_totals).  tm_batch_pack writes them:
 * ids_out[rows * row_len]; doc_index_out (may be NULL) the document of every position, counted from first_doc, 0xFFFFFFFF on padding;
 * position_out (may be NULL) its index inside the document, the separator being the document's last position, 0 on padding.  rows_cap
 * smaller than the rows needed: TM_E_NOSPACE, nothing is written, tm_last_error names the number (tm_batch_pack_rows returns it). */
int tm_batch_pack_rows(tm_batch* b, const tm_collate* how, uint64_t* rows_needed);   /* synchronizes like tm_batch_totals */
int tm_batch_pack(tm_batch* b, const tm_collate* how, void* stream, uint64_t rows_cap,
                  void* ids_out, uint32_t* doc_index_out, uint32_t* position_out);
/* The reverse: rows[nrows * row_len] ids of id_bytes each (device or page-locked memory, as above) become the batch's ragged ids and
 * offsets, one document per row, and the batch is in the state a run leaves it in - ndocs = nrows, ids, offsets, totals, missing = 0 - so
 * that tm_batch_decode, tm_batch_decoded_download, tm_batch_download and tm_batch_totals (and the two calls above) work on it.  What of a
 * row counts, with pad_id / bos_id / eos_id TM_NONE = not given: a leading run of pad_id is skipped (left padding); from there the row
 * extends over lengths[r] entries (device or page-locked, as tm_batch_collate writes them; NULL: to the row's end); one leading bos_id
 * is skipped; the ids end in front of the first eos_id inside that extent.  Without lengths and eos_id a row's right padding counts as
 * ids.  Ids >= tm_vocab_n_ids pass through (the decoder skips them).  May grow the batch's id buffer (then it waits for the device);
 * nrows > max_docs of tm_batch_create: TM_E_LIMIT.  Lengths, a scan of them (the k_scan_* kernels of the run) and a gather, all on `stream`. */
int tm_batch_load_ids(tm_batch* b, const void* rows, uint32_t nrows, uint32_t row_len, uint32_t id_bytes,
                      const uint32_t* lengths, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id, void* stream);

/* ---- byte spans of the ids: where in the text each id came from (the offset_mapping of other tokenizers) ----------------------------------- */
/* The walk stands at byte i of a document when it emits an id and then moves on by that token's advance: the id's span is [i, i + advance),
 * counted in bytes from the document's start in the NORMALIZED text the walk runs on - after tm_batch_upload_raw + tm_batch_normalize the text
 * tm_batch_download_text returns (the raw text itself for a vocabulary with capcode 0 and no normalization flags); mapping a span back through
 * the normalizer to offsets of the raw text is what tm_batch_raw_spans below does.  The delete token a forward-delete branch emits behind a token
 * gets the empty span at that token's end; a character without a token gets [i, i + 1) when the vocabulary has an unk token and otherwise
 * leaves no id, hence a gap; a token may advance by 0 bytes (a one-byte alternative in a forward-delete state): its span is empty.  Begins
 * never decrease and the spans of a document never overlap.  Neither the ids nor a decode give the spans back (the "D " duplicates of a
 * capcode vocabulary, forward deletes and alternatives of another length stand in the way).  Not offered for tm_tokenize_pipeline,
 * tm_tokenize_document, the streaming encoder and tm_batch_pack.
 * tm_batch_spans: spans_out (device or page-locked memory, aligned to 8 bytes) receives uint32_t[total ids][2], the pairs (begin, end) in
 * exactly the slot order of tm_batch_device_tokens.  Waits for the batch's last run as tm_batch_collate does, is then asynchronous on `stream`.
 * spans_cap (in ids) smaller than the total: TM_E_NOSPACE, nothing is written.  A batch whose ids did not come from a walk (no completed
 * tm_batch_run since the last upload, or tm_batch_load_ids since): TM_E_INVALID.  A document of 2^32 normalized bytes or more: TM_E_LIMIT.
 * The pass reads what the run left (it walks the chains again, without fetching an id) and changes none of it: ids, totals, missing and
 * counts stay as they are. */
int tm_batch_spans(tm_batch* b, void* stream, uint32_t* spans_out, uint64_t spans_cap);
/* The companion of tm_batch_collate, with the same tm_collate: spans_out[ndocs * row_len * 2] elements of span_bytes 4 or 8 (8: int64 as
 * torch wants it), (begin, end) per column.  A column that holds an id of the document gets that id's pair - head, TM_COLLATE_KEEP_TAIL and
 * TM_COLLATE_PAD_LEFT exactly as for the ids -; BOS, EOS and padding get (0, 0).  Every element is written, with 16-byte stores between an
 * unaligned head and tail.  The ragged pairs are produced first, on `stream`, into a grow-only buffer of the batch: two calls on one batch
 * at the same time want the same stream.  Errors as tm_batch_collate and tm_batch_spans. */
int tm_batch_collate_spans(tm_batch* b, const tm_collate* how, void* stream, void* spans_out, uint32_t span_bytes);
/* tm_tokenize_batch with the spans: spans_out[tokens_cap][2] beside tokens_out[tokens_cap].  On a lane like the other host-buffer calls (no
 * allocation in steady state, nothing on the NULL stream, callable concurrently); if tokens_cap is too small tok_offsets IS filled, nothing is
 * written to tokens_out and spans_out, and TM_E_NOSPACE is returned. */
int tm_tokenize_batch_spans(const tm_vocab* v, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs,
                            uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* tok_offsets, uint32_t* spans_out, uint32_t* missing);

/* ---- raw-text spans: the same pairs as offsets into the bytes the caller uploaded ---------------------------------------------------------- */
/* After tm_batch_upload_raw + tm_batch_normalize + tm_batch_run, the span of every id counted in bytes from its document's start in the RAW
 * text.  Every normalized byte is owned by one unit of the raw document (tm_build.h, tm_normalize_origins: a character; the bytes it turns
 * into and the capcode markers in front of its letter are its own, a 'W' / 'C' over a raw space is the space's); own[n] is the raw offset
 * of the owner of normalized byte n.  An id with the normalized span [nb, ne), ne > nb, gets [own[nb], next(ne - 1)): next(n) is the first
 * own[n'] > own[n] with n' > n, or the raw length of the document - so what the normalizer drops (a collapsed space, a '\r', a removed mark)
 * falls into the span in front of it, and the spans of a document of a vocabulary with an unk token tile it.  An id without bytes (a delete
 * token, a step that consumes none) gets the empty span (x, x), x = next(nb - 1), or 0 at the document's start.
 *  - Begins and ends never decrease.
 *  - Two neighbouring ids may have the SAME or overlapping raw spans: a token boundary inside one character's output ("D" | " h" are both
 *    that 'H'), or inside a stretch whose combining marks NFD reordered (one unit on the host).
 *  - With capcode 0 and normalization flags 0 the raw spans ARE the normalized spans.
 * The documents the device normalized, of a vocabulary with capcode 0 or 2 and no flag but NFD and lowercase, are mapped on the device (the
 * normalizer's exact path again over the resident raw text, writing owners instead of text); every other document - those the normalizer left
 * to the host, and all of them under accents, quotemarks, collapse, trim, leadingspace or unixlines - is fetched back, mapped by
 * tm_normalize_origins on the host and its owners uploaded; *host_docs (may be NULL) receives their number.  The owners live in a grow-only
 * buffer of the batch (4 bytes per normalized byte, counted in tm_batch_device_bytes) made on request only: tm_batch_normalize and
 * tm_batch_run do nothing for it.  The call waits for the run like tm_batch_spans, and for its own host part where there is one; it changes
 * nothing a later call reads.
 * Slot order, alignment, TM_E_NOSPACE (nothing written) and the errors of tm_batch_spans / tm_batch_collate_spans / tm_tokenize_batch_spans
 * apply unchanged; besides: a batch whose text did not come from tm_batch_upload_raw + tm_batch_normalize: TM_E_INVALID; a raw document of
 * 2^32 bytes or more: TM_E_LIMIT.  Not offered for tm_tokenize_pipeline, tm_tokenize_document, the streaming encoder and tm_batch_pack. */
int tm_batch_raw_spans(tm_batch* b, void* stream, uint32_t* spans_out, uint64_t spans_cap, uint32_t* host_docs);
/* As tm_batch_raw_spans, with its three parts between HIP events on `stream`: ms[0] the normalized pairs (tm_batch_spans' pass), ms[1] the
 * origin pass (with the host's share where documents are mapped there), ms[2] the map.  Synchronizes.  ms NULL: tm_batch_raw_spans. */
int tm_batch_raw_spans_timed(tm_batch* b, void* stream, uint32_t* spans_out, uint64_t spans_cap, uint32_t* host_docs, float* ms);
int tm_batch_collate_raw_spans(tm_batch* b, const tm_collate* how, void* stream, void* spans_out, uint32_t span_bytes);
/* tm_tokenize_batch_spans for RAW documents: normalize, run and map on a lane, like tm_count_batch_raw. */
int tm_tokenize_batch_raw_spans(const tm_vocab* v, const uint8_t* raw, const uint64_t* offsets, uint32_t ndocs,
                                uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* tok_offsets, uint32_t* spans_out, uint32_t* missing);

/* ---- sliding windows: a long document as several rows that overlap (stride / return_overflowing_tokens / overflow_to_sample_mapping) ------- */
/* The third layout beside tm_batch_collate (which drops what does not fit a row) and tm_batch_pack (which cuts where the stream crosses a row
 * end): every id of every document is kept, a document longer than a row becomes several rows, and consecutive rows of a document share
 * `overlap` ids.  The same tm_collate; the overlap travels beside it.  With ns the number of specials given (bos_id, eos_id):
 * room = row_len - ns content ids per row, step = room - overlap.  room < 1 or overlap >= room: TM_E_INVALID.  A document of n ids yields
 * w(n) = 1 rows if n <= room (an empty document too: its specials and padding), else 1 + ceil((n - room) / step).  Row k of the document is
 * [bos] ids[k * step .. min(k * step + room, n)) [eos], then pad_id up to row_len - on the left under TM_COLLATE_PAD_LEFT: every row of a
 * document but its last is full, and the last holds at least one id the one before did not.  Rows stand in the order of the documents, then
 * of k.  TM_COLLATE_KEEP_TAIL has no meaning here: TM_E_INVALID.  The ids are those of the ONE walk over the whole document: tokenizing the
 * text of a window by itself gives other ids at the cuts.
 * tm_batch_window_rows: the rows that takes, sum of w(n) over the documents - counted on the device (a count per document, a scan of them
 * into a grow-only buffer of the batch, counted in tm_batch_device_bytes), one number read back; synchronizes like tm_batch_pack_rows.
 * tm_batch_windows does the same and then, on `stream`, finds the document of every row (4 bytes per row in a second such buffer) and writes
 * the rows: ids_out[rows * row_len] elements of id_bytes; mask_out (may be NULL)
 * [rows * row_len] bytes, 1 on an entry and 0 on padding; lengths_out (may be NULL) [rows]: entries of a row, specials included; row_doc_out
 * (may be NULL) [rows]: the row's document, counted from first_doc (overflow_to_sample_mapping); row_start_out (may be NULL) [rows]: k * step,
 * the index inside the document of the row's first content id.  rows_cap smaller than the rows needed: TM_E_NOSPACE, nothing is written,
 * tm_last_error names the number (tm_batch_window_rows returns it); more than 2^36 elements in one output: TM_E_LIMIT.  Otherwise outputs,
 * alignment, stores and errors are those of tm_batch_collate (not its freedom of streams: below).
 * tm_batch_windows_spans / tm_batch_windows_raw_spans: spans_out[rows * row_len * 2] elements of span_bytes 4 or 8, (begin, end) per column
 * - a content column gets exactly the pair tm_batch_spans / tm_batch_raw_spans give for its id, so a document's offsets keep counting from
 * the DOCUMENT's start in every one of its rows; BOS, EOS and padding get (0, 0).  The ragged pairs are produced first, on `stream`, into the
 * batch's own buffer as for tm_batch_collate_spans / tm_batch_collate_raw_spans, whose errors apply: ids from tm_batch_load_ids, or for the
 * raw form a text that did not come from tm_batch_upload_raw + tm_batch_normalize, are TM_E_INVALID.
 * The calls change nothing a later call reads - ids, offsets, totals, missing stay as they are.
 * Streams - stricter than for tm_batch_collate: EVERY one of the four calls, tm_batch_window_rows included, rewrites the rows per document
 * and their offsets in the batch's buffer on the stream of the batch's last run, and the fill calls rewrite the document of every row (and
 * the span forms the ragged pairs) on `stream`, while a fill reads all of them on `stream`.  So before the next window call of any kind on
 * the batch, the last fill must have completed or have run on the stream of the batch's last run - passing that stream to every call is
 * the simple way. */
int tm_batch_window_rows(tm_batch* b, const tm_collate* how, uint32_t overlap, uint64_t* rows_needed);   /* synchronizes like tm_batch_pack_rows */
int tm_batch_windows(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap,
                     void* ids_out, uint8_t* mask_out, uint32_t* lengths_out, uint32_t* row_doc_out, uint32_t* row_start_out);
int tm_batch_windows_spans(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap,
                           void* spans_out, uint32_t span_bytes);
int tm_batch_windows_raw_spans(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap,
                               void* spans_out, uint32_t span_bytes);

/* ---- character offsets: the same pairs counted in code points or UTF-16 units ----------------------------------------------------------- */
/* Two units are added beside bytes: */
#define TM_UNIT_BYTES 0u
#define TM_UNIT_CODEPOINTS 1u
#define TM_UNIT_UTF16 2u
/* A byte is a *continuation byte* if (b & 0xC0) == 0x80.
 * For a document of `len` bytes and a byte offset x in 0..len:
 *  - U(x) under TM_UNIT_CODEPOINTS is the number of non-continuation bytes in [0, x).
 *  - U(x) under TM_UNIT_UTF16 is that number plus the number of bytes >= 0xF0 in [0, x).
 *  - char_start(x) is x if x == len or byte x is not a continuation byte.
 *  - Otherwise char_start(x) is the nearest of x-1, x-2, x-3 that lies inside the document and holds a non-continuation byte.
 *  - If there is no such byte, char_start(x) is x.
 *  - D(x) = U(char_start(x)).
 * A byte pair (b, e) becomes:
 *  - (D(b), U(e)) if e > b;
 *  - (D(b), D(b)) if the span is empty.
 * Consequences:
 *  - On well-formed UTF-8 with both ends on character boundaries, this is the index into the decoded string: Python str for code points, a
 *    UTF-16 string for TM_UNIT_UTF16.
 *  - An end inside a character rounds outward.
 *  - Malformed text follows the rule literally.  Every non-continuation byte is one unit.  This header makes no claim about any decoder.
 *  - Pairs can end inside a character: TokenMonster tokens are byte strings, so normalized spans can; so can raw spans of a vocabulary with
 *    capcode 0 and no normalization flags (the identity map of tm_batch_raw_spans, which does not round to characters).
 *  - Begins never decrease.
 *  - The end of an empty span inside a character may lie one unit before the end in front of it (the empty span rounds down, the end in
 *    front of it rounded outward).
 *  - Units never exceed bytes, so 32-bit offsets still hold.
 *  - With TM_UNIT_BYTES every call below returns exactly what its existing counterpart returns.
 * `text` says which text the offsets point into: */
#define TM_TEXT_NORMALIZED 0u   /* offsets into the text the walk runs on (tm_batch_download_text) */
#define TM_TEXT_RAW        1u   /* offsets into the documents as uploaded (tm_batch_upload_raw) */
/* tm_batch_spans_in is tm_batch_spans (TM_TEXT_NORMALIZED) / tm_batch_raw_spans (TM_TEXT_RAW) in `unit`; tm_batch_collate_spans_in and
 * tm_batch_windows_spans_in are tm_batch_collate_spans / tm_batch_collate_raw_spans and tm_batch_windows_spans / tm_batch_windows_raw_spans;
 * tm_tokenize_batch_spans_in takes normalized input like tm_tokenize_batch_spans under TM_TEXT_NORMALIZED and raw input like
 * tm_tokenize_batch_raw_spans under TM_TEXT_RAW.  Slot order, alignment, TM_E_NOSPACE (nothing written), host_docs, the stream rules (the
 * stricter ones of the window calls included) and every error are those of the byte-span calls; BOS, EOS and padding columns stay (0, 0).
 * An unknown `text` or `unit`, and TM_TEXT_RAW on a batch whose text did not come from tm_batch_upload_raw + tm_batch_normalize, are
 * TM_E_INVALID before any device work.
 * The units come from an index of the text, made on request only and kept until the batch's next upload, one per `text` kind: per 256 bytes
 * of the text the number of non-continuation bytes (and, for TM_UNIT_UTF16 only, of bytes >= 0xF0) in front of them, counted in one streaming
 * pass over the resident text - the raw text as uploaded, or the normalized text (packed first, on `stream`, where it still lies in the normalizer's
 * buffers: a second tm_batch_run of the same upload wants that stream, or the pack completed) - and scanned.  It lives in a grow-only buffer of the batch of at most 1/8 of the text's bytes, counted in
 * tm_batch_device_bytes; tm_batch_normalize and tm_batch_run do nothing for it.  The ragged byte pairs are then converted in place (a work-item
 * per pair: the index entry plus a count over the part of a 256-byte block in front of the offset) and the collate and window fills run on
 * the converted pairs.  With TM_UNIT_BYTES no index is made and nothing is converted.
 * ms (may be NULL), when given, receives four parts and the call synchronizes as tm_batch_raw_spans_timed does: ms[0..2] are its parts
 * (ms[1..2] are 0 for TM_TEXT_NORMALIZED), ms[3] is the unit work, index plus conversion. */
int tm_batch_spans_in(tm_batch* b, void* stream, uint32_t text, uint32_t unit,
                      uint32_t* spans_out, uint64_t spans_cap, uint32_t* host_docs, float* ms /* may be NULL */);
int tm_batch_collate_spans_in(tm_batch* b, const tm_collate* how, void* stream, uint32_t text, uint32_t unit,
                              void* spans_out, uint32_t span_bytes);
int tm_batch_windows_spans_in(tm_batch* b, const tm_collate* how, uint32_t overlap, void* stream, uint64_t rows_cap,
                              uint32_t text, uint32_t unit, void* spans_out, uint32_t span_bytes);
int tm_tokenize_batch_spans_in(const tm_vocab* v, const uint8_t* docs, const uint64_t* offsets, uint32_t ndocs,
                               uint32_t text, uint32_t unit, uint32_t* tokens_out, uint64_t tokens_cap,
                               uint64_t* tok_offsets, uint32_t* spans_out, uint32_t* missing);

/* ---- text pairs: two documents in one row, [bos] A [sep] B [eos] with token types (text_pair / truncation / stride of other tokenizers) ----- */
/* The fourth layout: what rerankers, cross-encoders, NLI models and extractive QA read.  No counterpart in the reference.
 * Sides:
 *  - Both sides are documents of the same run: pair p is (document first_a + p, document first_b + p), p in 0..npairs.  The two ranges may
 *    overlap or coincide.  A range that reaches beyond the run is TM_E_INVALID.
 *  - A and B are tokenized as separate documents: no token spans the join.
 * Row of pair p, with a and b the id counts of the two documents:
 *  - ns is the number of specials: bos if given, plus sep_count, plus eos if given.  R = row_len - ns; row_len < ns is TM_E_INVALID.
 *  - sep_count is 1 or 2 copies of sep_id between the sides, and 0 if and only if sep_id == TM_NONE; anything else is TM_E_INVALID.
 *  - The row is [bos] A[0..a') [sep]*sep_count B[0..b') [eos], then pad_id up to row_len - on the left under TM_COLLATE_PAD_LEFT.
 *  - Both sides keep their heads.  TM_COLLATE_KEEP_TAIL, or any other flag, is TM_E_INVALID.
 * Kept counts (a', b').  If a + b <= R nothing is cut.  Otherwise:
 *  - TM_PAIR_LONGEST_FIRST: remove one id at a time from the end of the side that is currently longer, from A on a tie, until
 *    a' + b' == R.  (In closed form, with h = R / 2 rounded down, the first that applies: a <= h gives (a, R - a); b <= R - h gives
 *    (R - b, b); otherwise (h, R - h).)
 *  - TM_PAIR_ONLY_SECOND: a' = min(a, R) and b' = min(b, R - a').
 *  - TM_PAIR_ONLY_FIRST: b' = min(b, R) and a' = min(a, R - b').
 *  - Neither ONLY_* form ever fails per row (the device has nowhere to report a per-row error): the side that is not to be cut is cut when
 *    it alone overflows the row.
 *  - An unknown `truncation` is TM_E_INVALID. */
#define TM_PAIR_LONGEST_FIRST 0u
#define TM_PAIR_ONLY_FIRST    1u
#define TM_PAIR_ONLY_SECOND   2u
typedef struct tm_pair {
  uint32_t first_a, first_b, npairs;   /* pair p = (document first_a + p, document first_b + p) of the last run */
  uint32_t row_len, id_bytes;          /* L; 2, 4 or 8 */
  uint32_t pad_id, bos_id, sep_id, eos_id;   /* TM_NONE: no such special (pad_id must be given) */
  uint32_t sep_count;                  /* copies of sep_id between the sides: 1 or 2 (0 iff sep_id == TM_NONE) */
  uint32_t truncation;                 /* TM_PAIR_* */
  uint32_t flags;                      /* TM_COLLATE_PAD_LEFT only */
} tm_pair;
/* Outputs of tm_batch_pair.  EVERY element of every output is written: the caller passes uninitialized memory.  Pointers are device or
 * page-locked, as for tm_batch_collate, with 16-byte stores between an unaligned head and tail; the call waits for the batch's last run
 * and is then asynchronous on `stream` in the same way, and every argument error is TM_E_INVALID.
 *  - ids_out[npairs * row_len] elements of id_bytes.
 *  - mask_out (may be NULL) [npairs * row_len] bytes: 1 on an entry and 0 on padding.
 *  - type_out (may be NULL) [npairs * row_len] bytes, the token_type_ids: 0 on bos, on A's ids and on the separators; 1 on B's ids and on
 *    eos; 0 on padding.
 *  - kept_out (may be NULL) uint32_t[npairs][2]: (a', b').  The row's entry count is ns + a' + b', and every column's role follows from
 *    (a', b') and the specials given - hence there is no separate special-tokens mask.
 *  - Two-byte ids follow the rule of tm_collate, with sep_id counted among the specials.
 *  - More than 2^36 elements in one output is TM_E_LIMIT.  npairs == 0 is TM_OK and touches nothing. */
int tm_batch_pair(tm_batch* b, const tm_pair* how, void* stream,
                  void* ids_out, uint8_t* mask_out, uint8_t* type_out, uint32_t* kept_out);
/* The spans of the ids laid out like the rows: spans_out[npairs * row_len * 2] elements of span_bytes 4 or 8, (begin, end) per column.  A
 * content column gets exactly the pair tm_batch_spans_in(text, unit) gives for its id, so each side's offsets count from its OWN
 * document's start; specials and padding get (0, 0).  The ragged pairs are produced first, on `stream`, into the batch's own buffer as for
 * tm_batch_collate_spans_in, whose errors and stream remark apply unchanged: TM_TEXT_RAW on a batch without raw text, ids that came from
 * tm_batch_load_ids and an unknown `text` or `unit` are TM_E_INVALID.  This is the one entry point: TM_TEXT_NORMALIZED with TM_UNIT_BYTES
 * is the plain case. */
int tm_batch_pair_spans_in(tm_batch* b, const tm_pair* how, void* stream, uint32_t text, uint32_t unit,
                           void* spans_out, uint32_t span_bytes);
/* Pair windows, the QA form: the question (A) stands in every row and the context (B) slides, every id of B kept.
 *  - `truncation` must be TM_PAIR_ONLY_SECOND, else TM_E_INVALID.
 *  - a' = min(a, max_first).  Per pair, room_p = R - a' ids of B per row and step_p = room_p - overlap.
 *  - max_first > R, or R - max_first <= overlap, is TM_E_INVALID (checked on the host): every pair has step_p >= 1.
 *  - Pair p yields w(b) rows with room_p and step_p, w as for tm_batch_windows: 1 if b <= room_p (an empty B too), else
 *    1 + ceil((b - room_p) / step_p).
 *  - Row k of pair p is [bos] A[0..a') [sep]*sep_count B[k * step_p .. min(k * step_p + room_p, b)) [eos] plus padding.
 *  - Rows stand in pair order, then k.
 * tm_batch_pair_window_rows: the rows that takes, counted on the device; synchronizes like tm_batch_window_rows.  tm_batch_pair_windows
 * writes them: ids_out, mask_out and type_out as above with rows in place of npairs; kept_out (may be NULL) [rows][2]: (a', ids of B in
 * this row); row_pair_out (may be NULL) [rows]: the pair of a row, counted from 0 (overflow_to_sample_mapping); row_start_out (may be
 * NULL) [rows]: k * step_p, the index inside B of the row's first id of B.  rows_cap smaller than the rows needed: TM_E_NOSPACE, nothing is
 * written, tm_last_error names the number (tm_batch_pair_window_rows returns it); more than 2^36 elements in one output: TM_E_LIMIT.
 * tm_batch_pair_windows_spans_in: spans_out[rows * row_len * 2] as for tm_batch_pair_spans_in; B's offsets count from B's document start
 * in every row.
 * Streams: the counts per pair, their scan and the pair of every row live in the SAME buffers of the batch as those of tm_batch_windows.
 * So the stricter stream rule of tm_batch_windows applies word for word, over the window calls of both kinds: every one of these three
 * calls, tm_batch_pair_window_rows included, rewrites the rows per pair and their offsets on the stream of the batch's last run, and the
 * fill calls rewrite the pair of every row (and the span form the ragged pairs) on `stream`, while a fill reads all of them on `stream`.
 * Before the next window call of any kind on the batch, the last fill must have completed or have run on the stream of the batch's last
 * run - passing that stream to every call is the simple way. */
int tm_batch_pair_window_rows(tm_batch* b, const tm_pair* how, uint32_t overlap, uint32_t max_first, uint64_t* rows_needed);
int tm_batch_pair_windows(tm_batch* b, const tm_pair* how, uint32_t overlap, uint32_t max_first, void* stream, uint64_t rows_cap,
                          void* ids_out, uint8_t* mask_out, uint8_t* type_out, uint32_t* kept_out,
                          uint32_t* row_pair_out, uint32_t* row_start_out);
int tm_batch_pair_windows_spans_in(tm_batch* b, const tm_pair* how, uint32_t overlap, uint32_t max_first, void* stream,
                                   uint64_t rows_cap, uint32_t text, uint32_t unit, void* spans_out, uint32_t span_bytes);

/* Streaming Decoder (go/tokenmonster.go:552-700 NewDecoder / Decode / DecodeSerialized / Flush; server jobs 5-9): ids arrive a few
 * at a time, a call returns the text that is COMPLETE so far; the bytes of a character that is not (a token may end in the middle of a
 * UTF-8 sequence) and the state of the capcode decoder are carried to the next call.  Per-connection host state: the gather of a
 * handful of ids runs on the host copy of the reverse table.  out_len receives the number of bytes decoded; on TM_E_NOSPACE
 * (out_cap too small) the ids HAVE been consumed and the text is kept: call again with n = 0 and a buffer of *out_len bytes.
 * tm_decoder_flush returns (and forgets) the held-back bytes.
 * Quirk kept from the reference: the number of bytes held back is incompleteUTF8Bytes' return value, which for a character that
 * is cut is the number of bytes still MISSING (go/tokenmonster.go:183-185), not the number present; where that exceeds the
 * buffer (Go panics there) the whole buffer is held back. */
int tm_decoder_new(const tm_vocab* v, tm_decoder** out);
void tm_decoder_free(tm_decoder* d);
int tm_decoder_decode(tm_decoder* d, const uint32_t* tokens, uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t* out_len);
int tm_decoder_decode_serialized(tm_decoder* d, const uint8_t* data, uint64_t nbytes, uint32_t encoding_length, uint8_t* out,
                                 uint64_t out_cap, uint64_t* out_len);
int tm_decoder_flush(tm_decoder* d, uint8_t* out, uint64_t out_cap, uint64_t* out_len);

/* Streaming ENCODER: one document that arrives in pieces (a file read in blocks, a socket, a decompressor) or that is larger than a device
 * workspace should be.  The ids returned by the tm_encoder_feed calls and by tm_encoder_finish, one after the other, are tm_tokenize_batch
 * of the concatenated text as ONE document - Vocab.tokenize (go/tokenmonster.go:1017), bit for bit - however the text was cut; so is `missing`.
 * tm_encoder_feed takes ALREADY NORMALIZED bytes, tm_encoder_feed_raw (below) raw UTF-8; one document is fed through one of the two.  Ids come
 * as uint32; no serialized form.
 * How: the walk's state at a token boundary is one of 80 entry states (tm_score_begin above); a pass over the text held so far owns all but
 * its last 128 bytes, which it may look at, emits every token that BEGINS in what it owns, and leaves the state it ended in on the device
 * for the next pass.  A feed therefore returns the ids that are FINAL so far: those of the last 128 bytes (and of a text shorter than 192
 * bytes altogether) come with a later call.  tm_encoder_finish says that the text ends here, returns the remaining ids and *missing (may be
 * NULL) for the whole document; the encoder is then ready for the next document.
 * max_piece_bytes: the most text one device pass takes (0 = 32 MiB; at least 64); a longer feed is split inside.  The device memory held
 * (tm_encoder_device_bytes) depends on this only, never on the length of the document.
 * On TM_E_NOSPACE (tokens_cap too small; *n_tokens = the capacity needed) the text HAS been consumed and the ids are kept: call
 * tm_encoder_feed with n = 0 and a larger buffer.  A text the walk cannot advance on (TM_E_INPUT above) is reported by the call whose pass
 * meets it; after any failed pass the encoder refuses work until tm_encoder_reset, which forgets the current document.
 * tm_encoder_state: the entry state (0..79: 2 * offset of the next token start + pending forward delete) the next pass will start in.
 * One encoder belongs to one caller at a time; different encoders of one vocabulary run concurrently: each owns a stream and a device
 * workspace (nothing on the NULL stream, no allocation in steady state).  Free the encoders of a vocabulary before the vocabulary. */
int tm_encoder_new(const tm_vocab* v, uint64_t max_piece_bytes, tm_encoder** out);
void tm_encoder_free(tm_encoder* e);
int tm_encoder_feed(tm_encoder* e, const uint8_t* text, uint64_t n, uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* n_tokens);
int tm_encoder_finish(tm_encoder* e, uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* n_tokens, uint32_t* missing);
int tm_encoder_reset(tm_encoder* e);
uint32_t tm_encoder_state(const tm_encoder* e);
uint64_t tm_encoder_device_bytes(const tm_encoder* e);
/* RAW text through the streaming encoder.  The normalizer carries state of its own across a cut (capcode's word look-ahead and rewrite
 * window, the order of marks under NFD, the neighbours `collapse` and `unixlines` look at), but right behind a line feed that state is the
 * state at the start of a text: normalize(a + b) == normalize(a) + normalize(b) when a ends in '\n'.  So the library cuts the raw text
 * itself: tm_encoder_feed_raw normalizes and tokenizes everything up to the last '\n' it has been given - on the device, as pieces of at most
 * max_piece_bytes; a piece with characters the device normalizer leaves to the host normalizer takes that path inside the call
 * (tm_encoder_host_pieces counts them per document) - and keeps the raw bytes behind it on the host (tm_encoder_raw_held of them) until more
 * text or tm_encoder_finish arrives; tm_encoder_finish normalizes them as the last piece.  The ids of the calls and of tm_encoder_finish, one
 * after the other, and `missing` are those of tm_normalize + tm_tokenize_batch of the whole text as one document, wherever the caller cut it:
 * inside a UTF-8 character, inside a run of capitals, between '\r' and '\n'.
 * Once max_piece_bytes are held without a '\n' the cut goes behind the last byte of  \t . , ; : ! ? ( ) [ ] { } < > = / - "  (the same holds
 * there); without one of those either the call returns TM_E_LIMIT - normalize such a text as a whole - and the encoder wants tm_encoder_reset.
 * Vocabularies: capcode 0 or 2 and none of the normalization flags quotemarks 8, trim 32, leadingspace 64 - those need the whole document -
 * (tm_encoder_raw_supported: 1 or 0).  With another vocabulary tm_encoder_feed_raw returns TM_E_INVALID, consumes nothing and leaves the
 * encoder to tm_encoder_feed.  Within one document tm_encoder_feed and tm_encoder_feed_raw do not mix (TM_E_INVALID, nothing consumed;
 * tm_encoder_finish and tm_encoder_reset end the document; calls with n = 0, which only fetch ids, are free).  TM_E_NOSPACE, tm_encoder_state
 * and the threading rule are those of tm_encoder_feed.  The normalizer's device workspace is made by the first raw feed - its size depends on
 * max_piece_bytes only - and counts in tm_encoder_device_bytes from then on; an encoder that is only fed normalized text never holds it. */
int tm_encoder_raw_supported(const tm_vocab* v);
int tm_encoder_feed_raw(tm_encoder* e, const uint8_t* raw, uint64_t n, uint32_t* tokens_out, uint64_t tokens_cap, uint64_t* n_tokens);
uint64_t tm_encoder_raw_held(const tm_encoder* e);
uint32_t tm_encoder_host_pieces(const tm_encoder* e);

/* ---- one large document, host to host ------------------------------------------------------------------------------ */
/* tm_tokenize_document: ONE document that is in hand as a whole (a file of hundreds of megabytes: the shape of the reference's own benchmark,
 * one Vocab.tokenize of the whole content), tokenized in pieces of piece_bytes (0 = 32 MiB; 64 .. 2^36) that run through `slots` device
 * workspaces (0 = 3; 2 .. 8) at once: while piece k resolves its entry state, emits, packs and downloads its ids, the match kernel of piece
 * k + 1 runs and piece k + 2 uploads.  The walk's state and - for raw text - the 128 bytes of look-ahead go from slot to slot on the device.
 * Output: what tm_tokenize_batch_serialized gives for this text as one document (after tm_normalize when raw != 0) - the ids of Vocab.tokenize
 * (go/tokenmonster.go:1017), bit for bit, encoding_length bytes each, little-endian (2, 3 or 4; 0 = automatic, go :990-996; 4 = plain uint32)
 * - and its *missing (may be NULL).  *bytes_needed is always set; on TM_E_NOSPACE nothing in bytes_out is promised and *bytes_needed is the
 * capacity required.  n == 0 is an empty document.
 * raw != 0: the text is cut behind line feeds (as tm_encoder_feed_raw cuts it) and each piece is normalized on the device, beside the walk of
 * the piece before; a piece the device normalizer leaves to the host normalizer takes that path inside the call (stats->host_pieces).  Raw
 * text of a vocabulary whose normalizer needs the whole document (quotemarks 8, trim 32, leadingspace 64), and a text with piece_bytes bytes
 * without a byte to cut behind, is normalized once by the host normalizer first (stats->host_normalized = 1).  Capcode 1 with raw != 0:
 * TM_E_INVALID.  Pageable buffers go through pinned staging; buffers from tm_host_alloc / tm_host_register are DMA'd directly.
 * The slots come from a grow-only pool of the vocabulary shaped by (piece_bytes, raw): a second call of the same shape allocates nothing, and
 * the device memory held (stats->device_bytes) depends on piece_bytes and slots only.  Concurrent calls take different slots (at most four
 * calls at once, further callers wait).  Nothing runs on the NULL stream; the call uses the calling thread only. */
typedef struct tm_document_stats {
  uint32_t pieces, slots;
  int input_pinned, output_pinned;
  uint64_t normalized_bytes;
  uint32_t host_pieces;        /* raw pieces the host normalizer took inside the call */
  uint32_t host_normalized;    /* 1: the whole document was normalized on the host first */
  uint64_t device_bytes;       /* device memory the call held: a function of piece_bytes and slots only */
} tm_document_stats;
int tm_tokenize_document(const tm_vocab* v, const uint8_t* text, uint64_t n, int raw, uint32_t encoding_length, uint64_t piece_bytes,
                         uint32_t slots, uint8_t* bytes_out, uint64_t bytes_cap, uint64_t* bytes_needed, uint32_t* missing,
                         uint32_t* encoding_length_used, tm_document_stats* stats);

/* ---- trainvocab scoring pass: replaces training/trainvocab.go:925-1176 ------------------------ */
/* Upload the normalized dataset once (trainvocab.go:1660-1665 keeps it for the whole run). */
int tm_dataset_upload(const uint8_t* normalized, uint64_t n, tm_dataset** out);
int tm_dataset_upload_on(const uint8_t* normalized, uint64_t n, int device, tm_dataset** out);   /* on a named device */
int tm_dataset_device(const tm_dataset* d);                                                       /* the device it lives on */
void tm_dataset_free(tm_dataset* d);
/* Walks each strip [strip_off[k], strip_off[k]+strip_len[k]) of the dataset exactly as the worker
 * does and accumulates scores[id] += bytes covered, scores[deleteToken] += 1 per forward-delete,
 * *tokens_in_text, and the 256-bit set of bytes that had no token.  scores has tm_vocab_n_ids()
 * entries and is OVERWRITTEN.  n_strips == 0 means one strip = the whole dataset. */
int tm_score(const tm_vocab* v, tm_dataset* d, const uint64_t* strip_off, const uint64_t* strip_len,
             uint32_t n_strips, uint32_t* scores, uint64_t* tokens_in_text, uint8_t missing_set[32]);
/* Device-resident variant for multi-GPU reduction: leaves the histogram in HBM and returns its
 * device pointer, *n_words = n_ids + 4 + 256 uint32: scores[n_ids] | tokens_in_text as four 16-bit limbs |
 * missing[256] per-byte counters - every word is a plain sum over ranks, so ONE RCCL all-reduce(sum, uint32)
 * merges the partial results of data-parallel ranks. */
int tm_score_device(const tm_vocab* v, tm_dataset* d, const uint64_t* strip_off, const uint64_t* strip_len,
                    uint32_t n_strips, void* stream, uint32_t** dev_hist, uint64_t* n_words);

/* As tm_score_device, but also copies the histogram (device to device, on `stream`) into a caller-owned device
 * buffer of dst_words >= n_ids + 4 + 256 uint32 — e.g. the storage of a torch tensor that is then all-reduced. */
int tm_score_device_into(const tm_vocab* v, tm_dataset* d, const uint64_t* strip_off, const uint64_t* strip_len,
                         uint32_t n_strips, void* stream, uint32_t* dst_device, uint64_t dst_words);

/* ---- one whole-buffer walk over several GPUs (training/trainvocab.go:909-922: after "midway" the worker walks the dataset as ONE
 * strip) --------------------------------------------------------------------------------------------------------------------
 * Rank r owns the bytes [off, off+len) of the dataset and has uploaded them followed by a halo of >= 128 bytes of the text that
 * comes next (continues != 0; the last rank has none).  The walk's state at a byte is (offset of the next token start, pending
 * forward-delete flag) = one of 80 ENTRY STATES (2 * offset + flag, offset < 40), and what a range does to it is a map of 80 entries:
 *   tm_score_begin   runs the match kernel over the range and returns exits[80]: exits[e] = the entry state of the NEXT range if this
 *                    one is entered in state e (0xFF: e cannot occur).  Ranks all-gather their 80 bytes; rank r's true entry state is
 *                    exits[r-1][ exits[r-2][ ... exits[0][0] ] ].
 *   tm_score_finish  completes the pass from that entry state: histogram exactly as tm_score_device[_into] leaves it (dst_device may be
 *                    NULL).  A token that begins inside the range is counted by this rank even if it ends in the halo.
 * Summed over the ranks (one all-reduce) the histograms equal tm_score of the whole dataset as one strip, bit for bit.
 * tm_score_read copies the histogram of the last pass to the host in tm_score's form.
 * continues: 0 = the text ends with the range; 1 = more text follows and the dataset holds >= 128 bytes of it behind the range (fewer:
 * TM_E_INVALID - the exit states would silently differ from the whole-buffer walk's); 2 = text follows and ALL of it is in the dataset
 * (it ends inside the halo).  One caller per dataset between the two halves of a pass. */
int tm_score_begin(const tm_vocab* v, tm_dataset* d, uint64_t off, uint64_t len, int continues, void* stream, uint8_t* exits);
int tm_score_finish(const tm_vocab* v, tm_dataset* d, uint32_t entry_state, void* stream, uint32_t* dst_device, uint64_t dst_words);
int tm_score_read(const tm_vocab* v, tm_dataset* d, uint32_t* scores, uint64_t* tokens_in_text, uint8_t missing_set[32]);

/* ---- several devices of one node behind one handle: the multi-GPU half of the path for a host that stays ONE process ------------------------
 * The reference's parallelism is in-process: trainvocab starts `workers` goroutines over one dataset (training/trainvocab.go:1827-1829; after
 * "midway" each walks it as ONE strip, :909-922), the server fans a job's documents out over goroutines (training/tokenmonsterserver.go:363-378,
 * :773-787).  tm_devices names the GPUs; every call below drives all of them from inside the library, one host thread per device, and the ONE
 * collective of the path - the sum of the scoring pass's histograms - is an ncclAllReduce(sum, uint32) over xGMI inside tm_score_multi.
 * RCCL is loaded at the first collective (librccl.so.1 is 570 MB: the single-GPU entry points never map it).
 *
 * tm_devices_open: the first max_devices visible devices (<= 0: all).  In a test process (TM_TEST_HOOKS set, like tm_debug_flags) TM_VIRTUAL_DEVICES=N
 * gives the handle N members that all sit on device 0 instead - the multi-device code paths on a one-GPU box; tm_devices_open_list names the devices itself (a device may appear
 * more than once).  Members that share a device cannot form an RCCL communicator (RCCL refuses two ranks on one device): there, with TM_RCCL=0, and
 * where librccl cannot be loaded, member 0 sums the histograms by peer copies and an add kernel - same result.  tm_devices_rccl_ranks: the
 * number of ranks of the communicator the handle uses (it is made on the first call of this or of tm_score_multi), 0 and *why_not = the
 * reason if there is none.  One-member handles skip the collective unless TM_RCCL=1.  Every call of this section leaves the calling thread's
 * current device as it found it. */
typedef struct tm_devices tm_devices;
typedef struct tm_vocab_set tm_vocab_set;       /* one replica of a vocabulary per member */
typedef struct tm_dataset_set tm_dataset_set;   /* one byte range of a normalized dataset per member */
int tm_devices_open(int max_devices, tm_devices** out);
int tm_devices_open_list(const int* devices, int n, tm_devices** out);
int tm_devices_count(const tm_devices* g);
int tm_devices_device(const tm_devices* g, int member);
int tm_devices_rccl_ranks(tm_devices* g, const char** why_not);
void tm_devices_close(tm_devices* g);            /* after every vocabulary set and dataset set made from it has been freed */
/* Load for all members: the tables are built once (tm_vocab_load on member 0) and the finished device block is copied device to device into
 * every other member (tm_vocab_block_export / _import).  tm_vocab_set_member(s, 0) is a full vocabulary (decoder, image); the other members
 * have device tables only.  The handles stay owned by the set. */
int tm_vocab_load_all(tm_devices* g, const uint8_t* vocab_file, size_t n, tm_vocab_set** out);
int tm_vocab_set_count(const tm_vocab_set* s);
const tm_vocab* tm_vocab_set_member(const tm_vocab_set* s, int member);
void tm_vocab_set_free(tm_vocab_set* s);
/* tm_vocab_tune for every member: the tables are laid out again once (member 0) and the block goes to the others as at tm_vocab_load_all. */
int tm_vocab_set_tune(tm_vocab_set* s, const uint8_t* normalized_sample, uint64_t n);
/* tm_tokenize_pipeline over every device (the server's fan-out, tokenmonsterserver.go:363-378): the chunks of whole documents are handed to
 * lanes_per_device lanes (0 = 4) of EVERY member from one queue, so a faster or less loaded device takes more of them; ids land in document
 * order whichever device computed them.  No collective.  Arguments and results exactly as tm_tokenize_pipeline. */
int tm_tokenize_pipeline_multi(const tm_vocab_set* s, const uint8_t* text, const uint64_t* offsets, uint32_t ndocs, int raw,
                               uint32_t encoding_length, uint64_t chunk_bytes, uint32_t lanes_per_device, uint8_t* bytes_out, uint64_t bytes_cap,
                               uint64_t* byte_offsets, uint32_t* missing, uint32_t* encoding_length_used, tm_pipeline_stats* stats);
/* The dataset of a training run cut into one contiguous byte range per member (multiples of 4 bytes, trainvocab.go:1674), each uploaded with
 * the 128 bytes that follow it (tokens straddle the cuts); a dataset of less than 4 KiB per member uses fewer members.
 * tm_dataset_set_range: bytes of a member's range, *halo_bytes (may be NULL) the bytes of following text it holds as well. */
int tm_dataset_upload_sharded(tm_devices* g, const uint8_t* normalized, uint64_t n, tm_dataset_set** out);
uint64_t tm_dataset_set_range(const tm_dataset_set* s, int member, uint64_t* halo_bytes);
void tm_dataset_set_free(tm_dataset_set* s);
/* One scoring pass over the WHOLE dataset as one strip (trainvocab.go:909-922), bit-identical to tm_score(v, whole dataset, n_strips = 0) on one
 * device: every member runs the match kernel on its range, the 80-entry exit maps of all ranges are gathered on every device (ncclAllGather
 * of 80 bytes per member; peer copies where there is no communicator) and chained there into the member's entry state, the histogram walk
 * follows on the same stream, and one all-reduce(sum) of the n_ids + 4 + 256 uint32 histogram words merges them: a member's host thread
 * enqueues its whole half of the pass and waits once.  Results as tm_score. */
int tm_score_multi(const tm_vocab_set* vs, tm_dataset_set* ds, uint32_t* scores, uint64_t* tokens_in_text, uint8_t missing_set[32]);

#ifdef __cplusplus
}
#endif
#endif

/* tokenize_stream.c — the streaming encoder of libtokenmonster_hip.so (tm_encoder_*) from plain C.
 *
 *   tokenize_stream [--raw] <file.vocab> <text file> [block MiB = 32] [ids file]
 *
 * Tokenizes the file (already normalized bytes, go/tokenmonster.go:963; with --raw: raw UTF-8, which the library normalizes piece by piece,
 * cutting behind line feeds) as ONE document without ever holding it whole: it is read in blocks of N MiB, every block is fed to the
 * encoder, and the ids that are final so far are written as they come — four bytes each, little-endian, to the ids file, or as decimal
 * numbers on one line to stdout, as tokenize_file prints them.  The ids are those tokenize_file gives for the normalized file - with --raw,
 * for the raw file normalized as a whole -; host and device memory depend on the block size only.  Needs an MI355X: there is no CPU path. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tokenmonster_hip.h"

static FILE* out_file = NULL;
static uint64_t total = 0;

static void put(const uint32_t* ids, uint64_t n) {
  if (out_file) {
    if (n && fwrite(ids, 4, (size_t)n, out_file) != (size_t)n) { perror("ids file"); exit(2); }
  } else {
    for (uint64_t i = 0; i < n; i++) printf(total + i ? " %u" : "%u", ids[i]);
  }
  total += n;
}

int main(int argc, char** argv) {
  const char* prog = argv[0];
  int raw = 0;
  if (argc > 1 && strcmp(argv[1], "--raw") == 0) { raw = 1; argv++; argc--; }
  if (argc < 3) { fprintf(stderr, "usage: %s [--raw] <file.vocab> <text file> [block MiB] [ids file]\n", prog); return 2; }
  const uint64_t block = (argc > 3 && atoi(argv[3]) > 0 ? (uint64_t)atoi(argv[3]) : 32u) << 20;
  FILE* vf = fopen(argv[1], "rb");
  if (!vf) { perror(argv[1]); return 2; }
  fseek(vf, 0, SEEK_END);
  const long vsz = ftell(vf);
  fseek(vf, 0, SEEK_SET);
  uint8_t* vfile = (uint8_t*)malloc((size_t)vsz + 1);
  if (!vfile || fread(vfile, 1, (size_t)vsz, vf) != (size_t)vsz) { fprintf(stderr, "%s: read error\n", argv[1]); return 2; }
  fclose(vf);
  FILE* tf = fopen(argv[2], "rb");
  if (!tf) { perror(argv[2]); return 2; }
  if (argc > 4 && !(out_file = fopen(argv[4], "wb"))) { perror(argv[4]); return 2; }

  tm_vocab* vocab = NULL;
  tm_encoder* enc = NULL;
  if (tm_vocab_load(vfile, (size_t)vsz, &vocab) != TM_OK) { fprintf(stderr, "tm_vocab_load: %s\n", tm_last_error()); return 1; }
  if (raw && !tm_encoder_raw_supported(vocab)) { fprintf(stderr, "--raw: this vocabulary's normalization needs the whole document (quotemarks, trim, leadingspace or capcode 1)\n"); return 1; }
  if (tm_encoder_new(vocab, block, &enc) != TM_OK) { fprintf(stderr, "tm_encoder_new: %s\n", tm_last_error()); return 1; }

  /* a feed returns at most the ids of the text held so far: two per byte at the very worst; TM_E_NOSPACE says what is needed and keeps the ids */
  uint8_t* text = (uint8_t*)malloc((size_t)block);
  uint64_t cap = block / 2 + 1024, n = 0, nbytes = 0;
  uint32_t* ids = (uint32_t*)malloc((size_t)cap * sizeof *ids);
  uint32_t missing = 0;
  if (!text || !ids) { fprintf(stderr, "out of memory\n"); return 2; }
  for (int last = 0; !last;) {
    const size_t got = fread(text, 1, (size_t)block, tf);
    last = got == 0;
    nbytes += got;
    int rc = last ? tm_encoder_finish(enc, ids, cap, &n, &missing) : raw ? tm_encoder_feed_raw(enc, text, got, ids, cap, &n) : tm_encoder_feed(enc, text, got, ids, cap, &n);
    if (rc == TM_E_NOSPACE) {                    /* the text has been consumed: fetch the ids with a buffer of the size reported */
      cap = n + n / 4;
      free(ids);
      if (!(ids = (uint32_t*)malloc((size_t)cap * sizeof *ids))) { fprintf(stderr, "out of memory\n"); return 2; }
      rc = tm_encoder_feed(enc, NULL, 0, ids, cap, &n);
    }
    if (rc != TM_OK) { fprintf(stderr, "tm_encoder_%s: %d %s\n", last ? "finish" : "feed", rc, tm_last_error()); return 1; }
    put(ids, n);
  }
  if (!out_file) printf("\n");
  else fclose(out_file);
  fprintf(stderr, "1 document, %llu %sbytes in blocks of %llu MiB, %llu tokens, %u missing, %llu bytes of device memory", (unsigned long long)nbytes, raw ? "raw " : "",
          (unsigned long long)(block >> 20), (unsigned long long)total, missing, (unsigned long long)tm_encoder_device_bytes(enc));
  if (raw) fprintf(stderr, ", %u pieces normalized on the host", tm_encoder_host_pieces(enc));
  fprintf(stderr, "\n");
  tm_encoder_free(enc);
  tm_vocab_free(vocab);
  fclose(tf);
  free(ids); free(text); free(vfile);
  return 0;
}

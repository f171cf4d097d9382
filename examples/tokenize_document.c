/* tokenize_document.c — tm_tokenize_document of libtokenmonster_hip.so from plain C.
 *
 *   tokenize_document [--raw] <file.vocab> <text file> [piece MiB = 32] [ids file]
 *
 * Reads the whole file and tokenizes it as ONE document in one call (already normalized bytes; with --raw: raw UTF-8, which the library cuts
 * behind line feeds and normalizes piece by piece): the pieces of N MiB run through three device workspaces at once, so that the text goes in
 * and the ids come out behind the kernels.  The ids are written four bytes each, little-endian, to the ids file, or as decimal numbers on
 * one line to stdout - the same arguments and the same output as tokenize_stream, which never holds the file whole and takes longer for it:
 * `cmp` the two ids files.  Needs an MI355X: there is no CPU path. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tokenmonster_hip.h"

static uint8_t* read_all(const char* path, uint64_t* size, int pinned) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* p = pinned ? (uint8_t*)tm_host_alloc((size_t)sz + 1) : (uint8_t*)malloc((size_t)sz + 1);
  if (!p || fread(p, 1, (size_t)sz, f) != (size_t)sz) { fprintf(stderr, "%s: read error\n", path); exit(2); }
  fclose(f);
  *size = (uint64_t)sz;
  return p;
}

int main(int argc, char** argv) {
  const char* prog = argv[0];
  int raw = 0;
  if (argc > 1 && strcmp(argv[1], "--raw") == 0) { raw = 1; argv++; argc--; }
  if (argc < 3) { fprintf(stderr, "usage: %s [--raw] <file.vocab> <text file> [piece MiB] [ids file]\n", prog); return 2; }
  const uint64_t piece = (argc > 3 && atoi(argv[3]) > 0 ? (uint64_t)atoi(argv[3]) : 32u) << 20;
  uint64_t vsz = 0, n = 0;
  uint8_t* vfile = read_all(argv[1], &vsz, 0);
  tm_vocab* vocab = NULL;
  if (tm_vocab_load(vfile, (size_t)vsz, &vocab) != TM_OK) { fprintf(stderr, "tm_vocab_load: %s\n", tm_last_error()); return 1; }
  uint8_t* text = read_all(argv[2], &n, 1);      /* page-locked: DMA'd as it lies */

  /* four bytes per id; TM_E_NOSPACE says what is needed */
  uint64_t cap = n + 4096, need = 0;
  uint8_t* ids = (uint8_t*)tm_host_alloc((size_t)cap);
  uint32_t missing = 0;
  tm_document_stats st;
  if (!ids) { fprintf(stderr, "out of memory\n"); return 2; }
  int rc = tm_tokenize_document(vocab, text, n, raw, 4, piece, 0, ids, cap, &need, &missing, NULL, &st);
  if (rc == TM_E_NOSPACE) {
    tm_host_free(ids);
    cap = need;
    if (!(ids = (uint8_t*)tm_host_alloc((size_t)cap))) { fprintf(stderr, "out of memory\n"); return 2; }
    rc = tm_tokenize_document(vocab, text, n, raw, 4, piece, 0, ids, cap, &need, &missing, NULL, &st);
  }
  if (rc != TM_OK) { fprintf(stderr, "tm_tokenize_document: %d %s\n", rc, tm_last_error()); return 1; }
  const uint64_t total = need / 4;
  if (argc > 4) {
    FILE* of = fopen(argv[4], "wb");
    if (!of) { perror(argv[4]); return 2; }
    if (total && fwrite(ids, 4, (size_t)total, of) != (size_t)total) { perror("ids file"); return 2; }
    fclose(of);
  } else {
    const uint32_t* w = (const uint32_t*)ids;
    for (uint64_t i = 0; i < total; i++) printf(i ? " %u" : "%u", w[i]);
    printf("\n");
  }
  fprintf(stderr, "1 document, %llu %sbytes in %u pieces of %llu MiB through %u slots, %llu tokens, %u missing, %llu bytes of device memory",
          (unsigned long long)n, raw ? "raw " : "", st.pieces, (unsigned long long)(piece >> 20), st.slots, (unsigned long long)total, missing,
          (unsigned long long)st.device_bytes);
  if (raw && st.host_normalized) fprintf(stderr, ", normalized on the host as a whole");
  else if (raw) fprintf(stderr, ", %u pieces normalized on the host", st.host_pieces);
  fprintf(stderr, "\n");
  tm_host_free(ids);
  tm_host_free(text);
  tm_vocab_free(vocab);
  free(vfile);
  return 0;
}

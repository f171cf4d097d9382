#!/bin/bash
# tools/emu/asan_teardown.sh — builds the library's sources for the host (tools/emu) together with tools/emu/asan_teardown.cpp under
# -fsanitize=address,undefined and runs it: a use after free or an overrun in the host layer's teardown (batches, lanes, the block cache,
# the worker pool) is reported by the sanitizers.  Arguments are passed on to the program ("leave": nothing is freed before exit).
set -e
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
CXX=${TM_EMU_CXX:-/opt/rocm/lib/llvm/bin/clang++}
OUT=${TM_ASAN_OUT:-/tmp/tm_asan}; mkdir -p "$OUT"
FLAGS="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DTM_EMU -I $ROOT/tools/emu -I $ROOT/include -I $ROOT/tokenmonster_amd/csrc -Wno-unused-result -Wno-unknown-pragmas -Wno-pass-failed"
pids=()
for f in tm_vocab.hip tm_kernels.hip tm_score.hip tm_norm.hip tm_decode.hip tm_collate.hip tm_spans.hip tm_units.hip tm_windows.hip tm_pairs.hip tm_host.hip tm_decoder.hip tm_encoder.hip tm_document.hip tm_formats.hip tm_multi.hip tm_build.cpp tm_normalize.cpp; do
  $CXX $FLAGS -x c++ -c "$ROOT/tokenmonster_amd/csrc/$f" -o "$OUT/$f.o" & pids+=($!)
done
$CXX $FLAGS -x c++ -c "$ROOT/tools/emu/emu_runtime.cpp" -o "$OUT/emu_runtime.o" & pids+=($!)
$CXX $FLAGS -x c++ -c "$ROOT/tools/emu/asan_teardown.cpp" -o "$OUT/asan_teardown.o" & pids+=($!)
for p in "${pids[@]}"; do wait $p; done
$CXX -fsanitize=address,undefined -o "$OUT/asan_teardown" "$OUT"/*.o -licuuc -licui18n -lz -lpthread -ldl
TM_TEST_HOOKS=1 ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/asan_teardown" "$@"

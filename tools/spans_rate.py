"""Time of the span pass (tm_batch_spans, tm_spans.hip) beside the emit stage of the run it follows, in the same process:

    python tools/spans_rate.py [--mib 1024] [--out profiles/spans_rate.txt]

bench.py's default shape: --mib MiB of synthetic englishcode text (bench.py's seed), the englishcode-32000-consistent vocabulary, raw text
normalized on the device, one batch.  The span pass is bracketed with HIP events (torch's) on the stream of the run; the yardstick is the
`emit` figure of tm_batch_run_timed - K4, which walks the same chains and stores 4 bytes per id where the span pass stores 8 - so the span
pass should stay within twice that.  Three warm-up calls, then the median of 20 (min .. max); tm_batch_run_timed: the median of 5 runs.
(tm_batch_spans waits for the batch's last run before it launches - host time inside the events, a few microseconds once the run is done.)
Also the collated form at L = 2048, int64, of the first 65 536 documents: the span pass into the batch's own buffer plus the gather."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from tokenmonster_amd import _native as N
from tokenmonster_amd import synth, torch_api
from tokenmonster_amd.vocab import Vocab


def timed(fn, stream, warm=3, reps=20):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join("profiles", "spans_rate.txt"))
    a = ap.parse_args()
    L = 2048
    v = Vocab(synth.config_vocab("englishcode-32000-consistent"))
    text, offs = synth.synth_corpus(synth.ENGLISHCODE, a.mib << 20, seed=0x434F5250 + 2)
    nd = offs.size - 1
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, int(text.size * 1.3) + 16 * nd + (1 << 20), nd, C.byref(b)))      # (capcode markers: the normalized text is about 1.1 x the raw text)
    N.check(N.lib.tm_batch_upload_raw(b, N.ptr(text), N.ptr(offs), nd))
    N.check(N.lib.tm_batch_normalize(b, st))
    ms = (C.c_float * N.TM_NUM_KERNELS)()
    names = [N.lib.tm_kernel_name(k).decode() for k in range(N.TM_NUM_KERNELS)]
    N.check(N.lib.tm_batch_run(b, st))
    total = C.c_uint64()
    N.check(N.lib.tm_batch_totals(b, C.byref(total), None))          # (grows the id buffer if the first run needed it: the timed runs below do not)
    runs = []
    for _ in range(6):
        N.check(N.lib.tm_batch_run_timed(b, st, ms))
        runs.append(list(ms))
    kernel_ms = {n: statistics.median(r[k] for r in runs[1:]) for k, n in enumerate(names)}
    emit = kernel_ms["emit"]
    N.check(N.lib.tm_batch_totals(b, C.byref(total), None))
    n_ids, nbytes = int(total.value), int(N.lib.tm_batch_normalized_bytes(b))
    lines = ["%d MiB of raw englishcode text, englishcode-32000-consistent, %d documents, %d normalized bytes, %d ids" % (a.mib, nd, nbytes, n_ids),
             "tm_batch_run_timed, median of 5 (ms): " + "  ".join("%s %.3f" % (n, kernel_ms[n]) for n in names)]
    print("\n".join(lines), flush=True)
    with torch.cuda.stream(stream):
        spans = torch.empty((n_ids, 2), dtype=torch.int32, device="cuda")
        med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_spans(b, st, spans.data_ptr(), n_ids)), stream)
        lines.append("span pass (tm_batch_spans)          %8.3f ms (%.3f .. %.3f)  %6.2f G ids/s, %6.1f GB/s written | emit stage %8.3f ms | ratio span / emit %.2f" % (
            med, lo, hi, n_ids / med / 1e6, n_ids * 8 / med / 1e6, emit, med / emit))
        print(lines[-1], flush=True)
        # (a look at what it wrote: no end lies before its begin)
        s = spans.to(torch.int64)
        assert bool((s[:, 1] >= s[:, 0]).all())
        del s
        ndc = min(nd, 1 << 16)                   # (the first 65 536 documents: 2 GiB of rows)
        how = torch_api._Collate(0, ndc, L, 8, v.n_ids(), N.TM_NONE, N.TM_NONE, 0)
        rows = torch.empty((ndc, L, 2), dtype=torch.int64, device="cuda")
        med2, lo2, hi2 = timed(lambda: N.check(N.lib.tm_batch_collate_spans(b, C.byref(how), st, rows.data_ptr(), 8)), stream)
        lines.append("collated, %d rows of L = %d, int64 (span pass over the batch + gather) %8.3f ms (%.3f .. %.3f)  %6.1f GB/s written" % (
            ndc, L, med2, lo2, hi2, (n_ids * 8 + ndc * L * 16) / med2 / 1e6))
        print(lines[-1], flush=True)
        # the run is what it was: the emit stage again, and the totals
        N.check(N.lib.tm_batch_run_timed(b, st, ms))
        again = C.c_uint64()
        N.check(N.lib.tm_batch_totals(b, C.byref(again), None))
        assert again.value == total.value
    N.lib.tm_batch_free(b)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

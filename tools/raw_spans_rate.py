"""What tm_batch_raw_spans costs, beside its parts as they were before it existed, in one process:

    python tools/raw_spans_rate.py [--mib 1024] [--out profiles/raw_spans_rate.txt]

On a --mib MiB batch of the benchmark's default shape (englishcode-32000-consistent, synthetic mixed text), after tm_batch_upload_raw +
tm_batch_normalize + tm_batch_run: the three parts of tm_batch_raw_spans between HIP events on the run's stream (tm_batch_raw_spans_timed: the
normalized pairs, the origin pass, the map) and their sum; tm_batch_spans alone; and tm_batch_normalize under test hook 8 - the exact
normalizer path, k_norm_summary + k_norm_carry + k_norm_emit<2>, which the origin pass redoes with owners in place of text (that call also
holds the piece table, two scans and its trips to the host).  Three warm-up calls, then the median of 20 (min .. max).  Also the size of the
origin buffer (tm_batch_device_bytes before and after the first call)."""
import argparse
import ctypes as C
import os
import statistics
import sys

os.environ.setdefault("TM_TEST_HOOKS", "1")          # (the hook-8 leg: tm_debug_flags is armed only in a process that says so)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402

from tokenmonster_amd import _native as N  # noqa: E402
from tokenmonster_amd import synth  # noqa: E402
from tokenmonster_amd.vocab import Vocab  # noqa: E402


def stat(xs):
    return "%8.3f ms (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


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
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join("profiles", "raw_spans_rate.txt"))
    a = ap.parse_args()
    v = Vocab(synth.config_vocab("englishcode-32000-consistent"))
    text, offs = synth.synth_corpus(synth.ENGLISHCODE, a.mib << 20, seed=1)
    nd = offs.size - 1
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, int(text.size) * 2 + 16 * nd + 1024, nd, C.byref(b)))
    N.check(N.lib.tm_batch_upload_raw(b, N.ptr(text), N.ptr(offs), nd))
    N.check(N.lib.tm_batch_normalize(b, st))
    N.check(N.lib.tm_batch_run(b, st))
    total = C.c_uint64()
    N.check(N.lib.tm_batch_totals(b, C.byref(total), None))
    n_ids, nbytes = int(total.value), int(N.lib.tm_batch_normalized_bytes(b))
    lines = ["%d MiB of raw englishcode-32000 text, %d documents, %d normalized bytes, %d ids; median of 20 (min .. max) after 3 warm-up calls, HIP events on the run's stream"
             % (a.mib, nd, nbytes, n_ids)]
    with torch.cuda.stream(stream):
        spans = torch.empty((n_ids, 2), dtype=torch.int32, device="cuda")
        before = int(N.lib.tm_batch_device_bytes(b))
        ms = (C.c_float * 3)()
        hd = C.c_uint32()
        parts = [[], [], []]
        for k in range(23):
            N.check(N.lib.tm_batch_raw_spans_timed(b, st, spans.data_ptr(), n_ids, C.byref(hd), ms))
            if k >= 3:
                for j in range(3):
                    parts[j].append(float(ms[j]))
        after = int(N.lib.tm_batch_device_bytes(b))
        whole = [x + y + z for x, y, z in zip(*parts)]
        plain = timed(lambda: N.check(N.lib.tm_batch_spans(b, st, spans.data_ptr(), n_ids)), stream)
        N.lib.tm_debug_flags(256)
        exact = timed(lambda: N.check(N.lib.tm_batch_normalize(b, st)), stream)
        N.lib.tm_debug_flags(0)
    med = statistics.median
    lines += [
        "tm_batch_raw_spans, normalized pairs   " + stat(parts[0]),
        "tm_batch_raw_spans, origin pass        " + stat(parts[1]) + "   (%d documents mapped on the host)" % hd.value,
        "tm_batch_raw_spans, map (k_raw_spans)  " + stat(parts[2]),
        "tm_batch_raw_spans, whole              " + stat(whole),
        "tm_batch_spans                         " + stat(plain),
        "tm_batch_normalize under hook 8 (exact)" + stat(exact),
        "whole / (tm_batch_spans + exact normalizer path) = %.2f" % (med(whole) / (med(plain) + med(exact))),
        "origin pass / exact normalizer path = %.2f; map / tm_batch_spans = %.2f" % (med(parts[1]) / med(exact), med(parts[2]) / med(plain)),
        "grow-only buffers of the first call (owners, the batch's own pairs, scratch): %.1f MiB = %.2f bytes per normalized byte" % ((after - before) / 2**20, (after - before) / max(nbytes, 1)),
    ]
    for l in lines:
        print(l, flush=True)
    N.lib.tm_batch_free(b)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

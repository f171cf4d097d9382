"""What character offsets cost beside the parts of the raw-span call they ride on, in one process:

    python tools/span_units_rate.py [--mib 256] [--out profiles/span_units.txt]

One batch of --mib MiB of the benchmark's default shape (englishcode-32000-consistent, synthetic mixed text).  For each unit - bytes, code
points, UTF-16 - tm_batch_spans_in(TM_TEXT_RAW, unit, ms) after tm_batch_upload_raw + tm_batch_normalize + tm_batch_run, its four parts
between HIP events on the run's stream, per GiB of raw text: ms[0] the normalized pairs, ms[1] the origin pass, ms[2] the map, ms[3] the unit
work.  "first": the call behind a fresh upload, whose ms[3] holds the index pass over the text, the scan and the conversion (median of 5
uploads); "cached": the calls behind it on the same run, whose ms[3] is the conversion alone (median of 10).  The yardstick is traffic: the
index pass reads the text once and writes at most an eighth of it, the origin pass (ms[1]) reads the same text and writes 4 bytes per
normalized byte - ms[3] of a first call should lie below its ms[1].  Also the size of the index (tm_batch_device_bytes around the first call)."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402

from tokenmonster_amd import _native as N  # noqa: E402
from tokenmonster_amd import synth  # noqa: E402
from tokenmonster_amd.vocab import Vocab  # noqa: E402

UNITS = [("bytes", N.TM_UNIT_BYTES), ("code points", N.TM_UNIT_CODEPOINTS), ("utf-16", N.TM_UNIT_UTF16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "span_units.txt"))
    a = ap.parse_args()
    v = Vocab(synth.config_vocab("englishcode-32000-consistent"))
    text, offs = synth.synth_corpus(synth.ENGLISHCODE, a.mib << 20, seed=1)
    nd = offs.size - 1
    per_gib = 1024.0 / a.mib
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, int(text.size) * 2 + 16 * nd + 1024, nd, C.byref(b)))

    def run():
        N.check(N.lib.tm_batch_upload_raw(b, N.ptr(text), N.ptr(offs), nd))
        N.check(N.lib.tm_batch_normalize(b, st))
        N.check(N.lib.tm_batch_run(b, st))
        total = C.c_uint64()
        N.check(N.lib.tm_batch_totals(b, C.byref(total), None))
        return int(total.value)

    n_ids = run()
    nbytes = int(N.lib.tm_batch_normalized_bytes(b))
    lines = ["%d MiB of raw englishcode-32000 text, %d documents, %d normalized bytes, %d ids; ms per GiB of raw text, HIP events on the run's stream"
             % (a.mib, nd, nbytes, n_ids),
             "%-12s %-7s %10s %10s %10s %10s" % ("unit", "call", "ms[0]", "ms[1]", "ms[2]", "ms[3]")]
    verdict = []
    with torch.cuda.stream(stream):
        spans = torch.empty((n_ids, 2), dtype=torch.int32, device="cuda")
        ms = (C.c_float * 4)()
        hd = C.c_uint32()

        def call(unit):
            N.check(N.lib.tm_batch_spans_in(b, st, N.TM_TEXT_RAW, unit, spans.data_ptr(), n_ids, C.byref(hd), ms))
            return [float(ms[k]) * per_gib for k in range(4)]

        call(N.TM_UNIT_BYTES)                              # (the grow-only buffers of the raw-span call exist from here on)
        before = int(N.lib.tm_batch_device_bytes(b))
        call(N.TM_UNIT_UTF16)
        index_bytes = int(N.lib.tm_batch_device_bytes(b)) - before
        for name, unit in UNITS:
            first, cached = [], []
            for _ in range(5):
                assert run() == n_ids
                first.append(call(unit))
            for _ in range(10):
                cached.append(call(unit))
            for what, rows in (("first", first), ("cached", cached)):
                med = [statistics.median(r[k] for r in rows) for k in range(4)]
                lines.append("%-12s %-7s %10.3f %10.3f %10.3f %10.3f" % (name, what, med[0], med[1], med[2], med[3]))
                if what == "first" and unit != N.TM_UNIT_BYTES:
                    verdict.append("%s: ms[3] / ms[1] of a first call = %.2f (%s the origin pass)" % (name, med[3] / max(med[1], 1e-9), "below" if med[3] < med[1] else "NOT below"))
    lines += verdict
    lines.append("the index, both planes: %.2f MiB = %.4f bytes per byte of raw text (%d documents mapped on the host)" % (index_bytes / 2**20, index_bytes / max(int(text.size), 1), hd.value))
    for l in lines:
        print(l, flush=True)
    N.lib.tm_batch_free(b)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""ONE large raw document host to host, three ways in the same process - the shape of the reference's own benchmark, one Vocab.tokenize of a
whole file (benchmark/tokenmonster_bench.go):

    python tools/document_rate.py [--mib 1024] [--reps 7] [--out profiles/document_rate.json]

The benchmark corpus (englishcode-32000 shape) as ONE document of --mib MiB of raw text in page-locked memory, ids into page-locked memory:

    document   tm_tokenize_document: pieces of 32 MiB through three slots, upload | match | resolve + emit | download overlapped
    encoder    the streaming encoder, tm_encoder_feed_raw in blocks of 32 MiB + tm_encoder_finish: one pass behind the other
    pipeline   tm_tokenize_pipeline with ndocs = 1: the whole document one chunk, upload, kernels, download one after the other

Every call returns with its ids on the host, so a host clock around it is the time.  One warm-up round (it makes the workspaces), then --reps
rounds that run the three one after the other - alternating, so that whatever else the host is doing falls on all three -, the median of
each, and its spread (max - min).  The ids of the three are compared before anything is printed.  One JSON line, also written to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from tokenmonster_amd import _native as N
from tokenmonster_amd import synth
from tokenmonster_amd.vocab import DocumentStats, PinnedBuffer, Vocab

BLOCK = 32 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--piece-mib", type=int, default=32)
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "document_rate.json"))
    a = ap.parse_args()
    v = Vocab(synth.config_vocab("englishcode-32000-consistent"))
    text, _ = synth.synth_corpus(synth.ENGLISHCODE, a.mib << 20, seed=1)
    n = int(text.size)
    pin_in = PinnedBuffer(n)
    pin_in.array[:] = text
    del text
    cap = (n + n // 2) // 4 * 4                     # bytes of ids, four each: this text has about one id per five bytes
    outs = {k: PinnedBuffer(cap) for k in ("document", "encoder", "pipeline")}
    offs = np.array([0, n], dtype=np.uint64)
    stats = DocumentStats()
    result = {}

    def document():
        need, miss = C.c_uint64(), C.c_uint32()
        N.check(N.lib.tm_tokenize_document(v.handle, N.ptr(pin_in.array), n, 1, 4, a.piece_mib << 20, a.slots, N.ptr(outs["document"].array), cap,
                                           C.byref(need), C.byref(miss), None, C.byref(stats)))
        result["document"] = (int(need.value) // 4, int(miss.value))

    enc = C.c_void_p()
    N.check(N.lib.tm_encoder_new(v.handle, BLOCK, C.byref(enc)))

    def encoder():
        ids = outs["encoder"].array.view("<u4")
        got, k = 0, C.c_uint64()
        for pos in range(0, n, BLOCK):
            N.check(N.lib.tm_encoder_feed_raw(enc, N.ptr(pin_in.array[pos:pos + BLOCK]), min(BLOCK, n - pos), N.ptr(ids[got:]), ids.size - got, C.byref(k)))
            got += int(k.value)
        miss = C.c_uint32()
        N.check(N.lib.tm_encoder_finish(enc, N.ptr(ids[got:]), ids.size - got, C.byref(k), C.byref(miss)))
        result["encoder"] = (got + int(k.value), int(miss.value))

    def pipeline():
        boff = np.zeros(2, dtype=np.uint64)
        miss = np.zeros(1, dtype=np.uint32)
        N.check(N.lib.tm_tokenize_pipeline(v.handle, N.ptr(pin_in.array), N.ptr(offs), 1, 1, 4, 0, 0, N.ptr(outs["pipeline"].array), cap, N.ptr(boff), N.ptr(miss),
                                           None, None))
        result["pipeline"] = (int(boff[1]) // 4, int(miss[0]))

    ways = {"document": document, "encoder": encoder, "pipeline": pipeline}
    ms = {k: [] for k in ways}
    for rep in range(a.reps + 1):
        for name, fn in ways.items():
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep > 0:
                ms[name].append(dt)
        if rep == 0:      # the ids of all three are equal - or nothing is reported
            ntok, miss = result["document"]
            ref = outs["document"].array[:ntok * 4]
            for name in ("encoder", "pipeline"):
                assert result[name] == (ntok, miss), (name, result[name], (ntok, miss))
                assert np.array_equal(outs[name].array[:ntok * 4], ref), "%s: ids differ from tm_tokenize_document's" % name
    N.lib.tm_encoder_free(enc)
    line = {"what": "one raw document host to host", "vocab": "englishcode-32000-consistent", "raw_bytes": n, "ids": result["document"][0], "missing": result["document"][1],
            "reps": a.reps, "piece_bytes": a.piece_mib << 20}
    for name in ways:
        med = statistics.median(ms[name])
        line[name] = {"median_ms": round(med, 3), "min_ms": round(min(ms[name]), 3), "max_ms": round(max(ms[name]), 3),
                      "spread_ms": round(max(ms[name]) - min(ms[name]), 3), "GBps": round(n / med / 1e6, 2)}
    best = min(("encoder", "pipeline"), key=lambda k: line[k]["median_ms"])
    spread = max(line["document"]["spread_ms"], line[best]["spread_ms"])
    line["best_parent_path"] = best
    line["document_faster_by_ms"] = round(line[best]["median_ms"] - line["document"]["median_ms"], 3)
    line["faster_by_more_than_the_spread"] = bool(line["document_faster_by_ms"] > spread)
    line["stats"] = {k: getattr(stats, k) for k, _ in DocumentStats._fields_}
    s = json.dumps(line)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")
    print(s, flush=True)


if __name__ == "__main__":
    main()

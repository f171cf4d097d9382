"""Host-to-host rate of the streaming encoder against the one-call path, on ONE document (profiles/stream_encoder.txt).

  python tools/stream_encoder_rate.py --mode encoder [--mib 256] [--piece-mib 32] [--reps 3]
  python tools/stream_encoder_rate.py --mode batch   [--mib 256] [--reps 3] [--lib path/to/another/build/libtokenmonster_hip.so]

encoder: tm_encoder_feed over pieces of --piece-mib MiB + tm_encoder_finish; batch: tm_tokenize_batch of the same bytes in one call (--lib: the
library of another build, e.g. the parent commit's, bound through ctypes by itself).  Both take the text from and return the ids to pageable
host buffers and wait for them.  Text: the synthetic englishcode corpus, normalized, cut to --mib MiB; vocabulary: englishcode-32000-consistent.
Prints one JSON line: ids, seconds of every repetition, ids per second of the best one, device bytes of the workspace."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["encoder", "batch"], required=True)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--piece-mib", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    from tokenmonster_amd import _native as N, synth
    total = a.mib << 20
    img = np.frombuffer(synth.config_vocab("englishcode-32000-consistent"), dtype=np.uint8)
    raw, offs = synth.synth_corpus(synth.ENGLISHCODE, total + (1 << 20), seed=7)
    ntext, _ = synth.normalize_batch(raw, offs, 2, 1)
    data = np.ascontiguousarray(ntext[:total])
    assert data.size == total
    del raw, ntext
    lib = N.lib
    if a.lib:
        lib = C.CDLL(a.lib)
        for name, (res, args) in N.SIGNATURES.items():
            if hasattr(lib, name):              # (an older build has no tm_encoder_*)
                getattr(lib, name).restype, getattr(lib, name).argtypes = res, args

    def check(rc):
        if rc != 0:
            raise RuntimeError("error %d: %s" % (rc, (lib.tm_last_error() or b"").decode(errors="replace")))
    v = C.c_void_p()
    check(lib.tm_vocab_load(N.ptr(img), img.size, C.byref(v)))
    out = np.empty(total // 2 + 4096, dtype=np.uint32)
    out[:] = 0                      # (pages touched before the clock starts)
    secs, nids, dev = [], 0, 0
    if a.mode == "batch":
        offsets = np.array([0, total], dtype=np.uint64)
        toff = np.zeros(2, dtype=np.uint64)
        miss = np.zeros(1, dtype=np.uint32)
        for rep in range(a.reps + 1):          # (the first one warms up: workspace, staging)
            t0 = time.perf_counter()
            check(lib.tm_tokenize_batch(v, N.ptr(data), N.ptr(offsets), 1, N.ptr(out), out.size, N.ptr(toff), N.ptr(miss)))
            secs.append(time.perf_counter() - t0)
            nids = int(toff[1])
        b = C.c_void_p()                       # what the call's lane holds for this document (tm_host.hip: bytes + a quarter + 1 MiB)
        check(lib.tm_batch_create(v, total + total // 4 + (1 << 20), 65, C.byref(b)))
        dev = int(lib.tm_batch_device_bytes(b))
        lib.tm_batch_free(b)
    else:
        piece = a.piece_mib << 20
        e = C.c_void_p()
        check(lib.tm_encoder_new(v, piece, C.byref(e)))
        n = C.c_uint64()
        miss = C.c_uint32()
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            got = 0
            for p in range(0, total, piece):
                m = min(piece, total - p)
                check(lib.tm_encoder_feed(e, data.ctypes.data + p, m, out.ctypes.data + 4 * got, out.size - got, C.byref(n)))
                got += int(n.value)
            check(lib.tm_encoder_finish(e, out.ctypes.data + 4 * got, out.size - got, C.byref(n), C.byref(miss)))
            got += int(n.value)
            secs.append(time.perf_counter() - t0)
            nids = got
        dev = int(lib.tm_encoder_device_bytes(e))
        lib.tm_encoder_free(e)
    lib.tm_vocab_free(v)
    best = min(secs[1:])
    print(json.dumps({"mode": a.mode, "lib": a.lib or "this build", "mib": a.mib, "piece_mib": a.piece_mib if a.mode == "encoder" else None, "ids": nids,
                      "ids_crc": int(np.bitwise_xor.reduce(out[:nids].astype(np.uint64) * np.arange(1, nids + 1, dtype=np.uint64) & 0xFFFFFFFF)),
                      "warmup_s": round(secs[0], 4), "seconds": [round(s, 4) for s in secs[1:]], "ids_per_s": round(nids / best), "bytes_per_s": round(total / best),
                      "device_bytes": dev}))


if __name__ == "__main__":
    main()

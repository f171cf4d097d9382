"""Rates of the layout kernels (tm_collate.hip) beside a device-to-device copy of the same byte count, in the same run:

    python tools/collate_rate.py [--mib 256] [--out profiles/collate.txt]

collate at int64 and pack at uint16 (both L = 2048) and load_ids of the int64 rows, on the ids of a --mib MiB batch of the benchmark's
englishcode-32000 shape.  HIP events (torch's) around the launches on ONE stream; GB/s counts the bytes a call reads plus the bytes it writes;
the yardstick is hipMemcpyAsync device to device of that many bytes (half read, half written), timed the same way.  Three warm-up calls, then
the median of 20.  (tm_batch_collate / tm_batch_pack wait for the batch's last run before they launch and tm_batch_pack_rows fetches two
offsets: host time, outside the kernels but inside the events - with 256 MiB of text it is a few percent of a call.)"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
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
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "collate.txt"))
    a = ap.parse_args()
    L = 2048
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
    n_ids, pad, eos = int(total.value), v.n_ids(), v.n_ids() + 1
    lines = ["%d MiB of englishcode-32000 text, %d documents, %d ids, L = %d; median of 20 (min .. max), GB/s = bytes read + written" % (a.mib, nd, n_ids, L)]

    def copy_rate(nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(stream):
            med, lo, hi = timed(lambda: dst.copy_(src, non_blocking=True), stream)
        return nbytes / med / 1e6, med

    def report(name, nbytes, med, lo, hi):
        gbs = nbytes / med / 1e6
        cgbs, cmed = copy_rate(nbytes)
        lines.append("%-34s %8.3f ms (%.3f .. %.3f)  %7.1f GB/s | copy of %d MB: %8.3f ms %7.1f GB/s | ratio %.2f" % (name, med, lo, hi, gbs, nbytes >> 20, cmed, cgbs, gbs / cgbs))
        print(lines[-1], flush=True)

    with torch.cuda.stream(stream):
        # collate, int64: reads the ids a row keeps (at most L each), writes rows * L * (8 + 1) + rows * 4
        how = torch_api._Collate(0, nd, L, 8, pad, N.TM_NONE, N.TM_NONE, 0)
        ids = torch.empty((nd, L), dtype=torch.int64, device="cuda")
        mask = torch.empty((nd, L), dtype=torch.uint8, device="cuda")
        lens = torch.empty((nd,), dtype=torch.int32, device="cuda")
        med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_collate(b, C.byref(how), st, ids.data_ptr(), mask.data_ptr(), lens.data_ptr())), stream)
        kept = int(lens.to(torch.int64).sum().item())
        report("collate int64 + mask + lengths", kept * 4 + nd * L * 9 + nd * 4, med, lo, hi)
        # pack, uint16: reads every id, writes rows * L * (2 + 4 + 4)
        howp = torch_api._Collate(0, nd, L, 2, pad, N.TM_NONE, eos, 0)
        rows = C.c_uint64()
        N.check(N.lib.tm_batch_pack_rows(b, C.byref(howp), C.byref(rows)))
        r = int(rows.value)
        pids = torch.empty((r, L), dtype=torch.int16, device="cuda")
        pdi = torch.empty((r, L), dtype=torch.int32, device="cuda")
        ppo = torch.empty((r, L), dtype=torch.int32, device="cuda")
        med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_pack(b, C.byref(howp), st, r, pids.data_ptr(), pdi.data_ptr(), ppo.data_ptr())), stream)
        report("pack uint16 + doc_index + position", n_ids * 4 + r * L * 10, med, lo, hi)
        # load_ids of the int64 rows: the extents pass reads every element once, the gather reads the kept ones again and writes them as uint32
        b2 = C.c_void_p()
        N.check(N.lib.tm_batch_create(v.handle, 4096, nd, C.byref(b2)))
        med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_load_ids(b2, ids.data_ptr(), nd, L, 8, lens.data_ptr(), pad, N.TM_NONE, N.TM_NONE, st)), stream)
        report("load_ids int64 rows", nd * L * 8 + kept * 12 + nd * 16, med, lo, hi)
    N.lib.tm_batch_free(b2)
    N.lib.tm_batch_free(b)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

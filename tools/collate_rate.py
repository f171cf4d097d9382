"""Rates of the layout kernels (tm_collate.hip) beside a device-to-device copy of the same byte count, in the same run:

    python tools/collate_rate.py [--mib 256] [--out profiles/collate.txt] [--only pairs] [--append]

collate at int64 and pack at uint16 (both L = 2048), windows at int64 beside a collate of the same output element count (L = 256 and L = 2048) and load_ids
of the int64 rows, and text pairs and pair windows at int64 and L = 512 beside a collate of the same output element count (the batch's documents paired
first half against second half), on the ids of a --mib MiB batch of the benchmark's
englishcode-32000 shape.  HIP events (torch's) around the launches on ONE stream; GB/s counts the bytes a call reads plus the bytes it writes;
the yardstick is hipMemcpyAsync device to device of that many bytes (half read, half written), timed the same way.  Three warm-up calls, then
the median of 20.  --only pairs: the pair lines alone; --append: add to --out under a dated heading instead of replacing it.  (tm_batch_collate / tm_batch_pack wait for the batch's last run before they launch and tm_batch_pack_rows fetches two
offsets: host time, outside the kernels but inside the events - with 256 MiB of text it is a few percent of a call.)"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

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
    ap.add_argument("--only", choices=["pairs"], default=None)
    ap.add_argument("--append", action="store_true")
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
    lines = ["%d MiB of englishcode-32000 text, %d documents, %d ids, L = %s; median of 20 (min .. max), GB/s = bytes read + written" % (
        a.mib, nd, n_ids, "512" if a.only == "pairs" else "%d (the pair lines: 512)" % L)]

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

    def pairs_lines():
        """pairs and pair windows, int64, L = 512: document p against document nd / 2 + p.  Beside each a collate of the SAME output element count
        with the outputs a collate has (ids, mask, a count per row), the pair fill once with exactly those (ids, mask, kept) and once with the
        types too, and the copy yardstick of report().  A pair row's plan is four offset loads where a collate row's is two."""
        LP, n = 512, nd // 2
        pids = torch.empty((nd, LP), dtype=torch.int64, device="cuda")
        pmask = torch.empty((nd, LP), dtype=torch.uint8, device="cuda")
        ptype = torch.empty((nd, LP), dtype=torch.uint8, device="cuda")
        pkept = torch.empty((nd, 2), dtype=torch.int32, device="cuda")
        plens, prow, pstart = (torch.empty((nd,), dtype=torch.int32, device="cuda") for _ in range(3))
        sep = eos + 1

        def pair_how(k, trunc):
            return N.Pair(0, n, k, LP, 8, pad, N.TM_NONE, sep, N.TM_NONE, 1, trunc, 0)

        def collate_line(rows):
            howc = torch_api._Collate(0, rows, LP, 8, pad, N.TM_NONE, N.TM_NONE, 0)
            med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_collate(b, C.byref(howc), st, pids.data_ptr(), pmask.data_ptr(), plens.data_ptr())), stream)
            keptc = int(plens[:rows].to(torch.int64).sum().item())
            report("collate int64, %d rows of %d" % (rows, LP), keptc * 4 + rows * LP * 9 + rows * 4, med, lo, hi)
            lines.append("  (collate's spread over its 20 repetitions: %.3f ms)" % (hi - lo))
            return med, hi - lo

        cmed, spread = collate_line(n)
        howp = pair_how(n, N.TM_PAIR_LONGEST_FIRST)
        med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_pair(b, C.byref(howp), st, pids.data_ptr(), pmask.data_ptr(), None, pkept.data_ptr())), stream)
        keptp = int(pkept[:n].to(torch.int64).sum().item())
        report("pairs int64 + mask + kept, %d rows" % n, keptp * 4 + n * LP * 9 + n * 8, med, lo, hi)
        lines.append("  (pairs less collate at the same element count: %+.3f ms, collate's spread %.3f ms)" % (med - cmed, spread))
        med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_pair(b, C.byref(howp), st, pids.data_ptr(), pmask.data_ptr(), ptype.data_ptr(), pkept.data_ptr())), stream)
        report("pairs int64 + mask + types + kept", keptp * 4 + n * LP * 10 + n * 8, med, lo, hi)
        # pair windows: A cut to MF ids, OV ids of B shared between rows, over the first pairs whose windows make at most nd rows
        OV, MF = 64, 64
        need = C.c_uint64()

        def pair_window_rows(k):
            N.check(N.lib.tm_batch_pair_window_rows(b, C.byref(pair_how(k, N.TM_PAIR_ONLY_SECOND)), OV, MF, C.byref(need)))
            return int(need.value)

        lo_p, hi_p = 1, n
        while lo_p < hi_p:
            mid = (lo_p + hi_p + 1) // 2
            lo_p, hi_p = (mid, hi_p) if pair_window_rows(mid) <= nd else (lo_p, mid - 1)
        k, rw = lo_p, pair_window_rows(lo_p)
        howw = pair_how(k, N.TM_PAIR_ONLY_SECOND)
        cmed, spread = collate_line(rw)

        def windows(types):
            N.check(N.lib.tm_batch_pair_windows(b, C.byref(howw), OV, MF, st, rw, pids.data_ptr(), pmask.data_ptr(), types, pkept.data_ptr(), prow.data_ptr(), pstart.data_ptr()))

        med, lo, hi = timed(lambda: windows(None), stream)
        keptw = int(pkept[:rw].to(torch.int64).sum().item())
        report("pair windows int64 + mask + kept + maps", keptw * 4 + rw * LP * 9 + rw * 16, med, lo, hi)
        rmed, rlo, rhi = timed(lambda: pair_window_rows(k), stream)
        lines.append("  pair_window_rows alone              %8.3f ms (%.3f .. %.3f)  -> row pairs + fill: %.3f ms; less collate: %+.3f ms, collate's spread %.3f ms" % (
            rmed, rlo, rhi, med - rmed, med - rmed - cmed, spread))
        med, lo, hi = timed(lambda: windows(ptype.data_ptr()), stream)
        report("pair windows, the types too", keptw * 4 + rw * LP * 10 + rw * 16, med, lo, hi)
        lines.append("(pair windows: %d pairs -> %d rows, max_first %d, overlap %d; a call = tm_batch_pair_window_rows' work, then the row pairs and the fill)" % (k, rw, MF, OV))

    def write_out():
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            if a.append:
                f.write("\n==== %s: tools/collate_rate.py%s ====\n" % (time.strftime("%Y-%m-%d"), " --only " + a.only if a.only else ""))
            f.write("\n".join(lines) + "\n")

    if a.only == "pairs":
        with torch.cuda.stream(stream):
            pairs_lines()
        N.lib.tm_batch_free(b)
        write_out()
        return
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
        # windows, int64, beside a collate of the SAME output element count: rows of LW ids with OV shared, over the first documents whose
        # windows make at most nd rows (bisection over tm_batch_window_rows), and a collate of that many documents at LW.  In front of the fill
        # kernels a windows call finds the document of every row (k_window_row_docs: one binary search per row); the fill then differs from
        # the collate's by one load of that map per row it touches, and reads every id (the collate only what a row keeps)
        def windows_pair(LW, OV):
            need = C.c_uint64()

            def window_rows(k):
                hw = torch_api._Collate(0, k, LW, 8, pad, N.TM_NONE, N.TM_NONE, 0)
                N.check(N.lib.tm_batch_window_rows(b, C.byref(hw), OV, C.byref(need)))
                return int(need.value)

            lo_d, hi_d = 1, nd
            while lo_d < hi_d:
                mid = (lo_d + hi_d + 1) // 2
                lo_d, hi_d = (mid, hi_d) if window_rows(mid) <= nd else (lo_d, mid - 1)
            ndw, rw = lo_d, window_rows(lo_d)
            howw = torch_api._Collate(0, ndw, LW, 8, pad, N.TM_NONE, N.TM_NONE, 0)
            howc = torch_api._Collate(0, rw, LW, 8, pad, N.TM_NONE, N.TM_NONE, 0)
            wids = torch.empty((rw, LW), dtype=torch.int64, device="cuda")
            wmask = torch.empty((rw, LW), dtype=torch.uint8, device="cuda")
            wlens = torch.empty((rw,), dtype=torch.int32, device="cuda")
            for rep in range(3):                                         # (repeated: the spread of the collate runs is the noise to read the pair against)
                med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_collate(b, C.byref(howc), st, wids.data_ptr(), wmask.data_ptr(), wlens.data_ptr())), stream)
                keptc = int(wlens.to(torch.int64).sum().item())
                report("collate int64, %d rows of %d [%d]" % (rw, LW, rep), keptc * 4 + rw * LW * 9 + rw * 4, med, lo, hi)
                med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_windows(b, C.byref(howw), OV, st, rw, wids.data_ptr(), wmask.data_ptr(), wlens.data_ptr(), None, None)), stream)
                keptw = int(wlens.to(torch.int64).sum().item())
                report("windows int64, %d rows of %d [%d]" % (rw, LW, rep), keptw * 4 + rw * LW * 9 + rw * 4, med, lo, hi)
                # the part of a windows call in front of k_window_row_docs and the fill - count, scan, one 8-byte read-back, a wait for the stream - is
                # tm_batch_window_rows; what is left holds the row-docs kernel too
                rmed, rlo, rhi = timed(lambda: window_rows(ndw), stream)
                lines.append("window_rows alone [%d]                 %8.3f ms (%.3f .. %.3f)  -> row docs + fill: windows less window_rows = %.3f ms" % (rep, rmed, rlo, rhi, med - rmed))
                print(lines[-1], flush=True)
            lines.append("(windows: %d documents -> %d rows, overlap %d; a call = tm_batch_window_rows' work, then the row docs and the fill)" % (ndw, rw, OV))

        windows_pair(256, 32)          # 19 M elements: the outputs stay in the cache, latency shows
        windows_pair(2048, 256)        # 154 M elements: bound by HBM bytes like the collate line above
        # load_ids of the int64 rows: the extents pass reads every element once, the gather reads the kept ones again and writes them as uint32
        b2 = C.c_void_p()
        N.check(N.lib.tm_batch_create(v.handle, 4096, nd, C.byref(b2)))
        med, lo, hi = timed(lambda: N.check(N.lib.tm_batch_load_ids(b2, ids.data_ptr(), nd, L, 8, lens.data_ptr(), pad, N.TM_NONE, N.TM_NONE, st)), stream)
        report("load_ids int64 rows", nd * L * 8 + kept * 12 + nd * 16, med, lo, hi)
        pairs_lines()
    N.lib.tm_batch_free(b2)
    N.lib.tm_batch_free(b)
    write_out()


if __name__ == "__main__":
    main()

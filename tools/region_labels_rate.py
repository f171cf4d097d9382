"""What region labels cost beside the span pass they ride on, in one process:

    python tools/region_labels_rate.py [--mib 256] [--out profiles/region_labels.txt]

One batch of --mib MiB of the benchmark's default shape (englishcode-32000-consistent, synthetic mixed text) after tm_batch_upload_raw +
tm_batch_normalize + tm_batch_run, one region per 20 ids (the pair of every 20th id, made on the device from the pairs themselves).  Per text and
unit, between events on the run's stream, three warm-ups and the median of 20: tm_batch_spans_in (the yardstick: the parent's code),
tm_batch_region_labels with labels only (the span pass, the documents' lengths, k_region_labels) and with the token ranges and the count of
regions out of order too (which reads the number of regions back once).  Beyond the span pass the label kernel reads 8 and writes 4 bytes per
id: the difference of the two calls is held against the span pass and against a device-to-device copy of the same traffic, 6 bytes per id
read and 6 written (the convention of tools/collate_rate.py)."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tokenmonster_amd import _native as N  # noqa: E402
from tokenmonster_amd import synth  # noqa: E402
from tokenmonster_amd.vocab import Vocab  # noqa: E402

FORMS = [("normalized, bytes", N.TM_TEXT_NORMALIZED, N.TM_UNIT_BYTES), ("raw, code points", N.TM_TEXT_RAW, N.TM_UNIT_CODEPOINTS), ("raw, utf-16", N.TM_TEXT_RAW, N.TM_UNIT_UTF16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "region_labels.txt"))
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
    n = int(total.value)
    lines = ["%d MiB of raw englishcode-32000 text, %d documents, %d ids, one region per 20 ids; median of 20 (min .. max) after 3 warm-ups" % (a.mib, nd, n)]

    def timed(fn):
        ms = []
        for k in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if k >= 3:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    with torch.cuda.stream(stream):
        spans = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        labels = torch.empty((n,), dtype=torch.int32, device="cuda")
        toff = torch.empty((nd + 1,), dtype=torch.int64, device="cuda")
        N.check(N.lib.tm_device_copy(toff.data_ptr(), N.lib.tm_batch_device_tok_offsets(b), 8 * (nd + 1)))
        src, dst = torch.empty((6 * n,), dtype=torch.uint8, device="cuda"), torch.empty((6 * n,), dtype=torch.uint8, device="cuda")
        copy = timed(lambda: dst.copy_(src))
        lines.append("device-to-device copy of 6 bytes per id to 6 bytes per id (%d MB read + written, the label kernel's 8 + 4): %.3f ms (%.3f .. %.3f)" % (12 * n // 10**6, *copy))
        for name, kind, unit in FORMS:
            def spans_in():
                N.check(N.lib.tm_batch_spans_in(b, st, kind, unit, spans.data_ptr(), n, None, None))
            t_spans = timed(spans_in)
            stream.synchronize()
            reg = torch.cat([spans[::20], torch.arange(spans[::20].shape[0], dtype=torch.int32, device="cuda")[:, None] % 9 - 2], dim=1).contiguous()
            roff = ((toff + 19) // 20).contiguous()
            rtok = torch.empty((reg.shape[0], 2), dtype=torch.int32, device="cuda")
            bad = torch.zeros((1,), dtype=torch.int32, device="cuda")
            stream.synchronize()
            rg = N.Regions(roff.data_ptr(), reg.data_ptr(), kind, unit, -100)

            def only_labels():
                N.check(N.lib.tm_batch_region_labels(b, st, C.byref(rg), labels.data_ptr(), 4, n, None, None, None))

            def everything():
                N.check(N.lib.tm_batch_region_labels(b, st, C.byref(rg), labels.data_ptr(), 4, n, rtok.data_ptr(), bad.data_ptr(), None))
            t_lab, t_all = timed(only_labels), timed(everything)
            stream.synchronize()
            lines.append("%-18s tm_batch_spans_in %.3f ms (%.3f .. %.3f) | region_labels, labels only %.3f ms (%.3f .. %.3f) | with token ranges and count %.3f ms (%.3f .. %.3f)"
                         % (name, *t_spans, *t_lab, *t_all))
            extra = t_lab[0] - t_spans[0]
            lines.append("%-18s labels beyond the span pass: %.3f ms = %.2f of the span pass, %.2f of the copy; %d regions, %d out of order, %d ids labelled"
                         % ("", extra, extra / t_spans[0], extra / copy[0], reg.shape[0], int(bad.item()), int((labels != -100).sum().item())))
    for l in lines:
        print(l, flush=True)
    N.lib.tm_batch_free(b)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

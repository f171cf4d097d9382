"""-m gpu: the grow-only buffers a batch owns (tm_batch_device_bytes: ids, spans, origins and their scratch, the unit index of both texts, windows,
window rows) over rounds of raw text of different sizes on ONE batch - small, large, small again, many tiny documents, small again.  Every output
of every round is what a fresh batch gives that has seen only that round; the byte count never falls, and a round the batch has grown for already
changes nothing and replaces no buffer.  tests/test_batch_buffers_emulated.py runs this file on the emulated device (tools/emu), without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from fixed_shape import Collate, Out, NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM, RAW = 0, 1                     # TM_TEXT_*
CODEPOINTS, UTF16 = 1, 2             # TM_UNIT_*
WINDOW_LEN, OVERLAP = 64, 8
MAX_BYTES, MAX_DOCS = 1 << 18, 1300  # the batch: its id buffer starts at MAX_BYTES / 2 + 2 * MAX_DOCS + 1024 ids, fewer than the large round makes
pytestmark = pytest.mark.gpu


def _mods():
    import tokenmonster_amd as tm
    from tokenmonster_amd import _native as N, synth
    return tm, N, synth


def make_vocab():
    """a..t, the capcode markers and some punctuation as tokens of one byte, 'é' and its parts; an emoji has no token (unk ids)"""
    tm, _, synth = _mods()
    toks = {bytes([c]) for c in b"abcdefghijklmnopqrst .,'\nDCW"} | {"é".encode(), "́".encode(), b" a", b"ab", b" the"}
    return tm.Vocab(synth.build_vocab(sorted(toks), capcode=2, charset=1, norm_flag=1, with_unk=True))


def text(rng, n):
    """about n bytes: words of a..t, a capital here and there, 'é' (two bytes, two UTF-8 forms after NFD) and an emoji (four bytes, two UTF-16 units)"""
    out = []
    size = 0
    while size < n:
        w = "".join("abcdefghijklmnopqrst"[int(x)] for x in rng.integers(0, 20, size=int(rng.integers(1, 9))))
        k = int(rng.integers(0, 40))
        w = w.capitalize() if k < 3 else w + "é" if k == 3 else w + "\U0001F600" if k == 4 else "the" if k == 5 else w
        out.append(w)
        size += len(w.encode()) + 1
    return " ".join(out).encode()


def rounds():
    """name -> (documents, row length of the collate calls).  large: every buffer sized by text, ids or rows is too small for it after `small`
    (the collated rows hold more ids than the batch's id buffer, for tm_batch_load_ids); wide: more documents than the headroom of the buffers
    sized by documents (windows, the origin pass's scratch)"""
    rng = np.random.default_rng(99001)
    return {"small": ([text(rng, 300) for _ in range(3)], 512),
            "large": ([text(rng, 5000) for _ in range(40)], 7000),
            "wide": ([text(rng, 12) if d % 7 else b"" for d in range(1200)], 24)}


ORDER = ["small", "large", "small", "wide", "small"]


def new_batch(v):
    _, N, _ = _mods()
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, MAX_BYTES, MAX_DOCS, C.byref(b)))
    return b


def sync(b):
    _, N, _ = _mods()
    N.check(N.lib.tm_batch_totals(b, None, None))           # (everything here runs on the NULL stream, which this waits for)


def one_round(v, b, docs, L):
    """the round on batch b -> name -> array, every output of every call"""
    tm, N, _ = _mods()
    nd = len(docs)
    raw, offs = tm.pack_documents(docs)
    N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(offs), nd))
    N.check(N.lib.tm_batch_normalize(b, None))
    N.check(N.lib.tm_batch_run(b, None))
    n = C.c_uint64()
    N.check(N.lib.tm_batch_totals(b, C.byref(n), None))
    total = int(n.value)
    ids, toff = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(nd + 1, dtype=np.uint64)
    N.check(N.lib.tm_batch_download(b, N.ptr(ids), total, N.ptr(toff), None))
    got = {"ids": ids[:total], "toff": toff}
    pad, bos, eos = v.n_ids() + 5, v.n_ids() + 6, v.n_ids() + 7
    outs = []

    def keep(name, out, dtype):
        outs.append((name, out, dtype))

    # the ragged pairs: raw text in UTF-16 units, normalized text in code points (the unit index of both texts, both planes of one)
    for name, txt, unit in (("raw utf16", RAW, UTF16), ("norm chars", NORM, CODEPOINTS)):
        o = Out(2 * total, 4)
        N.check(N.lib.tm_batch_spans_in(b, None, txt, unit, o.ptr, total, None, None))
        keep(name, o, np.uint32)
    # one document per row
    how = Collate(0, nd, L, 4, pad, bos, eos, 0)
    o = Out(2 * nd * L, 4)
    N.check(N.lib.tm_batch_collate_spans_in(b, C.byref(how), None, RAW, CODEPOINTS, o.ptr, 4))
    keep("collate spans", o, np.uint32)
    # windows
    win = Collate(0, nd, WINDOW_LEN, 2, pad, bos, NONE, 0)
    need = C.c_uint64()
    N.check(N.lib.tm_batch_window_rows(b, C.byref(win), OVERLAP, C.byref(need)))
    rows = int(need.value)
    w = [Out(rows * WINDOW_LEN, 2), Out(rows * WINDOW_LEN, 1), Out(rows, 4), Out(rows, 4), Out(rows, 4)]
    N.check(N.lib.tm_batch_windows(b, C.byref(win), OVERLAP, None, rows, *[x.ptr for x in w]))
    for name, x, dt in zip(("window ids", "window mask", "window lengths", "window row_doc", "window row_start"), w, (np.uint16, np.uint8, np.uint32, np.uint32, np.uint32)):
        keep(name, x, dt)
    o = Out(2 * rows * WINDOW_LEN, 8)
    N.check(N.lib.tm_batch_windows_spans_in(b, C.byref(win), OVERLAP, None, rows, NORM, UTF16, o.ptr, 8))
    keep("window spans", o, np.uint64)
    # the collated rows, loaded back as the batch's ids, and their text
    rows_out, lens = Out(nd * L, 4), Out(nd, 4)
    N.check(N.lib.tm_batch_collate(b, C.byref(how), None, rows_out.ptr, None, lens.ptr))
    keep("rows", rows_out, np.uint32)
    sync(b)
    N.check(N.lib.tm_batch_load_ids(b, rows_out.ptr, nd, L, 4, lens.ptr, pad, bos, eos, None))
    nbytes, host_docs = C.c_uint64(), C.c_uint32()
    N.check(N.lib.tm_batch_decode(b, 0, None, C.byref(nbytes), C.byref(host_docs)))
    dec, doff = np.zeros(len(raw) * 2 + 64, dtype=np.uint8), np.zeros(nd + 1, dtype=np.uint64)
    N.check(N.lib.tm_batch_decoded_download(b, N.ptr(dec), dec.size, N.ptr(doff)))
    got["decoded"], got["decoded offsets"] = dec[:int(doff[nd])], doff
    sync(b)
    for name, o, dt in outs:
        assert o.sentinels_intact(), name
        got[name] = o.view(dt).copy()
    got["device_bytes"] = int(N.lib.tm_batch_device_bytes(b))
    return got


def same(a, e, what):
    assert sorted(a) == sorted(e)
    for k in a:
        if k != "device_bytes":
            assert a[k].shape == e[k].shape and (a[k] == e[k]).all(), (what, k)


def test_rounds_match_a_fresh_batch_and_the_buffers_only_grow():
    _, N, _ = _mods()
    v = make_vocab()
    R = rounds()
    fresh = {}
    for name, (docs, L) in R.items():
        f = new_batch(v)
        try:
            fresh[name] = one_round(v, f, docs, L)
        finally:
            N.lib.tm_batch_free(f)
    # the rounds hold what they were made for
    assert fresh["large"]["ids"].size + 4 > MAX_BYTES // 2 + 2 * MAX_DOCS + 1024 and 40 * 7000 > fresh["large"]["ids"].size * 5 // 4 + 1024
    assert not np.array_equal(fresh["large"]["raw utf16"], fresh["large"]["norm chars"])
    assert (fresh["large"]["decoded"].size > 150_000) and fresh["wide"]["window row_doc"].size >= 1200
    b = new_batch(v)
    try:
        sizes = [int(N.lib.tm_batch_device_bytes(b))]
        seen = set()
        for k, name in enumerate(ORDER):
            got = one_round(v, b, *R[name])
            same(got, fresh[name], "round %d (%s)" % (k, name))
            assert got["device_bytes"] >= sizes[-1], (k, name, sizes)
            if name in seen:
                assert got["device_bytes"] == sizes[-1], (k, name, sizes)          # grown for it already: nothing changes
            else:
                assert got["device_bytes"] > sizes[-1], (k, name, sizes)           # (each new shape is larger somewhere than everything before it)
                again = one_round(v, b, *R[name])                                   # ... and once grown, the same round again changes nothing
                same(again, fresh[name], "round %d (%s) again" % (k, name))
                assert again["device_bytes"] == got["device_bytes"], (k, name)
            seen.add(name)
            sizes.append(got["device_bytes"])
    finally:
        N.lib.tm_batch_free(b)
        v.close()


def repeated_round_child():
    """(run in a process of its own with TM_TRACE set: see test_a_repeated_round_replaces_no_buffer)"""
    _, N, _ = _mods()
    v = make_vocab()
    R = rounds()
    b = new_batch(v)
    for name in ("small", "large", "wide"):
        for mark in ("FIRST", "SECOND"):
            sys.stderr.write(mark + "\n")
            sys.stderr.flush()
            one_round(v, b, *R[name])
    N.lib.tm_batch_free(b)
    v.close()


def test_a_repeated_round_replaces_no_buffer():
    """TM_TRACE names every buffer that is replaced by a larger one ([grow]): the large round names some, no round names one the second time"""
    code = "import sys; sys.path.insert(0, 'tests'); import conftest; import test_gpu_batch_buffers as t; t.repeated_round_child()"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, TM_TRACE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    parts = err.split("SECOND\n")
    assert len(parts) == 4, err[-3000:]
    assert "[grow]" in parts[1], err[-3000:]          # (between the large round's first and second run)
    grows = [l for p in parts[1:] for l in p.split("FIRST\n")[0].splitlines() if "[grow]" in l]
    assert not grows, grows

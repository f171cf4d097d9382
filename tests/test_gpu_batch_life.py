"""-m gpu: ONE tm_batch through its whole life.  Every other -m gpu file builds a batch for one family of calls and feeds it one way; here one
handle takes every way ids or text arrive (A upload + run, B raw upload + normalize + run, N tm_batch_normalize alone on the raw text it still
holds, C tm_batch_load_ids, D the same after a scoring pass of the vocabulary, E no documents), document counts up and down, totals of other
magnitudes, texts of equal length and other characters - and after every arrival every call the header allows is held against the suite's own
references (np_collate, select, masked_range, np_pack, np_fit, np_windows, np_pairs, check_order, the span / owner / unit recipes, the region
rule, the oracle), every call it does not allow must return TM_E_INVALID and write nothing.  What goes wrong here is state the handle carries
from call to call: the unit index (units_forget), last_totals, the reserves by document count, out_cap, has_output / row_form, the last decode.

The vocabulary: every single byte plus ASCII words, capcode 0, NFD - text of NFD-stable characters is its own normalized form, so two texts
can have equal raw AND equal normalized lengths, and marks out of canonical order still send a document to the host normalizer.
A scoring pass keeps its text in a workspace of the tm_dataset: no call of the C ABI lends a caller's tm_batch to it, so D checks that a pass
beside the batch disturbs nothing of it.  The header does not say what tm_batch_decoded_download returns between a new arrival and the next
tm_batch_decode: not checked.  Twin: tests/test_batch_life_emulated.py."""
import ctypes as C

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N, synth
from conftest import EMULATED
from fixed_shape import Collate, Out, spec, DT, KEEP_TAIL, NONE, PAD_LEFT
import origin_recipe
import unit_recipe as UR
from oracle_bind import Oracle
from span_recipe import oracle_spans
from test_gpu_collate import np_collate, np_pack
from test_gpu_select import check_order, select, load, sync
from test_gpu_masked import masked_range, masking, ONE, SHARES
from test_gpu_fit import check as check_fit
from test_gpu_windows import np_windows
from test_gpu_pairs import Pair, np_pairs, LONGEST, ONLY_FIRST, ONLY_SECOND
from test_gpu_spans import download, np_collate_spans
from test_gpu_raw_spans import lib_origins
from test_gpu_char_offsets import spans_in, converted, B as BLOCK
from test_gpu_region_labels import reference as region_reference
from test_gpu_score_handle import Runtime

pytestmark = pytest.mark.gpu
PAD, BOS, EOS, SEP = 60001, 60002, 60003, 60005          # (no document holds them: ids stay below 60000)
NORM, RAW = 0, 1
T = 2048                                     # ORD_TILE of tm_order.hip
HOST_DOC = "Ab ạ́ cD é x".encode()          # two combining marks out of canonical order: the host normalizer's (test_gpu_char_offsets.MicroCase)
WORDS = [b" the", b"the", b" cat", b"at", b" a", b"he", b" on", b"mat", b"ab", b"abc", b" ab", b"cde", b"dea"]
IDS_ONLY = ["collate", "collate_select", "collate_masked", "pack", "fit", "windows", "pair", "order_ascending", "order_descending", "decode"]
WALKED = ["spans", "collate_spans", "region_labels"]
SEEN, FIRST = {}, set()                      # (arrival, checker) -> times exercised; (arrival, checker) that ran directly behind the arrival


# ---- the texts -------------------------------------------------------------------------------------------------------------------------------
def ascii_text(n):
    return (b"the cat on a mat abc de " * (n // 24 + 1))[:n]


def straddle_text(n):
    """n bytes (a multiple of 256, four blocks or more) of NFD-stable text: a 2-, a 3- and a 4-byte character across the first three boundaries
    of the index's blocks (the model: test_gpu_char_offsets.straddle_doc), others inside the blocks, ASCII elsewhere"""
    d = bytearray()
    for blk, ch in enumerate(("я", "あ", "😀"), 1):
        e = ch.encode()
        while len(d) + len(e) // 2 + (len(e) == 3) < blk * BLOCK:
            d += "я😀 あ".encode() if len(d) % 64 == 10 and len(d) + 40 < blk * BLOCK else b"abc de "[len(d) % 7:len(d) % 7 + 1]
        assert len(d) < blk * BLOCK < len(d) + len(e)
        d += e
    d += ascii_text(n - len(d))
    d.decode()                                           # (well formed)
    return bytes(d)


def halves(t, cut=300):
    assert t[cut] < 0x80 and t[cut - 1] < 0x80
    return [t[:cut], b"", t[cut:]]


# ---- what a batch should hold ----------------------------------------------------------------------------------------------------------------
class State:
    """the plain record: kind of arrival, the documents' expected ids, and - for ids that came from a walk - the normalized text with its byte
    pairs and, for text that arrived raw, the raw text with its byte pairs"""

    def __init__(self, kind, ids, norm=None, norm_spans=None, raw=None, raw_spans=None, host=0):
        self.kind, self.ids, self.norm, self.norm_spans, self.raw, self.raw_spans, self.host = kind, ids, norm, norm_spans, raw, raw_spans, host
        self.nd, self.counts = len(ids), [len(x) for x in ids]
        self.toff = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.total = int(self.toff[-1])

    def texts(self):
        """-> [(TM_TEXT_*, the documents, their byte pairs)] the batch can be asked about"""
        return ([(NORM, self.norm, self.norm_spans)] if self.norm is not None else []) + ([(RAW, self.raw, self.raw_spans)] if self.raw is not None else [])

    def allowed(self):
        return IDS_ONLY + (WALKED if self.norm is not None else [])


class Env:
    def __init__(self):
        toks = [bytes([i]) for i in range(256)] + WORDS
        self.img = synth.build_vocab(toks, capcode=0, charset=1, norm_flag=1, with_unk=True)
        self.v, self.orc = tm.Vocab(self.img), Oracle(self.img)
        self.n_ids = self.v.n_ids()
        assert self.n_ids < 60000
        self.memo = {}
        self.rt = Runtime()
        self.data = np.frombuffer(ascii_text(3000) + straddle_text(1024), dtype=np.uint8)          # the dataset of the scoring pass (D)
        self.ds = C.c_void_p()
        N.check(N.lib.tm_dataset_upload(N.ptr(self.data), self.data.size, C.byref(self.ds)))
        self.score = self.orc.score(self.data)
        self.batches = []

    def new_batch(self, max_bytes=1 << 14, max_docs=2 * T + 8):
        b = C.c_void_p()
        N.check(N.lib.tm_batch_create(self.v.handle, max_bytes, max_docs, C.byref(b)))
        self.batches.append(b)
        return b

    def doc(self, raw):
        """a raw document -> (ids, normalized text, its byte pairs, the raw pairs, whether the host normalizes it); computed once, never changed"""
        if raw not in self.memo:
            norm, host = synth.normalize(raw, 0, 1), raw == HOST_DOC
            nb, own = lib_origins(raw, 0, 1) if host else origin_recipe.normalize_with_owners(raw, 0, 1)
            assert nb == norm
            ids, _ = self.orc.tokenize(norm)
            sp = oracle_spans(self.orc, norm, True)
            rsp = origin_recipe.raw_spans(sp, own, len(raw))
            assert sp.shape[0] == ids.size
            for a in (ids, sp, rsp):
                a.setflags(write=False)
            self.memo[raw] = (ids, norm, sp, rsp, host)
        return self.memo[raw]

    def state(self, kind, docs, raw):
        r = [self.doc(d) for d in docs]
        return State(kind, [x[0] for x in r], [x[1] for x in r], [x[2] for x in r], list(docs) if raw else None, [x[3] for x in r] if raw else None,
                     sum(x[4] for x in r) if raw else 0)

    def close(self):
        for b in self.batches:
            N.lib.tm_batch_free(b)
        N.lib.tm_dataset_free(self.ds)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


# ---- calls that must be refused: TM_E_INVALID, nothing written ---------------------------------------------------------------------------------
def refused(b, calls, nd):
    """each of `calls` (name, TM_TEXT_*) on one document (none where the batch has none): TM_E_INVALID, and no output is touched"""
    outs = [Out(64, 8) for _ in range(4)]
    p, n = [o.ptr for o in outs], min(nd, 1)
    how, pr = Collate(0, n, 8, 4, PAD, NONE, NONE, 0), Pair(0, 0, n, 8, 4, PAD, NONE, NONE, NONE, 0, LONGEST, 0)
    need = C.c_uint64()
    L = N.lib
    table = {
        "collate": lambda t: L.tm_batch_collate(b, C.byref(how), None, p[0], None, None),
        "collate_select": lambda t: L.tm_batch_collate_select(b, C.byref(how), p[1], None, p[0], None, None, None),
        "collate_masked": lambda t: L.tm_batch_collate_masked(b, C.byref(how), C.byref(masking(1, ONE // 2, (1, 3), SHARES[0], 4)), None, None, p[0], p[1], None, None, None),
        "pack": lambda t: L.tm_batch_pack(b, C.byref(how), None, 8, p[0], None, None) if L.tm_batch_pack_rows(b, C.byref(how), C.byref(need)) == N.TM_E_INVALID else 12345,
        "fit": lambda t: L.tm_batch_fit(b, C.byref(how), None, 8, p[0], None, None, None, None, None) if L.tm_batch_fit_rows(b, C.byref(how), C.byref(need)) == N.TM_E_INVALID else 12345,
        "windows": lambda t: L.tm_batch_windows(b, C.byref(how), 1, None, 8, p[0], None, None, None, None) if L.tm_batch_window_rows(b, C.byref(how), 1, C.byref(need)) == N.TM_E_INVALID else 12345,
        "pair": lambda t: L.tm_batch_pair(b, C.byref(pr), None, p[0], None, None, None),
        "order": lambda t: L.tm_batch_length_order(b, 0, n, 0, None, p[0], p[1]),
        "spans": lambda t: L.tm_batch_spans_in(b, None, t, UR.CODEPOINTS, p[0], 32, None, None),
        "collate_spans": lambda t: L.tm_batch_collate_spans_in(b, C.byref(how), None, t, UR.UTF16, p[0], 4),
        "windows_spans": lambda t: L.tm_batch_windows_spans_in(b, C.byref(how), 1, None, 8, t, UR.BYTES, p[0], 8),
        "pair_spans": lambda t: L.tm_batch_pair_spans_in(b, C.byref(pr), None, t, UR.BYTES, p[0], 8),
        "region_labels": lambda t: L.tm_batch_region_labels(b, None, C.byref(N.Regions(p[2], p[3], t, 0, -100)), p[0], 4, 64, None, None, None),
        "collate_region_labels": lambda t: L.tm_batch_collate_region_labels(b, C.byref(how), None, C.byref(N.Regions(p[2], p[3], t, 0, -100)), p[0], 4, None),
    }
    for name, text in calls:
        assert table[name](text) == N.TM_E_INVALID, (name, text)
    assert all(o.untouched() for o in outs), calls


NEEDS_IDS = [(n, NORM) for n in ("collate", "collate_select", "collate_masked", "pack", "fit", "windows", "pair", "order", "spans")]
NEEDS_WALK = [(n, t) for n in ("spans", "collate_spans", "windows_spans", "pair_spans", "region_labels", "collate_region_labels") for t in (NORM, RAW)]
NEEDS_RAW = [(n, RAW) for n, t in NEEDS_WALK if t == RAW]


# ---- arrivals ---------------------------------------------------------------------------------------------------------------------------------
def arrive(env, b, how, docs=None, id_bytes=4, raw_state=None):
    """one arrival -> the State the batch should be in.  how: A, B, N (raw_state: what the raw text it still holds gives), C (docs: id counts),
    D, E (tm_batch_load_ids of no rows), Eu (an upload of no documents and its run)"""
    L = N.lib
    if how == "D":
        s, t, m = np.full(env.n_ids, 0xA5A5A5A5, dtype=np.uint32), C.c_uint64(77), np.full(32, 0xA5, dtype=np.uint8)
        N.check(L.tm_score(env.v.handle, env.ds, None, None, 0, N.ptr(s), C.byref(t), N.ptr(m)))
        assert (s == env.score[0]).all() and t.value == env.score[1] and (m == env.score[2]).all()
    if how in ("A", "D", "Eu"):
        st = env.state(how, docs or [], False)
        text, offs = tm.pack_documents(st.norm)
        N.check(L.tm_batch_upload(b, N.ptr(text), N.ptr(offs), st.nd))
        refused(b, NEEDS_IDS, st.nd)
        N.check(L.tm_batch_run(b, None))
        refused(b, NEEDS_RAW, st.nd)
    elif how == "B":
        st = env.state(how, docs, True)
        raw, offs = tm.pack_documents(docs)
        N.check(L.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(offs), st.nd))
        refused(b, NEEDS_IDS, st.nd)
        N.check(L.tm_batch_normalize(b, None))
        refused(b, NEEDS_IDS, st.nd)
        N.check(L.tm_batch_run(b, None))
        assert int(L.tm_batch_host_fallback_docs(b)) == st.host
    elif how == "N":
        st = State("N", raw_state.ids, raw_state.norm, raw_state.norm_spans, raw_state.raw, raw_state.raw_spans, raw_state.host)
        N.check(L.tm_batch_normalize(b, None))
        refused(b, NEEDS_IDS, st.nd)
        N.check(L.tm_batch_run(b, None))
    elif how == "C":
        st = State("C", load(b, docs, id_bytes))
        refused(b, NEEDS_WALK, st.nd)
    else:
        assert how == "E"
        st = State("E", [])
        N.check(L.tm_batch_load_ids(b, None, 0, 0, 4, None, NONE, NONE, NONE, None))
        refused(b, NEEDS_WALK, st.nd)
    ids, toff, miss, total, missing = download(b, st.nd)
    assert total == st.total and missing == 0 and (toff.astype(np.int64) == st.toff).all() and not miss.any(), (how, total, st.total)
    assert (ids == np.concatenate(list(st.ids) + [np.zeros(0, np.uint32)])).all(), how
    return st


# ---- checkers: one call each into page-locked outputs behind sentinels, compared exactly ------------------------------------------------------
def shape(st, k):
    """-> (first_doc, ndocs, L, id_bytes, bos, eos, flags, shift) of step k: a part of the run where it has three documents or more"""
    first = 1 if st.nd >= 3 and k & 1 else 0
    return (first, st.nd - first - (1 if st.nd >= 3 and k & 2 else 0), [1, 7, 9, 33, 64][k % 5] + 2, [2, 4, 8][k % 3], BOS if k & 1 else None, EOS if k & 2 else None,
            [0, PAD_LEFT, KEEP_TAIL, PAD_LEFT | KEEP_TAIL][(k // 2) % 4], k & 1)


def compare(outs, exps, what, written=True):
    for x, e in zip(outs, exps):
        assert x.sentinels_intact() and (x.view(DT[x.elem] if x.elem > 1 else np.uint8) == np.asarray(e).reshape(-1)).all() if written else x.untouched(), what


def c_collate(env, b, st, k):
    first, n, L, id_bytes, bos, eos, flags, shift = shape(st, k)
    o = [Out(n * L, id_bytes, shift), Out(n * L, 1, shift), Out(n, 4)]
    N.check(N.lib.tm_batch_collate(b, C.byref(Collate(first, n, L, id_bytes, PAD, spec(bos), spec(eos), flags)), None, *[x.ptr for x in o]))
    sync(b)
    compare(o, np_collate(st.ids[first:first + n], L, PAD, bos, eos, flags, DT[id_bytes]), ("collate", st.kind, k), n > 0)


def c_collate_select(env, b, st, k):
    _, _, L, id_bytes, bos, eos, flags, shift = shape(st, k)
    sel = (list(range(st.nd))[::-1] + [0, st.nd + 3, st.nd // 2])[:600] if st.nd else []
    select(b, st.ids, sel, L, id_bytes, bos, eos, flags, shift, (True, True, st.nd > 0))


def masked(b, docs, m, L, id_bytes, bos, eos, flags, first=0, n=None, sel=None, shift=0, stream=None, wait=None):
    """tm_batch_collate_masked against the rule (test_gpu_masked.run with a first_doc and a stream): the counters are the ABSOLUTE places of
    the ids in the run's buffer -> (ids, labels) as [rows, L] arrays"""
    dt, ign = DT[id_bytes], m.label_ignore % (1 << (8 * id_bytes))
    n = len(docs) - first if n is None else n
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    rows_of = list(range(first, first + n)) if sel is None else list(sel)
    done = {i: masked_range(docs[i], int(off[i]), m) for i in set(rows_of) if i < len(docs)}
    isbad = np.array([i >= len(docs) for i in rows_of], dtype=bool)
    e = list(np_collate([done[i][0] if i in done else [] for i in rows_of], L, PAD, bos, eos, flags, dt))
    lab = np_collate([[int(t) if s else ign for t, s in zip(docs[i], done[i][1])] if i in done else [] for i in rows_of], L, ign, None if bos is None else ign,
                     None if eos is None else ign, flags, dt)[0]
    if isbad.any():
        e[0][isbad], e[1][isbad], e[2][isbad], lab[isbad] = PAD, 0, 0, ign
    rows = len(rows_of)
    o, idx = [Out(rows * L, id_bytes, shift), Out(rows * L, id_bytes, shift), Out(rows * L, 1, shift), Out(rows, 4), Out(1, 4)], Out(rows, 4)
    idx.view(np.uint32)[:] = rows_of
    how = Collate(first if sel is None else 0, rows, L, id_bytes, PAD, spec(bos), spec(eos), flags)
    N.check(N.lib.tm_batch_collate_masked(b, C.byref(how), C.byref(m), None if sel is None else idx.ptr, stream, *[x.ptr for x in o[:4]], o[4].ptr if rows else None))
    wait() if wait else sync(b)
    compare(o[:4], [e[0], lab, e[1], e[2]], ("masked", L, id_bytes, first, n, sel is not None), rows > 0)
    assert (o[4].sentinels_intact() and int(o[4].view(np.uint32)[0]) == isbad.sum()) if rows else o[4].untouched()
    return o[0].view(dt).reshape(rows, L).copy(), o[1].view(dt).reshape(rows, L).copy()


def c_collate_masked(env, b, st, k):
    first, n, L, id_bytes, bos, eos, flags, shift = shape(st, k)
    m = masking(500 + k, ONE // 5, [(1, 1), (1, 32), (3, 3)][k % 3], SHARES[k % 3], id_bytes)
    sel = list(range(st.nd))[::-1][:300] + [st.nd + 1] if (k // 3) & 1 and st.nd else None
    masked(b, st.ids, m, L, id_bytes, bos, eos, flags, first, n, sel, shift)


def c_pack(env, b, st, k):
    first, n, L, id_bytes, _, eos, _, shift = shape(st, k)
    e = np_pack(st.ids[first:first + n], L, PAD, eos, DT[id_bytes])
    rows, need, how = e[0].shape[0], C.c_uint64(12345), Collate(first, n, L, id_bytes, PAD, NONE, spec(eos), 0)
    N.check(N.lib.tm_batch_pack_rows(b, C.byref(how), C.byref(need)))
    assert need.value == rows, ("pack", st.kind, k)
    o = [Out(rows * L, id_bytes, shift), Out(rows * L, 4, shift), Out(rows * L, 4)]
    N.check(N.lib.tm_batch_pack(b, C.byref(how), None, rows, *[x.ptr for x in o]))
    sync(b)
    compare(o, e[:3], ("pack", st.kind, k), rows > 0)


def c_fit(env, b, st, k):
    first, n, L, id_bytes, _, eos, _, shift = shape(st, k)
    check_fit(b, st.ids, first, n, L, id_bytes, 60002 if eos else None, shift)          # (its own PAD and EOS)


def c_windows(env, b, st, k):
    first, n, L, id_bytes, bos, eos, flags, shift = shape(st, k)
    overlap, left = (L - (bos is not None) - (eos is not None) - 1) // 2, bool(flags & PAD_LEFT)
    e = np_windows(st.ids[first:first + n], L, PAD, bos, eos, overlap, left)
    rows, need, how = e[0].shape[0], C.c_uint64(12345), Collate(first, n, L, id_bytes, PAD, spec(bos), spec(eos), PAD_LEFT if left else 0)
    N.check(N.lib.tm_batch_window_rows(b, C.byref(how), overlap, C.byref(need)))
    assert need.value == rows and rows >= n, ("windows", st.kind, k)
    o = [Out(rows * L, id_bytes, shift), Out(rows * L, 1, shift), Out(rows, 4), Out(rows, 4), Out(rows, 4)]
    N.check(N.lib.tm_batch_windows(b, C.byref(how), overlap, None, rows, *[x.ptr for x in o]))
    sync(b)
    compare(o, e[:5], ("windows", st.kind, k), rows > 0)


def c_pair(env, b, st, k):
    _, _, L, id_bytes, bos, eos, flags, shift = shape(st, k)
    n, nsep = (st.nd + 1) // 2, k % 3
    fa, fb = (0, st.nd - n) if k & 1 else (st.nd - n, 0)
    L, left, trunc = L + nsep, bool(flags & PAD_LEFT), (LONGEST, ONLY_FIRST, ONLY_SECOND)[(k // 3) % 3]
    e = np_pairs(st.ids[fa:fa + n], st.ids[fb:fb + n], L, PAD, bos, SEP if nsep else None, nsep, eos, trunc, left)
    how = Pair(fa, fb, n, L, id_bytes, PAD, spec(bos), SEP if nsep else NONE, spec(eos), nsep, trunc, PAD_LEFT if left else 0)
    o = [Out(n * L, id_bytes, shift), Out(n * L, 1, shift), Out(n * L, 1), Out(2 * n, 4)]
    N.check(N.lib.tm_batch_pair(b, C.byref(how), None, *[x.ptr for x in o]))
    sync(b)
    compare(o, [e.ids, e.mask, e.types, e.kept], ("pair", st.kind, k), n > 0)


def c_order(desc):
    def f(env, b, st, k):
        first, n = shape(st, k)[:2]
        check_order(b, st.counts, first, n, desc, with_counts=bool(k & 4) or n == 0)
    return f


def c_spans(env, b, st, k):
    """the ragged pairs of every text the batch holds in bytes, code points and UTF-16 units: UTF-16 in front of code points on even steps (both
    planes of the index at once, then nothing to make), behind them on odd ones (the second plane by itself)"""
    units = [UR.BYTES, UR.UTF16, UR.CODEPOINTS] if k % 2 == 0 else [UR.CODEPOINTS, UR.BYTES, UR.UTF16]
    for text, docs, sp in st.texts()[::-1 if k & 2 else 1]:
        for unit in units:
            got, hd = spans_in(b, text, unit, st.total)
            exp = converted(sp, docs, unit)
            assert got.shape == exp.shape and (got == exp).all(), ("spans", st.kind, k, text, unit, np.nonzero((got != exp).any(axis=1))[0][:4])
            assert (hd >= 1) == (text == RAW and st.host > 0), (hd, st.host)


def c_collate_spans(env, b, st, k):
    first, n, L, _, bos, eos, flags, shift = shape(st, k)
    text, docs, sp = st.texts()[k % len(st.texts())]
    unit, span_bytes = [UR.CODEPOINTS, UR.UTF16, UR.BYTES][(k // 2) % 3], (4, 8)[(k // 3) & 1]
    out, dt = Out(n * L * 2, span_bytes, shift), DT[span_bytes]
    N.check(N.lib.tm_batch_collate_spans_in(b, C.byref(Collate(first, n, L, 4, PAD, spec(bos), spec(eos), flags)), None, text, unit, out.ptr, span_bytes))
    sync(b)
    per = [UR.convert(s, d, unit) for s, d in zip(sp[first:first + n], docs[first:first + n])]
    compare([out], [np_collate_spans(per, L, bos, eos, flags, dt)], ("collate_spans", st.kind, k, text, unit), n > 0)


def c_region_labels(env, b, st, k):
    """two regions per document - one over its first units, one from the middle beyond its end - under the rule of test_gpu_region_labels"""
    text, docs, sp = st.texts()[k % len(st.texts())]
    unit, nbytes, ignore = [UR.UTF16, UR.BYTES, UR.CODEPOINTS][(k // 2) % 3], (4, 8)[k & 1], (-100, 0xFFFFFF)[(k // 2) & 1]
    lens = [int(UR.U_table(d, unit)[-1]) for d in docs]
    regs = np.array([r for d, n in enumerate(lens) for r in ((0, 2, d % 7 - 3), (max(2, n // 2 + 1), n + 9, 5 + d % 3))], np.int64).reshape(-1, 3)
    roff = np.arange(st.nd + 1, dtype=np.uint64) * 2
    pairs = converted(sp, docs, unit)
    exp, exp_rtok = region_reference(pairs, st.toff, regs, roff, lens, ignore)
    pin = [Out(roff.size, 8), Out(max(regs.size, 1), 4)]
    pin[0].view(np.uint64)[:] = roff
    pin[1].view(np.uint32)[:regs.size] = regs.astype(np.uint32).reshape(-1)
    rg = N.Regions(pin[0].ptr, pin[1].ptr, text, unit, ignore)
    out, rt, bad = Out(st.total, nbytes, k & 1), Out(2 * regs.shape[0], 4), Out(1, 4)
    N.check(N.lib.tm_batch_region_labels(b, None, C.byref(rg), out.ptr, nbytes, st.total, rt.ptr if st.nd else None, bad.ptr if st.nd else None, None))
    sync(b)
    if st.nd == 0:
        return compare([out, rt, bad], [[], [], []], ("region_labels", st.kind, k), False)
    assert out.sentinels_intact() and rt.sentinels_intact() and bad.sentinels_intact() and int(bad.view(np.uint32)[0]) == 0
    assert (out.view({4: np.int32, 8: np.int64}[nbytes]).astype(np.int64) == exp).all() and (rt.view(np.uint32).reshape(-1, 2) == exp_rtok).all(), ("region_labels", st.kind, k, text, unit)


def c_decode(env, b, st, k):
    """tm_batch_decode and its download: the oracle's bytes of the ids the vocabulary has (the decoder skips the others); no capcode, so both forms agree"""
    exp = [env.orc.decode_raw(np.asarray(d)[np.asarray(d) < env.n_ids]) for d in st.ids]
    nbytes, hd = C.c_uint64(123), C.c_uint32(123)
    N.check(N.lib.tm_batch_decode(b, k & 1, None, C.byref(nbytes), C.byref(hd)))
    size = sum(len(x) for x in exp)
    out, ooff = np.full(size + 64, 0xA5, dtype=np.uint8), np.full(st.nd + 1, 0xA5A5A5A5, dtype=np.uint64)
    N.check(N.lib.tm_batch_decoded_download(b, N.ptr(out), size, N.ptr(ooff)))
    assert nbytes.value == size and hd.value == 0 and (ooff == np.concatenate([[0], np.cumsum([len(x) for x in exp])])).all(), ("decode", st.kind, k)
    assert bytes(out[:size]) == b"".join(exp) and (out[size:] == 0xA5).all(), ("decode", st.kind, k)


CHECKERS = {"collate": c_collate, "collate_select": c_collate_select, "collate_masked": c_collate_masked, "pack": c_pack, "fit": c_fit, "windows": c_windows, "pair": c_pair,
            "order_ascending": c_order(False), "order_descending": c_order(True), "spans": c_spans, "collate_spans": c_collate_spans, "region_labels": c_region_labels,
            "decode": c_decode}
assert sorted(CHECKERS) == sorted(IDS_ONLY + WALKED)


def check_all(env, b, st, k, only=None):
    """every checker the state allows, beginning with the k-th"""
    names = list(CHECKERS)
    names = [n for n in names[k % len(names):] + names[:k % len(names)] if n in st.allowed() and (only is None or n in only)]
    for j, name in enumerate(names):
        CHECKERS[name](env, b, st, k + j)
        SEEN[(st.kind, name)] = SEEN.get((st.kind, name), 0) + 1
        if j == 0:
            FIRST.add((st.kind, name))


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------------
def tiny(seed):
    return np.random.default_rng(seed).integers(0, 4, size=2 * T + 1).tolist()


MIXED = ["the cat あ on 😀😀 я mat".encode(), b"", "я".encode() * 150 + b" abc " + "😀".encode() * 70, b"abc the cat"]
SCHEDULE = [
    # documents up and down: the sort from one tile to three, win_cap / fit_cap / order_cap grown, large while few are used, used in full again
    ("A", [b"the cat on a mat", b"", "я abc".encode()]), ("C", tiny(1), 2), ("B", [b"abc the", HOST_DOC, b"", "あ cat 😀".encode(), b"de abc " * 9]), ("C", tiny(2), 8),
    # equal length, other characters, once for every way text arrives: the block-count guard of unit_index_on cannot see a stale index
    ("A", halves(ascii_text(1024))), ("A", halves(straddle_text(1024))),
    ("B", halves(ascii_text(1024))), ("B", halves(straddle_text(1024))),
    ("A", halves(ascii_text(1024))), ("N",),
    ("D", halves(ascii_text(1024))), ("D", halves(straddle_text(1024))),
    # the planes of the index one by one and both at once (c_spans: the order of the units turns with the step)
    ("A", MIXED), ("B", MIXED),
    # totals of another magnitude: the radix passes of the length order follow the ids that are there; the load outgrows out_cap
    ("A", [b"the cat", b"", b"ab"]), ("C", [3, 70000, 0, 65536, 2, 300], 2), ("A", [b"abc", b"the cat on"]),
    # no documents between documents
    ("E",), ("B", [HOST_DOC, b"the mat"]), ("Eu", []), ("C", [5, 0, 9], 4),
]
BIG = 15                                     # (the step of 70 000 ids: not on the emulated device)


def run_schedule(env, order):
    b = env.new_batch()
    raw_state = None
    for k, i in enumerate(order):
        step = SCHEDULE[i]
        if i == BIG and EMULATED:
            continue
        how = step[0]
        if how == "N" and raw_state is None:
            how, step = "B", ("B", halves(straddle_text(1024)))              # (a shuffle that begins with it: no raw text yet)
        st = arrive(env, b, how, step[1] if len(step) > 1 else None, step[2] if len(step) > 2 else 4, raw_state)
        if how in ("B", "N"):
            raw_state = st
        check_all(env, b, st, k)
    N.lib.tm_batch_free(b)
    env.batches.remove(b)


_base_done = False


def base_schedule(env):
    global _base_done
    if not _base_done:
        run_schedule(env, list(range(len(SCHEDULE))))
        _base_done = True


def test_the_texts_are_what_the_schedule_needs(env):
    a, s = ascii_text(1024), straddle_text(1024)
    assert len(a) == len(s) == 4 * BLOCK and max(a) < 0x80 and synth.normalize(s, 0, 1) == s and synth.normalize(a, 0, 1) == a
    for blk, size in ((1, 2), (2, 3), (3, 4)):           # a character of every length lies across a block boundary
        starts = UR.char_start_table(s)
        assert starts[blk * BLOCK] < blk * BLOCK and len(s[starts[blk * BLOCK]:].decode()[0].encode()) == size
    for unit in (UR.CODEPOINTS, UR.UTF16):               # block by block the counts differ from the ASCII text's: a stale index shows
        assert all(UR.U_table(s, unit)[j * BLOCK] != UR.U_table(a, unit)[j * BLOCK] for j in (1, 2, 3))
    assert UR.U_table(s, UR.UTF16)[-1] != UR.U_table(s, UR.CODEPOINTS)[-1]
    assert env.doc(HOST_DOC)[4] and synth.normalize(HOST_DOC, 0, 1) != HOST_DOC
    assert sum(len(env.doc(d)[0]) for d in SCHEDULE[14][1]) < 256 and sum(len(env.doc(d)[0]) for d in SCHEDULE[16][1]) < 256      # one radix pass
    assert SCHEDULE[BIG][0] == "C" and max(SCHEDULE[BIG][1]) == 70000 and 70000 * len(SCHEDULE[BIG][1]) > (1 << 14) // 2 + 2 * (2 * T + 8) + 1024      # beyond out_cap


def test_schedule_in_order(env):
    base_schedule(env)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_schedule_shuffled(env, seed):
    run_schedule(env, np.random.default_rng(seed).permutation(len(SCHEDULE)).tolist())


@pytest.mark.parametrize("how", ["A", "B", "N", "C", "D", "E", "Eu"])
def test_every_checker_first_behind_every_arrival(env, how):
    """the arrival again for every checker, and that checker alone behind it"""
    b = env.new_batch(1 << 12, 16)
    docs = {"C": [3, 0, 40, 1, 9], "E": None, "Eu": []}.get(how, ["the cat あ".encode(), b"", "я😀 abc de".encode() * 9, HOST_DOC if how in "BN" else b"ab"])
    raw_state = arrive(env, b, "B", [b"abc", "😀 the".encode()]) if how == "N" else None
    for k, name in enumerate(CHECKERS):
        st = arrive(env, b, how, docs, 2, raw_state)
        if name in st.allowed():
            check_all(env, b, st, k, only=[name])
            assert (st.kind, name) in FIRST


# ---- the masked call's open ends --------------------------------------------------------------------------------------------------------------
def test_masked_rows_of_a_part_of_the_run_count_from_the_run(env):
    """no list, first_doc 2, ndocs = run - 3: the counters are off[first_doc + r] + ..., not counted from first_doc"""
    b = env.new_batch(1 << 12, 16)
    counts, L = [5, 7, 0, 1, 40, 300, 9], 32
    docs, off = load(b, counts, 4), np.concatenate([[0], np.cumsum(counts)])
    m = masking(21, ONE // 20, (1, 32), SHARES[2], 4)
    absolute = [masked_range(docs[i], int(off[i]), m) for i in range(2, 6)]
    relative = [masked_range(docs[i], int(off[i] - off[2]), m) for i in range(2, 6)]
    assert any((x[1][-L:] != y[1][-L:]).any() for x, y in zip(absolute, relative))          # a rule keyed from first_doc selects other ids of these rows
    cut = [masked_range(docs[i][-L:], int(off[i + 1]) - L, m)[1] for i in (4, 5)]          # ... as if a document began where its row does
    assert any((c != masked_range(docs[i], int(off[i]), m)[1][-L:]).any() for c, i in zip(cut, (4, 5)))      # a span enters a row from ids it cut off
    ids, lab = masked(b, docs, m, L, 4, None, None, KEEP_TAIL, first=2, n=len(counts) - 3)
    assert ids.shape == (4, L) and (lab != 2 ** 32 - 100).any() and (lab[3] == 2 ** 32 - 100).any()


def test_masked_rows_of_a_real_run(env):
    b = env.new_batch(1 << 13, 16)
    st = arrive(env, b, "A", [b"the cat on a mat abc de " * 20, b"", "я😀 the".encode(), ascii_text(700)])
    for k, (first, sel) in enumerate(((0, None), (1, None), (0, [3, 0, 9, 3]))):
        _, lab = masked(b, st.ids, masking(30 + k, ONE // 6, (1, 32), SHARES[2], 4), 64, 4, BOS, EOS, KEEP_TAIL if k else 0, first, None, sel, k & 1)
        assert (lab != 2 ** 32 - 100).any()


def test_masked_rows_on_a_stream_of_the_caller(env):
    b, s = env.new_batch(1 << 12, 16), env.rt.stream()
    try:
        docs = load(b, [5, 0, 130, 1, 64], 2)
        masked(b, docs, masking(40, ONE // 4, (1, 32), SHARES[2], 2), 65, 2, BOS, None, PAD_LEFT, first=1, n=4, shift=1, stream=s, wait=lambda: env.rt.sync(s))
    finally:
        env.rt.sync(s)
        env.rt.destroy(s)


# ---- the table --------------------------------------------------------------------------------------------------------------------------------
def test_no_allowed_pair_of_arrival_and_checker_is_missing(env):
    base_schedule(env)
    allowed = {k: IDS_ONLY + WALKED for k in ("A", "B", "N", "D", "Eu")}
    allowed.update({k: IDS_ONLY for k in ("C", "E")})
    missing = [(k, n) for k, names in allowed.items() for n in names if not SEEN.get((k, n))]
    assert not missing, missing
    assert {n for _, n in FIRST} == set(CHECKERS), sorted(set(CHECKERS) - {n for _, n in FIRST})

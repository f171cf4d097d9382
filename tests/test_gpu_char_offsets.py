"""-m gpu: character offsets - tm_batch_spans_in, tm_batch_collate_spans_in, tm_batch_windows_spans_in, tm_tokenize_batch_spans_in (the unit index
k_unit_index and the conversion k_unit_spans in tokenmonster_amd/csrc/tm_units.hip) and torch_api's offset_unit.

Expected values: the oracle's walk (tests/span_recipe.py), mapped through the owners for raw text (tests/origin_recipe.py), converted by the rule of
include/tokenmonster_hip.h in numpy (tests/unit_recipe.py).  Only the scan-form test, whose text is too long for the oracle's walk in Python, takes the
existing byte-span call's output and converts that.  tests/test_char_offsets_emulated.py runs this file (less the torch cases) on the emulated device."""
import ctypes as C
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

import test_gpu_spans as S
import test_gpu_raw_spans as R
import unit_recipe as UR
from test_gpu_spans import Collate, Out, download, hooks, new_batch, np_collate_spans, KEEP_TAIL, PAD_LEFT

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

B = 256                                           # bytes of text per index entry (UNIT_BLOCK, tm_units.hip)
NORM, RAW = 0, 1                                  # TM_TEXT_*
UNITS = {"chars": UR.CODEPOINTS, "utf16": UR.UTF16}
KINDS = [(NORM, "chars"), (NORM, "utf16"), (RAW, "chars"), (RAW, "utf16")]
HOOKS = {"plain": 0, "packed_text": 2048, "per_lane_normalizer": 256}
ALPHABET = ["é", "Ω", "я", "ế", "あ", "が", "한", "😀", " ", "a", "b", "c", "d", "e", "H", "i", ".", "\n", "S", "h", " the", " cat"]


def _mods():
    return S._mods()


def spans_in(b, text, unit, total, ms=None):
    """tm_batch_spans_in on the NULL stream into page-locked memory -> (int64 [total, 2], documents mapped on the host)"""
    _, N, _ = _mods()
    out = Out(2 * total, 4)
    hd = C.c_uint32(777)
    N.check(N.lib.tm_batch_spans_in(b, None, text, unit, out.ptr, total, C.byref(hd), ms))
    N.check(N.lib.tm_batch_totals(b, None, None))
    assert out.sentinels_intact()
    return out.view(np.uint32).reshape(total, 2).astype(np.int64), int(hd.value)


def converted(spans, texts, unit):
    """the byte pairs of every document (a list of [n, 2]) over its text -> one int64 [total, 2] in `unit`"""
    return np.concatenate([UR.convert(sp, t, unit) for sp, t in zip(spans, texts)] + [np.zeros((0, 2), np.int64)])


def first_difference(got, exp, toff):
    k = int(np.argwhere((got != exp).any(axis=1))[0, 0])
    d = int(np.searchsorted(toff, k, side="right")) - 1
    return "document %d, id %d of it: %s, the recipe says %s" % (d, k - int(toff[d]), got[k].tolist(), exp[k].tolist())


def mixed_text(rng, nbytes):
    """a str of the alphabet whose UTF-8 form has exactly nbytes bytes"""
    out, n = [], 0
    while n < nbytes:
        ch = ALPHABET[int(rng.integers(0, len(ALPHABET)))]
        if n + len(ch.encode()) > nbytes:
            ch = "a"
        out.append(ch)
        n += len(ch.encode())
    s = "".join(out)
    assert len(s.encode()) == nbytes
    return s


# ---- the all-single-bytes vocabulary: every character outside ASCII splits into one id per byte -----------------------------------------------------
class SplitCase:
    """Vocab.from_tokens(capcode 0, no flags): every single byte plus ASCII words.  Raw text is the identity map here; the expected byte pairs are the
    oracle's walk over the document, the same for both kinds of text."""

    def __init__(self):
        from oracle_bind import Oracle
        tm, _, _ = _mods()
        words = [b" the", b"the", b" cat", b"at", b" a", b"he", b" on", b"mat", b"ab", b"abc", b" ab", b"cde", b"dea"]
        assert all(max(w) < 0x80 for w in words)
        self.v = tm.Vocab.from_tokens([bytes([i]) for i in range(256)] + words, capcode=0, charset=1, norm_flag=0, with_unk=True)
        self.orc = Oracle(self.v.image())
        self.b = new_batch(self.v, 1 << 17, 256)
        self.memo = {}

    def oracle(self, doc):
        from span_recipe import oracle_spans
        if doc not in self.memo:
            ids, _ = self.orc.tokenize(doc)
            sp = oracle_spans(self.orc, doc, True)
            assert sp.shape[0] == ids.size
            sp.setflags(write=False)
            self.memo[doc] = (ids, sp)
        return self.memo[doc]

    def run(self, docs, text):
        if text == RAW:
            R.run_raw(self.b, docs)
        else:
            S.run_docs(self.b, docs)
        ids, toff, _, total, _ = download(self.b, len(docs))
        e_ids = np.concatenate([self.oracle(d)[0] for d in docs] + [np.zeros(0, np.uint32)])
        assert ids.size == e_ids.size and (ids == e_ids).all()
        return toff, total

    def check(self, docs, what):
        """the documents as one batch, both kinds of text and both units against the oracle's pairs converted by the recipe"""
        sp = [self.oracle(d)[1] for d in docs]
        for text in (NORM, RAW):
            toff, total = self.run(docs, text)
            for name, unit in UNITS.items():
                got, hd = spans_in(self.b, text, unit, total)
                exp = converted(sp, docs, unit)
                assert hd == 0 and got.shape == exp.shape
                assert (got == exp).all(), "%s, text %d, %s: %s" % (what, text, name, first_difference(got, exp, toff))
        return sp


_split = None


def split_case():
    global _split
    if _split is None:
        _split = SplitCase()
    return _split


def test_split_characters_begin_and_end_inside_a_character():
    c = split_case()
    docs = ["the cat é on Ω я, 한 mat あが 😀 ab😀é".encode(), "é".encode(), "😀".encode(), b"", "한한 the 😀😀".encode(), b"abc the cat"]
    sps = c.check(docs, "split characters")
    seen_begin, seen_end = set(), set()
    for doc, sp in zip(docs, sps):
        start = UR.char_start_table(doc)
        size = {}                                                     # byte offset of a character's begin -> its length
        bounds = [x for x in range(len(doc) + 1) if start[x] == x]
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            size[lo] = hi - lo
        for b_, e_ in sp.tolist():
            if e_ > b_ and start[b_] != b_:
                seen_begin.add(size[int(start[b_])])
            if e_ > b_ and start[e_] != e_:
                seen_end.add(size[int(start[e_])])
    assert seen_begin >= {2, 3, 4} and seen_end >= {2, 3, 4}, (seen_begin, seen_end)
    # an end inside a character rounds outward, its begin down: both bytes of "é" are the one character [0, 1)
    assert UR.convert(c.oracle("é".encode())[1], "é".encode(), UR.CODEPOINTS).tolist() == [[0, 1], [0, 1]]
    assert UR.convert(c.oracle("😀".encode())[1], "😀".encode(), UR.UTF16).tolist() == [[0, 2]] * 4


# ---- index edges ----------------------------------------------------------------------------------------------------------------------------------------
def straddle_doc():
    """a 2-, a 3- and a 4-byte character across a boundary of the index's blocks, at each possible split (the document opens the batch: its offsets
    are the buffer's)"""
    d = bytearray()
    for ch in ("é", "한", "😀"):
        e = ch.encode()
        for k in range(1, len(e)):
            while (len(d) + k) % B:
                d += b"abc de "[len(d) % 7:len(d) % 7 + 1]
            assert (len(d) + k) % B == 0
            d += e
    return bytes(d)


def test_index_edges():
    c = split_case()
    rng = np.random.default_rng(9901)
    lens = [B - 1, B, B + 1, 2 * B, 1023, 1024, 1025]
    docs = [straddle_doc()] + [mixed_text(rng, n).encode() for n in lens]
    docs += [b"", b"", mixed_text(rng, 300).encode(), b""]
    c.check(docs, "block edges")
    for d in docs[1:1 + len(lens)]:
        assert len(d) in lens
    # a document begins at every residue mod 16 of the buffer, empty documents between others
    docs = []
    for k in range(20):
        docs.append(mixed_text(rng, 17).encode())
        if k % 5 == 0:
            docs.append(b"")
    begins = np.cumsum([0] + [len(d) for d in docs])[:-1]
    assert {int(x) % 16 for x, d in zip(begins, docs) if d} == set(range(16))
    c.check(docs, "begins at every residue")
    # only continuation bytes: nothing to round down to, no unit to count
    docs = [b"ab", b"\x80" * 5, b"\x80" * 300, b"\x80", "é".encode()]
    sps = c.check(docs, "continuation bytes only")
    toff, total = c.run(docs, NORM)
    got, _ = spans_in(c.b, NORM, UR.CODEPOINTS, total)
    lo, hi = int(toff[1]), int(toff[3])
    assert hi - lo == 305 and not got[lo:hi].any() and len(sps[2]) == 300


# ---- the capcode-2, NFD + lowercase micro vocabulary -------------------------------------------------------------------------------------------------
class MicroCase:
    def __init__(self):
        _, _, synth = _mods()
        rng = np.random.default_rng(9902)
        img = synth.build_vocab(R.micro_tokens(rng, 2), capcode=2, charset=1, norm_flag=3, with_unk=True)
        self.strs = [mixed_text(rng, n) for n in R.RAW_LENS] + ["Ab ạ́ cD é x"]      # (the last: two marks out of canonical order, the host's)
        docs = [s.encode() for s in self.strs]
        self.host = len(docs) - 1
        self.c = R.RawCase(img, docs, host={self.host})
        self.docs = docs
        self.norm = [synth.normalize(d, 2, 3) for d in docs]
        self.which = list(range(len(docs)))

    def expected(self, text, unit):
        if text == RAW:
            return converted(self.c.raw_spans, self.docs, unit)
        return converted(self.c.norm_spans, self.norm, unit)


_micro = None


def micro():
    global _micro
    if _micro is None:
        _micro = MicroCase()
    return _micro


@pytest.mark.parametrize("hook", list(HOOKS))
def test_micro_vocabulary_both_texts_both_units(hook):
    _, N, _ = _mods()
    m = micro()
    assert [len(d) for d in m.docs[:-1]] == R.RAW_LENS
    with hooks(HOOKS[hook]):
        R.run_raw(m.c.b, m.docs)
        ids, toff, _, total, _ = download(m.c.b, len(m.docs))
        e_ids, e_raw = m.c.expected(m.which)
        assert ids.size == e_ids.size and (ids == e_ids).all()
        for text, name in KINDS:
            got, hd = spans_in(m.c.b, text, UNITS[name], total)
            exp = m.expected(text, UNITS[name])
            assert (got == exp).all(), "hook %s, text %d, %s: %s" % (hook, text, name, first_difference(got, exp, toff))
            assert hd >= 1 if text == RAW else hd == 0
        assert int(N.lib.tm_batch_host_fallback_docs(m.c.b)) >= 1
    # str in, "raw" + "chars": doc[b:e] is the text of the id
    chars, _ = spans_in(m.c.b, RAW, UR.CODEPOINTS, total)
    u16, _ = spans_in(m.c.b, RAW, UR.UTF16, total)
    for d, s in enumerate(m.strs):
        w = s.encode("utf-16-le")
        for k in range(int(toff[d]), int(toff[d + 1])):
            bb, be = e_raw[k]
            assert s[chars[k, 0]:chars[k, 1]].encode() == m.docs[d][bb:be]
            assert w[2 * u16[k, 0]:2 * u16[k, 1]].decode("utf-16-le") == s[chars[k, 0]:chars[k, 1]]


def test_python_layer_units():
    tm, _, _ = _mods()
    m = micro()
    raw, offs = tm.pack_documents(m.docs)
    text, noffs = tm.pack_documents(m.norm)
    e_ids = m.c.expected(m.which)[0]
    for name, unit in UNITS.items():
        ids, toff, sp, hd = m.c.v.tokenize_raw_spans_packed(raw, offs, unit=name)
        assert np.array_equal(ids, e_ids) and np.array_equal(sp.astype(np.int64), m.expected(RAW, unit)) and hd >= 1
        ids, toff, sp, _ = m.c.v.tokenize_spans_packed(text, noffs, unit=name)
        assert np.array_equal(ids, e_ids) and np.array_equal(sp.astype(np.int64), m.expected(NORM, unit))
    with pytest.raises(ValueError):
        m.c.v.tokenize_spans_packed(text, noffs, unit="graphemes")


# ---- byte identity ----------------------------------------------------------------------------------------------------------------------------------------
def host_call(fn, v, docs, *extra):
    tm, N, _ = _mods()
    text, offs = tm.pack_documents(docs)
    nd, cap = len(docs), int(text.size * 4 + 64)
    ids, sp = np.zeros(cap, dtype=np.uint32), np.zeros((cap, 2), dtype=np.uint32)
    toff, miss = np.zeros(nd + 1, dtype=np.uint64), np.zeros(nd, dtype=np.uint32)
    N.check(fn(v.handle, N.ptr(text), N.ptr(offs), nd, *extra, N.ptr(ids), cap, N.ptr(toff), N.ptr(sp), N.ptr(miss)))
    n = int(toff[nd])
    return ids[:n], toff, sp[:n], miss


def test_with_bytes_the_new_calls_are_the_old_ones():
    _, N, _ = _mods()
    m = micro()
    b, nd = m.c.b, len(m.docs)
    R.run_raw(b, m.docs)
    _, toff, _, total, _ = download(b, nd)
    pad, bos, eos = m.c.v.n_ids() + 5, m.c.v.n_ids() + 6, m.c.v.n_ids() + 7
    for text in (NORM, RAW):
        old = (S.batch_spans(b, total), 0) if text == NORM else R.batch_raw_spans(b, total)
        got, hd = spans_in(b, text, UR.BYTES, total)
        assert np.array_equal(got, old[0].astype(np.int64)) and hd == old[1]
        # collated
        how = Collate(1, nd - 2, 33, 4, pad, bos, eos, PAD_LEFT)
        o_old, o_new = Out((nd - 2) * 33 * 2, 8, 1), Out((nd - 2) * 33 * 2, 8, 1)
        N.check((N.lib.tm_batch_collate_raw_spans if text == RAW else N.lib.tm_batch_collate_spans)(b, C.byref(how), None, o_old.ptr, 8))
        N.check(N.lib.tm_batch_collate_spans_in(b, C.byref(how), None, text, UR.BYTES, o_new.ptr, 8))
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert np.array_equal(o_old.view(np.uint64), o_new.view(np.uint64)) and o_new.sentinels_intact() and o_new.view(np.uint64).any()
        # windows
        how = Collate(0, nd, 16, 4, pad, bos, N.TM_NONE, 0)
        rows = C.c_uint64()
        N.check(N.lib.tm_batch_window_rows(b, C.byref(how), 3, C.byref(rows)))
        rows = int(rows.value)
        w_old, w_new = Out(rows * 16 * 2, 4, 3), Out(rows * 16 * 2, 4, 3)
        N.check((N.lib.tm_batch_windows_raw_spans if text == RAW else N.lib.tm_batch_windows_spans)(b, C.byref(how), 3, None, rows, w_old.ptr, 4))
        N.check(N.lib.tm_batch_windows_spans_in(b, C.byref(how), 3, None, rows, text, UR.BYTES, w_new.ptr, 4))
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert np.array_equal(w_old.view(np.uint32), w_new.view(np.uint32)) and w_new.sentinels_intact() and rows > nd
        # the host-buffer call
        docs = m.docs if text == RAW else m.norm
        a = host_call(N.lib.tm_tokenize_batch_raw_spans if text == RAW else N.lib.tm_tokenize_batch_spans, m.c.v, docs)
        z = host_call(N.lib.tm_tokenize_batch_spans_in, m.c.v, docs, text, UR.BYTES)
        assert all(np.array_equal(x, y) for x, y in zip(a, z)) and np.array_equal(z[2].astype(np.int64), got)
        for name, unit in UNITS.items():
            z = host_call(N.lib.tm_tokenize_batch_spans_in, m.c.v, docs, text, unit)
            assert np.array_equal(z[0], a[0]) and np.array_equal(z[2].astype(np.int64), m.expected(text, unit)), (text, name)


# ---- collate and windows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,name", KINDS)
def test_collated_and_windowed_pairs_are_a_gather_of_the_converted_ones(text, name):
    from test_gpu_windows import np_windows
    _, N, _ = _mods()
    m = micro()
    b, nd, unit = m.c.b, len(m.docs), UNITS[name]
    R.run_raw(b, m.docs)
    ids, toff, _, total, _ = download(b, nd)
    ragged = m.expected(text, unit)
    doc_spans = [ragged[int(toff[d]):int(toff[d + 1])] for d in range(nd)]
    doc_ids = [ids[int(toff[d]):int(toff[d + 1])] for d in range(nd)]
    pad, bos, eos = m.c.v.n_ids() + 5, m.c.v.n_ids() + 6, m.c.v.n_ids() + 7
    for L, span_bytes, shift, flags, b_, e_, first, n in ((7, 4, 1, 0, None, None, 0, nd), (64, 8, 0, PAD_LEFT, bos, eos, 2, nd - 3), (33, 4, 3, KEEP_TAIL, None, eos, 0, nd),
                                                         (257, 8, 1, PAD_LEFT | KEEP_TAIL, bos, None, 1, nd - 1)):
        how = Collate(first, n, L, 4, pad, N.TM_NONE if b_ is None else b_, N.TM_NONE if e_ is None else e_, flags)
        out = Out(n * L * 2, span_bytes, shift)
        N.check(N.lib.tm_batch_collate_spans_in(b, C.byref(how), None, text, unit, out.ptr, span_bytes))
        N.check(N.lib.tm_batch_totals(b, None, None))
        dt = np.uint32 if span_bytes == 4 else np.uint64
        exp = np_collate_spans(doc_spans[first:first + n], L, b_, e_, flags, dt)
        assert out.sentinels_intact() and np.array_equal(out.view(dt).reshape(n, L, 2), exp), (L, span_bytes, flags)
    for L, span_bytes, shift, left, b_, e_, overlap in ((7, 4, 1, False, None, None, 2), (64, 8, 0, True, bos, eos, 17), (16, 8, 1, False, bos, None, 0), (33, 4, 2, True, None, eos, 20)):
        how = Collate(0, nd, L, 4, pad, N.TM_NONE if b_ is None else b_, N.TM_NONE if e_ is None else e_, PAD_LEFT if left else 0)
        exp = np_windows(doc_ids, L, pad, b_, e_, overlap, left, doc_spans)[5]
        rows = exp.shape[0]
        out = Out(rows * L * 2, span_bytes, shift)
        N.check(N.lib.tm_batch_windows_spans_in(b, C.byref(how), overlap, None, rows, text, unit, out.ptr, span_bytes))
        N.check(N.lib.tm_batch_totals(b, None, None))
        dt = np.uint32 if span_bytes == 4 else np.uint64
        assert out.sentinels_intact() and np.array_equal(out.view(dt).reshape(rows, L, 2).astype(np.int64), exp), (L, span_bytes, overlap)
        assert rows > nd
        # one row too few: TM_E_NOSPACE, nothing written
        small = Out((rows - 1) * L * 2, span_bytes)
        assert N.lib.tm_batch_windows_spans_in(b, C.byref(how), overlap, None, rows - 1, text, unit, small.ptr, span_bytes) == N.TM_E_NOSPACE
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert small.untouched()


# ---- the index is cached until the next upload -----------------------------------------------------------------------------------------------------------
def test_the_index_is_kept_until_the_next_upload_and_is_small():
    _, N, _ = _mods()
    c = split_case()
    rng = np.random.default_rng(9903)
    docs_a = [mixed_text(rng, n).encode() for n in (700, 0, 1500, 33)]
    docs_b = [mixed_text(rng, n).encode() for n in (1500, 33, 0, 700)]
    b = new_batch(c.v, 1 << 16, 16)
    try:
        for text in (NORM, RAW):
            (R.run_raw if text == RAW else S.run_docs)(b, docs_a)
            total = download(b, len(docs_a))[3]
            S.batch_spans(b, total)
            if text == RAW:
                R.batch_raw_spans(b, total)
            before = int(N.lib.tm_batch_device_bytes(b))
            first, _ = spans_in(b, text, UR.CODEPOINTS, total)
            grown = int(N.lib.tm_batch_device_bytes(b)) - before
            # two planes of 12 bytes per 256 of text with an eighth of headroom stay below text / 8; the constant: 16 blocks of headroom, the scan's
            # sums and total, rounding
            nbytes = sum(len(d) for d in docs_a)
            assert 0 <= grown <= nbytes // 8 + 1024, grown
            assert text == RAW or grown > 0
            second, _ = spans_in(b, text, UR.CODEPOINTS, total)
            wide, _ = spans_in(b, text, UR.UTF16, total)
            again, _ = spans_in(b, text, UR.CODEPOINTS, total)
            assert int(N.lib.tm_batch_device_bytes(b)) == before + grown
            sp_a = [c.oracle(d)[1] for d in docs_a]
            assert np.array_equal(first, converted(sp_a, docs_a, UR.CODEPOINTS)) and np.array_equal(first, second) and np.array_equal(first, again)
            assert np.array_equal(wide, converted(sp_a, docs_a, UR.UTF16)) and not np.array_equal(wide, first)
            # other text of the same size: the results are the new text's
            (R.run_raw if text == RAW else S.run_docs)(b, docs_b)
            total_b = download(b, len(docs_b))[3]
            sp_b = [c.oracle(d)[1] for d in docs_b]
            for unit in (UR.UTF16, UR.CODEPOINTS):
                got, _ = spans_in(b, text, unit, total_b)
                assert np.array_equal(got, converted(sp_b, docs_b, unit))
            assert int(N.lib.tm_batch_device_bytes(b)) == before + grown
    finally:
        N.lib.tm_batch_free(b)


# ---- where the scan of the index changes form (a real device only: 4 MiB of text) ---------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("TM_EMU") == "1", reason="4 MiB of text: a real device only")
@pytest.mark.parametrize("blocks,n", [(16383, 16383 * B - 5), (16384, 16384 * B), (16385, 16384 * B + 1)])
def test_scan_forms(blocks, n):
    _, N, _ = _mods()
    c = split_case()
    rng = np.random.default_rng(9904)
    chunk = mixed_text(rng, 1 << 16).encode()
    b = new_batch(c.v, (16385 * B) + 4096, 16)
    try:
        assert -(-n // B) == blocks
        text = (chunk * (n // len(chunk) + 1))[:n]
        cuts = [0, 1000, 1000, n // 3 + 1, n // 2 + 2, n - 7, n]      # (documents may begin and end inside a character)
        docs = [text[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
        S.run_docs(b, docs)
        _, toff, _, total, _ = download(b, len(docs))
        byte = S.batch_spans(b, total)
        per_doc = [byte[int(toff[d]):int(toff[d + 1])] for d in range(len(docs))]
        for unit in (UR.CODEPOINTS, UR.UTF16):
            got, _ = spans_in(b, NORM, unit, total)
            exp = converted(per_doc, docs, unit)
            assert (got == exp).all(), "%d blocks, unit %d: %s" % (blocks, unit, first_difference(got, exp, toff))
    finally:
        N.lib.tm_batch_free(b)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing():
    tm, N, _ = _mods()
    c = split_case()
    docs = ["the cat é".encode(), b"abc"]
    b = new_batch(c.v, 1 << 12, 8)
    try:
        R.run_raw(b, docs)
        total = download(b, len(docs))[3]
        how = Collate(0, len(docs), 8, 4, c.v.n_ids() + 1, N.TM_NONE, N.TM_NONE, 0)
        text, offs = tm.pack_documents(docs)

        def all_four(text_kind, unit):
            out, cout, wout = Out(2 * 64, 4), Out(len(docs) * 8 * 2, 4), Out(16 * 8 * 2, 4)
            ids, sp = np.zeros(64, dtype=np.uint32), np.zeros((64, 2), dtype=np.uint32)
            toff, miss = np.zeros(len(docs) + 1, dtype=np.uint64), np.zeros(len(docs), dtype=np.uint32)
            hd = C.c_uint32(5)
            rcs = [N.lib.tm_batch_spans_in(b, None, text_kind, unit, out.ptr, 64, C.byref(hd), None),
                   N.lib.tm_batch_collate_spans_in(b, C.byref(how), None, text_kind, unit, cout.ptr, 4),
                   N.lib.tm_batch_windows_spans_in(b, C.byref(how), 1, None, 16, text_kind, unit, wout.ptr, 4),
                   N.lib.tm_tokenize_batch_spans_in(c.v.handle, N.ptr(text), N.ptr(offs), len(docs), text_kind, unit, N.ptr(ids), 64, N.ptr(toff), N.ptr(sp), N.ptr(miss))]
            N.check(N.lib.tm_batch_totals(b, None, None))
            clean = out.untouched() and cout.untouched() and wout.untouched() and not ids.any() and not sp.any()
            return rcs, clean

        for text_kind, unit in ((2, UR.CODEPOINTS), (NORM, 3), (RAW, 7), (0xFFFFFFFF, UR.BYTES)):
            rcs, clean = all_four(text_kind, unit)
            assert rcs == [N.TM_E_INVALID] * 4 and clean, (text_kind, unit, rcs)
        rcs, clean = all_four(RAW, UR.UTF16)
        assert rcs == [0] * 4 and not clean
        # a batch uploaded NORMALIZED has no raw text to point into: TM_TEXT_RAW is refused by the three batch calls, in every unit
        S.run_docs(b, docs)
        for unit in (UR.BYTES, UR.CODEPOINTS, UR.UTF16):
            rcs, _ = all_four(RAW, unit)
            assert rcs[:3] == [N.TM_E_INVALID] * 3 and rcs[3] == 0, rcs
            out, cout, wout = Out(2 * 64, 4), Out(len(docs) * 8 * 2, 4), Out(16 * 8 * 2, 4)
            assert N.lib.tm_batch_spans_in(b, None, RAW, unit, out.ptr, 64, None, None) == N.TM_E_INVALID
            assert N.lib.tm_batch_collate_spans_in(b, C.byref(how), None, RAW, unit, cout.ptr, 4) == N.TM_E_INVALID
            assert N.lib.tm_batch_windows_spans_in(b, C.byref(how), 1, None, 16, RAW, unit, wout.ptr, 4) == N.TM_E_INVALID
            N.check(N.lib.tm_batch_totals(b, None, None))
            assert out.untouched() and cout.untouched() and wout.untouched()
        got, _ = spans_in(b, NORM, UR.CODEPOINTS, total)
        assert np.array_equal(got, converted([c.oracle(d)[1] for d in docs], docs, UR.CODEPOINTS))
        # too small: TM_E_NOSPACE, nothing written
        out = Out(2 * 64, 4)
        assert N.lib.tm_batch_spans_in(b, None, NORM, UR.CODEPOINTS, out.ptr, total - 1, None, None) == N.TM_E_NOSPACE
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert out.untouched()
        # the four parts of a timed call
        ms = (C.c_float * 4)(-1, -1, -1, -1)
        spans_in(b, NORM, UR.UTF16, total, ms)
        assert ms[0] >= 0 and ms[1] == 0 and ms[2] == 0 and ms[3] >= 0
    finally:
        N.lib.tm_batch_free(b)


# ---- torch: offset_unit of encode_batch and encode_windows, in a child process that imports torch first ---------------------------------------------------
def torch_child(out_path):
    import torch
    torch.cuda.init()
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    results = {}
    try:
        import tokenmonster_amd as tm
        from tokenmonster_amd import synth, torch_api
        from test_gpu_windows import np_windows
        rng = np.random.default_rng(9905)
        img = synth.build_vocab(R.micro_tokens(rng, 2), capcode=2, charset=1, norm_flag=3, with_unk=True)
        v = tm.Vocab(img)
        strs = [mixed_text(rng, int(n)) for n in list(rng.integers(0, 300, size=12)) + [0, 1, 1500]] + ["Café 한 HI 😀"]
        docs = [s.encode() for s in strs]
        raw, offs = tm.pack_documents(docs)
        ids, toff, byte, _ = v.tokenize_raw_spans_packed(raw, offs)
        per_ids = [ids[int(toff[d]):int(toff[d + 1])] for d in range(len(docs))]
        per_doc = [byte[int(toff[d]):int(toff[d + 1])].astype(np.int64) for d in range(len(docs))]
        n = v.n_ids()
        pad, bos, eos = n + 1, n + 2, n + 3
        L = 40
        for name, unit in UNITS.items():
            spans = [UR.convert(sp, d, unit) for sp, d in zip(per_doc, docs)]
            try:
                out = torch_api.encode_batch(v, strs, L, pad_id=pad, bos_id=bos, eos_id=eos, return_offsets="raw", offset_unit=name)
                got = out["offset_mapping"].cpu().numpy()
                assert out["offset_mapping"].is_cuda and out["offset_mapping"].dtype == torch.int64
                assert (got == np_collate_spans(spans, L, bos, eos, 0, np.int64)).all()
                if name == "chars":
                    rows = out["input_ids"].cpu().numpy()
                    for d, s in enumerate(strs):
                        for j in range(1, 1 + min(len(per_doc[d]), L - 2)):
                            bb, be = per_doc[d][j - 1]
                            assert s[got[d, j, 0]:got[d, j, 1]].encode() == docs[d][bb:be] and rows[d, j] == per_ids[d][j - 1]
                results["encode_batch[%s]" % name] = "ok"
            except Exception:      # noqa: BLE001
                results["encode_batch[%s]" % name] = traceback.format_exc()
            try:
                out = torch_api.encode_windows(v, strs, L, 9, pad_id=pad, bos_id=bos, pad_left=True, return_offsets="raw", offset_unit=name)
                exp = np_windows(per_ids, L, pad, bos, None, 9, True, spans)[5]
                assert out["offset_mapping"].is_cuda and (out["offset_mapping"].cpu().numpy() == exp).all() and exp.shape[0] > len(docs)
                norm = torch_api.encode_windows(v, strs, L, 9, pad_id=pad, bos_id=bos, pad_left=True, return_offsets=True, offset_unit=name)
                assert norm["offset_mapping"].shape == out["offset_mapping"].shape and not torch.equal(norm["offset_mapping"], out["offset_mapping"])
                results["encode_windows[%s]" % name] = "ok"
            except Exception:      # noqa: BLE001
                results["encode_windows[%s]" % name] = traceback.format_exc()
        try:
            for fn, extra in ((torch_api.encode_batch, ()), (torch_api.encode_windows, (2,))):
                try:
                    fn(v, [b"ab"], 8, *extra, pad_id=pad, return_offsets=True, offset_unit="graphemes")
                    raise AssertionError("accepted an unknown offset_unit")
                except ValueError:
                    pass
                a = fn(v, strs, 8, *extra, pad_id=pad, return_offsets=True)
                z = fn(v, strs, 8, *extra, pad_id=pad, return_offsets=True, offset_unit="bytes")
                assert torch.equal(a["offset_mapping"], z["offset_mapping"])
            results["arguments"] = "ok"
        except Exception:      # noqa: BLE001
            results["arguments"] = traceback.format_exc()
    except Exception:      # noqa: BLE001
        results["__env__"] = traceback.format_exc()
    with open(out_path, "w") as f:
        json.dump(results, f)


@pytest.fixture(scope="module")
def torch_results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("char_offsets_torch") / "results.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and os.path.exists(out), r.stdout.decode(errors="replace")[-4000:]
    res = json.load(open(out))
    assert "__env__" not in res, res["__env__"]
    return res


@pytest.mark.parametrize("what", ["encode_batch[chars]", "encode_batch[utf16]", "encode_windows[chars]", "encode_windows[utf16]", "arguments"])
def test_torch_offset_unit(torch_results, what):
    assert torch_results.get(what) == "ok", torch_results.get(what)


if __name__ == "__main__":
    torch_child(sys.argv[1])

"""-m gpu: raw-text byte spans - tm_batch_raw_spans, tm_batch_collate_raw_spans, tm_tokenize_batch_raw_spans (the origin pass k_norm_emit<4> in
tokenmonster_amd/csrc/tm_norm.hip, k_raw_spans in tm_spans.hip) and torch_api.encode_batch(return_offsets="raw").

Expected values: the oracle's walk over the NORMALIZED document (tests/span_recipe.py), mapped through the owners by the definition of
include/tokenmonster_hip.h in a few lines of numpy (tests/origin_recipe.py: raw_spans).  The owners of a document the device maps come from
the sequential model of tests/origin_recipe.py (its bytes checked against tm_normalize); those of a document the host maps from
tm_normalize_origins, which tests/test_origin_recipe.py checks on the CPU.  tests/test_raw_spans_emulated.py runs this file (less the torch
case) on the emulated device."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import traceback

import numpy as np
import pytest

import test_gpu_spans as S
from test_gpu_spans import Collate, Out, download, hooks, new_batch, np_collate_spans, truncated_index, FILL, KEEP_TAIL, PAD_LEFT

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

HOOKS = {"plain": 0, "dense_side": 64, "direct": 1024, "packed_text": 2048, "per_lane_normalizer": 256}
RAW_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097]      # piece 1 024, chunk 64, margins 64
SEG_BATCHES = [15, 16, 17, 33]


def _mods():
    return S._mods()


def lib_origins(doc, capcode, flag):
    _, N, _ = _mods()
    d = N.as_u8(doc)
    out, own, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    N.check(N.lib.tm_normalize_origins(N.ptr(d), d.size, capcode, flag, C.byref(out), C.byref(n), C.byref(own)))
    o = np.frombuffer(C.string_at(own.value, 4 * n.value), dtype=np.uint32).astype(np.int64) if n.value else np.zeros(0, dtype=np.int64)
    N.lib.tm_free(own)
    return N.take(out, n.value), o


def run_raw(b, docs, stream=None):
    tm, N, _ = _mods()
    raw, offs = tm.pack_documents(docs)
    N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(offs), len(docs)))
    N.check(N.lib.tm_batch_normalize(b, stream))
    N.check(N.lib.tm_batch_run(b, stream))


def batch_raw_spans(b, total):
    """tm_batch_raw_spans on the NULL stream into page-locked memory -> (uint32 [total, 2], documents mapped on the host)"""
    _, N, _ = _mods()
    out = Out(2 * total, 4)
    hd = C.c_uint32(12345)
    N.check(N.lib.tm_batch_raw_spans(b, None, out.ptr, total, C.byref(hd)))
    N.check(N.lib.tm_batch_totals(b, None, None))
    assert out.sentinels_intact()
    return out.view(np.uint32).reshape(total, 2).copy(), int(hd.value)


class RawCase:
    """a vocabulary, raw documents, and what the oracle and the owners say about them (computed once, shared, never changed)"""

    def __init__(self, img, docs, host=()):
        from oracle_bind import Oracle
        from span_recipe import SpanStats, oracle_spans
        import origin_recipe as R
        tm, _, synth = _mods()
        self.img, self.docs = img, docs
        self.v, self.orc = tm.Vocab(img), Oracle(img)
        self.has_unk = self.v.unk_token_id() is not None
        cap, flag = self.v.capcode(), self.v.normalization_code()
        self.stats = SpanStats()
        self.ids, self.norm_spans, self.raw_spans, self.own = [], [], [], []
        for k, d in enumerate(docs):
            norm = synth.normalize(d, cap, flag)
            if k in host or flag & ~3:
                nb, own = lib_origins(d, cap, flag)
            else:
                nb, own = R.normalize_with_owners(d, cap, flag)
            assert nb == norm, "document %d: the owners' text is not tm_normalize's" % k
            ids, _ = self.orc.tokenize(norm)
            sp = oracle_spans(self.orc, norm, self.has_unk, self.stats)
            assert sp.shape[0] == ids.size
            self.ids.append(ids)
            self.norm_spans.append(sp)
            self.own.append(own)
            self.raw_spans.append(R.raw_spans(sp, own, len(d)))
        self.b = new_batch(self.v, 4 * sum(len(d) for d in docs) + 8192, len(docs) + 8)

    def expected(self, which):
        ids = np.concatenate([self.ids[d] for d in which] + [np.zeros(0, np.uint32)])
        sp = np.concatenate([self.raw_spans[d] for d in which] + [np.zeros((0, 2), np.int64)])
        return ids, sp

    def check(self, which, what, host_docs=0):
        run_raw(self.b, [self.docs[d] for d in which])
        ids, toff, _, total, _ = download(self.b, len(which))
        e_ids, e_sp = self.expected(which)
        assert ids.size == e_ids.size and (ids == e_ids).all(), what
        got, hd = batch_raw_spans(self.b, total)
        got = got.astype(np.int64)
        if not (got == e_sp).all():
            k = int(np.argwhere((got != e_sp).any(axis=1))[0, 0])
            d = int(np.searchsorted(toff, k, side="right")) - 1
            raise AssertionError("%s: document %d (%d raw bytes), id %d of it: raw span %s, the owners say %s (normalized %s)" % (
                what, which[d], len(self.docs[which[d]]), k - int(toff[d]), got[k].tolist(), e_sp[k].tolist(),
                self.norm_spans[which[d]][k - int(toff[d])].tolist()))
        assert hd == host_docs, (what, hd)
        return got


# ---- vocabularies and documents ------------------------------------------------------------------------------------------------------------
def micro_tokens(rng, capcode):
    import conftest
    toks = set(conftest.fuzz_vocab_tokens(rng, capcode, 220, singles=True))
    toks |= {bytes([c]) for c in b"abcdefghilnorstw .,1290'\n"}
    if capcode == 2:
        toks |= {b"D", b"C", b"W", b" h", b" a", b"D a", b"DW", b"DC", b"W h", b"C a", b" b", b"i"}
    toks |= {"́".encode(), "é".encode(), "ᄀ".encode(), "ᅡ".encode(), "か".encode(), "゙".encode()}
    return sorted(toks)


def raw_fuzz(rng, n):
    """ASCII raw text over the micro vocabulary's alphabet, with capital runs of every shape, digits and apostrophes"""
    import conftest
    t = bytearray(conftest.fuzz_text(rng, 0, max(n, 1)).replace(b"\xff", b"Q").replace(b"\x00", b"'"))
    for _ in range(len(t) // 9):
        i = int(rng.integers(0, len(t)))
        j = min(len(t), i + int(rng.choice([1, 1, 2, 3, 6])))
        t[i:j] = bytes(t[i:j]).upper()
    return bytes(t[:n])


def doc_of_normalized_length(rng, cap, flag, target):
    """a raw document whose normalized text has exactly `target` bytes"""
    _, _, synth = _mods()
    d = b" " + raw_fuzz(rng, target)
    while len(synth.normalize(d, cap, flag)) > target:
        d = d[:-1 - (len(synth.normalize(d, cap, flag)) - target) // 5]
    while len(synth.normalize(d, cap, flag)) < target:
        d += b"."
    assert len(synth.normalize(d, cap, flag)) == target
    return d


BOUNDARY_CHARS = ["é", "É", "Ấ", "—", "한", "각", "が", "パ", "\U0001F642"]      # é É Ấ — 한 각 が パ 🙂


def boundary_docs():
    """every split of a two-, three- and four-byte character, a Hangul syllable and a voiced kana across raw offset 1024; capital runs and
    runs of 70 capitals / 70 digits across it (the normalizer's exact path); a piece of aBaB... that outgrows its slab"""
    docs = []
    for ch in BOUNDARY_CHARS:
        e = ch.encode("utf-8")
        for k in range(1, len(e)):
            docs.append(b"")
            head = (b"ab c " * 300)[:1024 - k]
            docs[-1] = head + e + " Tail aéb".encode("utf-8")
            assert len(head) == 1024 - k
    for word in (b"HELLO World", b"HEllo", b"Hello", b"IT'S", b"A1b"):
        for k in range(1, len(word)):
            docs.append((b"ab c " * 300)[:1023 - k] + b" " + word + b" tail Ab")
    docs.append((b"ab c " * 300)[:990] + b"A" * 70 + b"b cd")
    docs.append((b"ab c " * 300)[:990] + b"A" * 70 + b" cd")
    docs.append((b"ab c " * 300)[:990] + b"7" * 70 + b"A cd")
    docs.append(b"aB" * 700 + b" end")
    return docs


def build_micro(seed, capcode, flag, unk):
    _, _, synth = _mods()
    rng = np.random.default_rng(seed)
    img = synth.build_vocab(micro_tokens(rng, capcode), capcode=capcode, charset=1, norm_flag=flag, with_unk=unk)
    docs = [raw_fuzz(rng, n) for n in RAW_LENS] + [b".h.h Hi.h He SHe"]
    groups = {"lens": list(range(len(docs)))}
    if capcode == 2 and flag & 1:
        bd = boundary_docs()
        groups["boundary"] = list(range(len(docs), len(docs) + len(bd)))
        docs += bd
    for nseg in SEG_BATCHES:
        g = [513, 300] + [256] * (nseg - 6) + [1]
        groups["segs%d" % nseg] = list(range(len(docs), len(docs) + len(g)))
        docs += [doc_of_normalized_length(rng, capcode, flag, n) for n in g]
    c = RawCase(img, docs)
    c.groups = groups
    for nseg in SEG_BATCHES:
        assert sum((len(c.own[d]) + 255) // 256 for d in groups["segs%d" % nseg]) == nseg
    return c


def build_synth2048(unk):
    _, _, synth = _mods()
    img = synth.synth_vocab(synth.ENGLISHCODE, 2048, capcode=2, norm_flag=1, level=3, seed=0x52415753, with_unk=unk)
    raw, offs = synth.synth_corpus(synth.ENGLISHCODE, 40_000, seed=77, median_doc=1500)
    docs = [raw[int(offs[d]):int(offs[d + 1])].tobytes() for d in range(offs.size - 1)]
    docs = [d for d in docs if all(x < 0x80 for x in d)][:24] + ["Café ÉCOLE naïve 한국어 がぎ HELLO".encode()]
    c = RawCase(img, docs)
    c.groups = {"lens": list(range(len(docs)))}
    return c


BUILDERS = {
    "micro_unk": lambda: build_micro(9801, 2, 1, True),
    "micro": lambda: build_micro(9802, 2, 1, False),
    "micro_lower_unk": lambda: build_micro(9803, 2, 3, True),
    "micro_capcode0": lambda: build_micro(9804, 0, 1, True),
    "synth2048_unk": lambda: build_synth2048(True),
    "synth2048": lambda: build_synth2048(False),
}
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


# ---- 1. raw spans against the oracle's walk mapped through the owners ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BUILDERS))
def test_raw_spans_against_the_owners(name):
    c = case(name)
    for group, which in c.groups.items():
        c.check(which, "%s, batch %s" % (name, group))


@pytest.mark.parametrize("hook", [h for h in HOOKS if h != "plain"])
def test_test_hooks_give_identical_raw_spans(hook):
    c = case("micro_unk")
    for group, which in c.groups.items():
        plain = c.check(which, "plain, batch %s" % group)
        with hooks(HOOKS[hook]):
            hooked = c.check(which, "hook %s, batch %s" % (hook, group))
        assert np.array_equal(plain, hooked)


def test_the_cases_show_every_kind_of_span():
    from span_recipe import SpanStats
    total = SpanStats()
    for name in ("micro_unk", "micro"):
        total.add(case(name).stats)
    assert total.zero >= 1 and total.delete >= 1 and total.missing_unk >= 1 and total.missing_nounk >= 1, total
    # a token boundary inside one character's output (the markers in front of a capital are one token, " h" the next): two ids with bytes of
    # their own and the SAME raw span
    c = case("micro_unk")
    shared = 0
    for nsp, sp in zip(c.norm_spans, c.raw_spans):
        both = (nsp[:-1, 1] > nsp[:-1, 0]) & (nsp[1:, 1] > nsp[1:, 0]) & (sp[:-1] == sp[1:]).all(axis=1) & (sp[:-1, 1] - sp[:-1, 0] == 1)
        shared += int(both.sum())
    assert shared >= 1
    # begins and ends never decrease
    for c in (case("micro_unk"), case("micro")):
        for sp in c.raw_spans:
            assert (np.diff(sp[:, 0]) >= 0).all() and (np.diff(sp[:, 1]) >= 0).all() and (sp[:, 1] >= sp[:, 0]).all()
    # with an unk token the spans of a document tile it
    for sp, doc in zip(case("micro_unk").raw_spans, case("micro_unk").docs):
        if len(sp):
            assert sp[0, 0] == 0 and sp[-1, 1] == len(doc)


# ---- 2. the identity anchor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 2])
def test_without_capcode_the_raw_spans_are_the_normalized_spans(flag):
    import conftest
    _, N, synth = _mods()
    tm = _mods()[0]
    rng = np.random.default_rng(9810 + flag)
    img = synth.build_vocab(conftest.fuzz_vocab_tokens(rng, 0, 200, singles=True), capcode=0, charset=1, norm_flag=flag, with_unk=True)
    v = tm.Vocab(img)
    docs = [raw_fuzz(rng, n) if flag else conftest.fuzz_text(rng, 0, max(n, 1))[:n] for n in RAW_LENS]
    if not flag:
        docs.append("café 한 \xff\xfe".encode("latin-1", "ignore") + "é한".encode())       # (without flags any byte is the device's)
    b = new_batch(v, 4 * sum(len(d) for d in docs) + 4096, len(docs) + 8)
    try:
        run_raw(b, docs)
        _, _, _, total, _ = download(b, len(docs))
        raw, hd = batch_raw_spans(b, total)
        assert np.array_equal(raw, S.batch_spans(b, total)) and total > 100 and hd == 0
    finally:
        N.lib.tm_batch_free(b)


# ---- 3. documents the host maps ----------------------------------------------------------------------------------------------------------------------
def test_a_document_the_host_maps_between_device_ones():
    _, N, synth = _mods()
    rng = np.random.default_rng(9820)
    img = synth.build_vocab(micro_tokens(rng, 2), capcode=2, charset=1, norm_flag=1, with_unk=True)
    docs = [raw_fuzz(rng, 700), "Ab ạ́ cD é x".encode(), raw_fuzz(rng, 1500), b"", raw_fuzz(rng, 90)]      # two marks out of canonical order: NF_BAD on the device
    c = RawCase(img, docs, host={1})
    try:
        got = c.check(list(range(len(docs))), "host-mapped document", host_docs=1)
        assert int(N.lib.tm_batch_host_fallback_docs(c.b)) == 1
        again, hd = batch_raw_spans(c.b, got.shape[0])
        assert np.array_equal(again, got) and hd == 1
        # the reordered stretch is one unit: the ids inside it share one raw span
        lo = int(sum(len(x) for x in c.ids[:1]))
        inside = [tuple(s) for s in c.raw_spans[1].tolist() if s[0] == 3]
        assert len(inside) >= 2 and len(set(inside)) == 1 and inside[0] == (3, 8), c.raw_spans[1].tolist()
        assert lo > 0
    finally:
        N.lib.tm_batch_free(c.b)


def test_a_vocabulary_with_a_byte_level_flag_is_mapped_on_the_host():
    _, N, synth = _mods()
    rng = np.random.default_rng(9830)
    img = synth.build_vocab(micro_tokens(rng, 2), capcode=2, charset=1, norm_flag=1 | 16, with_unk=True)
    docs = [b"a  B   c", raw_fuzz(rng, 1100).replace(b"a", b"  "), b"", b" ", b"Ab   Cd  e" * 120]
    c = RawCase(img, docs)
    try:
        c.check(list(range(len(docs))), "collapse", host_docs=len(docs))
        # the collapsed spaces fall into the span in front of them: with an unk token the spans still tile the raw document
        sp = c.raw_spans[0]
        assert sp[0, 0] == 0 and sp[-1, 1] == len(docs[0]) and ((sp[1:, 0] == sp[:-1, 1]) | (sp[1:] == sp[:-1]).all(axis=1)).all(), sp.tolist()
        assert (sp[:, 1] - sp[:, 0]).max() >= 3
    finally:
        N.lib.tm_batch_free(c.b)


# ---- 4. collated -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 7, 64, 257])
def test_collated_raw_spans_are_a_gather_of_the_ragged_ones(L):
    _, N, _ = _mods()
    c = case("micro_unk")
    rng = np.random.default_rng(9840)
    docs = [c.docs[d] for d in c.groups["lens"]] + [raw_fuzz(rng, int(n)) for n in rng.integers(0, 40, size=30)]
    run_raw(c.b, docs)
    ids, toff, _, total, _ = download(c.b, len(docs))
    ragged, _ = batch_raw_spans(c.b, total)
    assert np.array_equal(ragged[:len(c.expected(c.groups["lens"])[1])].astype(np.int64), c.expected(c.groups["lens"])[1])
    doc_spans = [ragged[int(toff[d]):int(toff[d + 1])] for d in range(len(docs))]
    doc_ids = [ids[int(toff[d]):int(toff[d + 1])] for d in range(len(docs))]
    assert min(len(s) for s in doc_spans) == 0 and max(len(s) for s in doc_spans) > 257
    pad, bos, eos = c.v.n_ids() + 5, c.v.n_ids() + 6, c.v.n_ids() + 7
    k = 0
    for flags in (0, PAD_LEFT, KEEP_TAIL, PAD_LEFT | KEEP_TAIL):
        for b_, e_ in ((None, None), (bos, None), (None, eos), (bos, eos)):
            if L < (b_ is not None) + (e_ is not None):
                continue
            combos = [(4, 1), (4, 2), (4, 3), (8, 1), (8, 0), (4, 0)]
            for span_bytes, shift in (combos if L == 7 else [combos[k % 6]]):
                first, nd = (0, len(docs)) if k % 3 else (3, len(docs) - 5)
                k += 1
                how = Collate(first, nd, L, 4, pad, N.TM_NONE if b_ is None else b_, N.TM_NONE if e_ is None else e_, flags)
                out = Out(nd * L * 2, span_bytes, shift)
                N.check(N.lib.tm_batch_collate_raw_spans(c.b, C.byref(how), None, out.ptr, span_bytes))
                idm, mask, lens = Out(nd * L, 4), Out(nd * L, 1), Out(nd, 4)
                N.check(N.lib.tm_batch_collate(c.b, C.byref(how), None, idm.ptr, mask.ptr, lens.ptr))
                N.check(N.lib.tm_batch_totals(c.b, None, None))
                dt = np.uint32 if span_bytes == 4 else np.uint64
                exp = np_collate_spans(doc_spans[first:first + nd], L, b_, e_, flags, dt)
                got = out.view(dt).reshape(nd, L, 2)
                assert out.sentinels_intact() and np.array_equal(got, exp), (L, flags, b_, e_, span_bytes, shift, first)
                # column for column with tm_batch_collate: where it put content id j of a row, the pair of id j stands
                gi = idm.view(np.uint32).reshape(nd, L)
                for r in range(nd):
                    idx = truncated_index(len(doc_ids[first + r]), L, b_, e_, flags)
                    n = len(idx) + (b_ is not None) + (e_ is not None)
                    lo = (L - n if flags & PAD_LEFT else 0) + (b_ is not None)
                    assert np.array_equal(gi[r, lo:lo + len(idx)], doc_ids[first + r][idx]) and np.array_equal(got[r, lo:lo + len(idx)], doc_spans[first + r][idx])
    assert np.array_equal(download(c.b, len(docs))[0], ids)


# ---- 5. nothing disturbed -------------------------------------------------------------------------------------------------------------------------------
def decoded(b, nd):
    _, N, _ = _mods()
    nbytes, hd = C.c_uint64(), C.c_uint32()
    N.check(N.lib.tm_batch_decode(b, 0, None, C.byref(nbytes), C.byref(hd)))
    out = np.zeros(int(nbytes.value) + 64, dtype=np.uint8)
    off = np.zeros(nd + 1, dtype=np.uint64)
    N.check(N.lib.tm_batch_decoded_download(b, N.ptr(out), out.size, N.ptr(off)))
    return out[:int(off[nd])].copy(), off


def test_a_raw_span_call_leaves_the_batch_as_it_was():
    _, N, _ = _mods()
    c = case("micro_unk")
    which = c.groups["lens"] + c.groups["boundary"][:6]
    docs = [c.docs[d] for d in which]
    run_raw(c.b, docs)

    def state():
        ids, toff, miss, total, tmiss = download(c.b, len(docs))
        n = int(N.lib.tm_batch_normalized_bytes(c.b))
        text = np.zeros(max(n, 1), dtype=np.uint8)
        noff = np.zeros(len(docs) + 1, dtype=np.uint64)
        N.check(N.lib.tm_batch_download_text(c.b, N.ptr(text), n, N.ptr(noff)))
        return [ids.copy(), toff.copy(), miss.copy(), np.array([total, tmiss, n, int(N.lib.tm_batch_host_fallback_docs(c.b)), int(N.lib.tm_batch_device_bytes(c.b))]),
                S.batch_spans(c.b, total), text, noff]

    batch_raw_spans(c.b, download(c.b, len(docs))[3])                # (the grow-only buffers exist from here on)
    before = state()
    first, _ = batch_raw_spans(c.b, int(before[3][0]))
    between = state()
    dec1 = decoded(c.b, len(docs))
    second, _ = batch_raw_spans(c.b, int(before[3][0]))
    after = state()
    dec2 = decoded(c.b, len(docs))
    for other in (between, after):
        for x, y in zip(before, other):
            assert np.array_equal(x, y)
    assert np.array_equal(first, second) and np.array_equal(first.astype(np.int64), c.expected(which)[1])
    assert np.array_equal(dec1[0], dec2[0]) and np.array_equal(dec1[1], dec2[1])


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    tm, N, _ = _mods()
    c = case("micro_unk")
    docs = [c.docs[d] for d in c.groups["segs17"]]
    b = new_batch(c.v, 1 << 17, 64)
    try:
        out = Out(2 * 16384, 4)
        how = Collate(0, len(docs), 16, 4, c.v.n_ids() + 1, N.TM_NONE, N.TM_NONE, 0)
        cout = Out(len(docs) * 16 * 2, 4)
        hd = C.c_uint32()
        # no run yet: fresh, and after an upload
        assert N.lib.tm_batch_raw_spans(b, None, out.ptr, 16384, C.byref(hd)) == N.TM_E_INVALID
        raw, offs = tm.pack_documents(docs)
        N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(offs), len(docs)))
        assert N.lib.tm_batch_raw_spans(b, None, out.ptr, 16384, None) == N.TM_E_INVALID
        N.check(N.lib.tm_batch_normalize(b, None))
        assert N.lib.tm_batch_collate_raw_spans(b, C.byref(how), None, cout.ptr, 4) == N.TM_E_INVALID
        N.check(N.lib.tm_batch_run(b, None))
        _, _, _, total, _ = download(b, len(docs))
        assert total > 16
        # too small: TM_E_NOSPACE, nothing written
        assert N.lib.tm_batch_raw_spans(b, None, out.ptr, total - 1, None) == N.TM_E_NOSPACE
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert out.untouched()
        # argument errors
        assert N.lib.tm_batch_raw_spans(b, None, out.ptr + 4, 16384, None) == N.TM_E_INVALID             # a pair leaves in one 8-byte store
        assert N.lib.tm_batch_collate_raw_spans(b, C.byref(how), None, cout.ptr, 2) == N.TM_E_INVALID
        assert N.lib.tm_batch_collate_raw_spans(b, C.byref(how), None, None, 4) == N.TM_E_INVALID
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert out.untouched() and cout.untouched()
        # and it works
        N.check(N.lib.tm_batch_raw_spans(b, None, out.ptr, 16384, C.byref(hd)))
        N.check(N.lib.tm_batch_collate_raw_spans(b, C.byref(how), None, cout.ptr, 4))
        N.check(N.lib.tm_batch_totals(b, None, None))
        e_sp = c.expected(c.groups["segs17"])[1]
        assert np.array_equal(out.view(np.uint32)[:2 * total].reshape(total, 2).astype(np.int64), e_sp) and hd.value == 0
        assert (out.view(np.uint8)[8 * total:] == FILL).all()
        # a batch uploaded NORMALIZED has no raw text to point into - the normalized spans are there, the raw ones are refused
        norm = [c.v.normalize(d) for d in docs]
        text, noffs = tm.pack_documents(norm)
        N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(noffs), len(docs)))
        N.check(N.lib.tm_batch_run(b, None))
        out2 = Out(2 * 16384, 4)
        assert N.lib.tm_batch_raw_spans(b, None, out2.ptr, 16384, None) == N.TM_E_INVALID
        assert N.lib.tm_batch_collate_raw_spans(b, C.byref(how), None, cout.ptr, 4) == N.TM_E_INVALID
        N.check(N.lib.tm_batch_spans(b, None, out2.ptr, 16384))
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert not out2.untouched()
        # ids that came from no walk: tm_batch_load_ids behind a raw run
        N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(offs), len(docs)))
        N.check(N.lib.tm_batch_normalize(b, None))
        N.check(N.lib.tm_batch_run(b, None))
        rows = Out(4 * 8, 4)
        rows.view(np.uint32)[:] = 1
        N.check(N.lib.tm_batch_load_ids(b, rows.ptr, 4, 8, 4, None, N.TM_NONE, N.TM_NONE, N.TM_NONE, None))
        out3 = Out(2 * 64, 4)
        how3 = Collate(0, 4, 8, 4, c.v.n_ids() + 1, N.TM_NONE, N.TM_NONE, 0)
        assert N.lib.tm_batch_raw_spans(b, None, out3.ptr, 64, None) == N.TM_E_INVALID
        assert N.lib.tm_batch_collate_raw_spans(b, C.byref(how3), None, out3.ptr, 4) == N.TM_E_INVALID
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert out3.untouched()
        # a new raw run makes them available again
        run_raw(b, docs)
        assert np.array_equal(batch_raw_spans(b, total)[0].astype(np.int64), e_sp)
    finally:
        N.lib.tm_batch_free(b)


# ---- 7. the host-buffer call and the Python layer ------------------------------------------------------------------------------------------------------
def host_buffer_call(v, docs, cap=None):
    tm, N, _ = _mods()
    raw, offs = tm.pack_documents(docs)
    nd = len(docs)
    cap = int(raw.size * 4 + 64) if cap is None else cap
    ids = np.zeros(max(cap, 1), dtype=np.uint32)
    sp = np.zeros((max(cap, 1), 2), dtype=np.uint32)
    toff = np.zeros(nd + 1, dtype=np.uint64)
    miss = np.zeros(max(nd, 1), dtype=np.uint32)
    rc = N.lib.tm_tokenize_batch_raw_spans(v.handle, N.ptr(raw), N.ptr(offs), nd, N.ptr(ids), cap, N.ptr(toff), N.ptr(sp), N.ptr(miss))
    return rc, ids, toff, sp, miss


def test_host_buffer_call_from_four_threads():
    _, N, _ = _mods()
    c = case("micro_unk")
    base = c.groups["lens"] + c.groups["boundary"][:8]
    orders = [base, list(reversed(base)), base[::2], base[1::2]]
    res, errs = [None] * 4, []

    def work(k):
        try:
            for _ in range(2):
                res[k] = host_buffer_call(c.v, [c.docs[d] for d in orders[k]])
        except Exception:      # noqa: BLE001
            errs.append(traceback.format_exc())

    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in range(4):
        rc, ids, toff, sp, _ = res[k]
        e_ids, e_sp = c.expected(orders[k])
        n = int(toff[len(orders[k])])
        assert rc == 0 and n == e_ids.size and np.array_equal(ids[:n], e_ids) and np.array_equal(sp[:n].astype(np.int64), e_sp), k
    # TM_E_NOSPACE: tok_offsets is filled, nothing else
    n = int(res[0][2][len(base)])
    rc, ids, toff, sp, _ = host_buffer_call(c.v, [c.docs[d] for d in base], cap=n - 1)
    assert rc == N.TM_E_NOSPACE and np.array_equal(toff, res[0][2]) and not ids.any() and not sp.any()


def test_python_layer():
    tm, _, _ = _mods()
    c = case("micro_unk")
    which = c.groups["lens"]
    raw, offs = tm.pack_documents([c.docs[d] for d in which])
    ids, toff, sp, hd = c.v.tokenize_raw_spans_packed(raw, offs)
    e_ids, e_sp = c.expected(which)
    assert np.array_equal(ids, e_ids) and sp.shape == (ids.size, 2) and np.array_equal(sp.astype(np.int64), e_sp) and hd == 0 and toff[-1] == ids.size
    e = c.v.tokenize_raw_spans_packed(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert e[0].size == 0 and e[2].shape == (0, 2) and e[3] == 0
    text, own = c.v.normalize_origins(b"a HI")
    assert text == c.v.normalize(b"a HI") == b"D aW hi" and own.tolist() == [0, 0, 0, 1, 2, 2, 3]


# ---- 8. torch: encode_batch(return_offsets="raw"), in a child process that imports torch first ---------------------------------------------------------
def torch_child(out_path):
    import torch
    torch.cuda.init()
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    results = {}
    try:
        import tokenmonster_amd as tm
        from tokenmonster_amd import synth, torch_api
        rng = np.random.default_rng(9870)
        img = synth.build_vocab(micro_tokens(rng, 2), capcode=2, charset=1, norm_flag=1, with_unk=True)
        v = tm.Vocab(img)
        docs = [raw_fuzz(rng, int(n)) for n in list(rng.integers(0, 400, size=20)) + [0, 1, 2500]] + ["Café 한 HI".encode()]
        raw, offs = tm.pack_documents(docs)
        ids, toff, ragged, _ = v.tokenize_raw_spans_packed(raw, offs)
        spans = [ragged[int(toff[d]):int(toff[d + 1])].astype(np.int64) for d in range(len(docs))]
        n = v.n_ids()
        pad, bos, eos = n + 1, n + 2, n + 3
        L = 48
        for left in (False, True):
            name = "raw_offsets[%s]" % ("left" if left else "right")
            try:
                out = torch_api.encode_batch(v, docs, L, pad_id=pad, bos_id=bos, eos_id=eos, pad_left=left, keep_tail=left, return_offsets="raw")
                norm = torch_api.encode_batch(v, docs, L, pad_id=pad, bos_id=bos, eos_id=eos, pad_left=left, keep_tail=left, return_offsets=True)
                got = out["offset_mapping"].cpu().numpy()
                flags = (PAD_LEFT | KEEP_TAIL) if left else 0
                assert out["offset_mapping"].dtype == torch.int64 and got.shape == (len(docs), L, 2) and torch.equal(out["input_ids"], norm["input_ids"])
                assert (got == np_collate_spans(spans, L, bos, eos, flags, np.int64)).all()
                assert not torch.equal(out["offset_mapping"], norm["offset_mapping"])
                results[name] = "ok"
            except Exception:      # noqa: BLE001
                results[name] = traceback.format_exc()
        try:
            for bad in (dict(raw=False, return_offsets="raw"), dict(return_offsets="normalized")):
                try:
                    torch_api.encode_batch(v, [b"ab"], 8, pad_id=pad, **bad)
                    raise AssertionError("accepted %r" % (bad,))
                except ValueError:
                    pass
            results["arguments"] = "ok"
        except Exception:      # noqa: BLE001
            results["arguments"] = traceback.format_exc()
    except Exception:      # noqa: BLE001
        results["__env__"] = traceback.format_exc()
    with open(out_path, "w") as f:
        json.dump(results, f)


@pytest.fixture(scope="module")
def torch_results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("raw_spans_torch") / "results.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and os.path.exists(out), r.stdout.decode(errors="replace")[-4000:]
    res = json.load(open(out))
    assert "__env__" not in res, res["__env__"]
    return res


@pytest.mark.parametrize("what", ["raw_offsets[right]", "raw_offsets[left]", "arguments"])
def test_torch_encode_batch_return_offsets_raw(torch_results, what):
    assert torch_results.get(what) == "ok", torch_results.get(what)


if __name__ == "__main__":
    torch_child(sys.argv[1])

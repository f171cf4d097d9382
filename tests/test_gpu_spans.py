"""-m gpu: the byte span of every id - tm_batch_spans, tm_batch_collate_spans, tm_tokenize_batch_spans (tokenmonster_amd/csrc/tm_spans.hip) and
torch_api.encode_batch(return_offsets=True) - against the oracle's walk chained one token boundary at a time (tests/span_recipe.py; the recipe
itself is checked on the CPU by tests/test_span_recipe.py).  Spans are never checked by comparing text[a:e] with a token's bytes: the "D "
duplicates make that false for half the tokens.  tests/test_spans_emulated.py runs this file (less the torch cases) on the emulated device."""
import base64
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import traceback

import numpy as np
import pytest

from fixed_shape import Collate, Out, FILL, KEEP_TAIL, PAD_LEFT

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

HOOKS = {"plain": 0, "dense_side": 64, "direct": 1024, "deep_tree": 4096, "id_staging": 32768}      # test hooks 6, 10, 12, 15 (include/tokenmonster_hip.h)
DOC_LENS = [0, 1, 2, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097]
SEG_BATCHES = [15, 16, 17, 33]


def _mods():
    import tokenmonster_amd as tm
    from tokenmonster_amd import _native as N, synth
    return tm, N, synth


@contextlib.contextmanager
def hooks(flags):
    _, N, _ = _mods()
    old = N.lib.tm_debug_flags(flags)
    try:
        yield
    finally:
        N.lib.tm_debug_flags(old)


# ---- batches at the C ABI ------------------------------------------------------------------------------------------------------------------
def new_batch(v, max_bytes, max_docs):
    _, N, _ = _mods()
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, max_bytes, max_docs, C.byref(b)))
    return b


def download(b, nd):
    """-> (ids, tok_offsets, missing, total ids, total missing) of the batch's last run"""
    _, N, _ = _mods()
    n, m = C.c_uint64(), C.c_uint64()
    N.check(N.lib.tm_batch_totals(b, C.byref(n), C.byref(m)))
    ids = np.zeros(max(n.value, 1), dtype=np.uint32)
    toff = np.zeros(nd + 1, dtype=np.uint64)
    miss = np.zeros(max(nd, 1), dtype=np.uint32)
    N.check(N.lib.tm_batch_download(b, N.ptr(ids), n.value, N.ptr(toff), N.ptr(miss)))
    assert toff[nd] == n.value
    return ids[:n.value], toff, miss[:nd], int(n.value), int(m.value)


def batch_spans(b, total):
    """tm_batch_spans on the NULL stream into page-locked memory -> uint32 [total, 2]"""
    _, N, _ = _mods()
    out = Out(2 * total, 4)
    N.check(N.lib.tm_batch_spans(b, None, out.ptr, total))
    N.check(N.lib.tm_batch_totals(b, None, None))                      # (waits for the NULL stream)
    assert out.sentinels_intact()
    return out.view(np.uint32).reshape(total, 2).copy()


def run_docs(b, docs):
    tm, N, _ = _mods()
    text, offs = tm.pack_documents(docs)
    N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(offs), len(docs)))
    N.check(N.lib.tm_batch_run(b, None))


# ---- the cases: a vocabulary, documents, and what the oracle says about them (computed once, shared, never changed) ------------------------
class Case:
    def __init__(self, img, docs, has_unk):
        from oracle_bind import Oracle
        from span_recipe import SpanStats, check_order, oracle_spans
        tm, _, _ = _mods()
        self.img, self.docs, self.has_unk = img, docs, has_unk
        self.v, self.orc = tm.Vocab(img), Oracle(img)
        self.stats = SpanStats()
        self.ids, self.spans = [], []
        for d in docs:
            ids, _ = self.orc.tokenize(d)
            sp = oracle_spans(self.orc, d, has_unk, self.stats)
            assert sp.shape[0] == ids.size
            check_order(sp)
            self.ids.append(ids)
            self.spans.append(sp)
        self.b = new_batch(self.v, sum(len(d) for d in docs) + 4096, len(docs) + 8)

    def expected(self, which):
        ids = np.concatenate([self.ids[d] for d in which] + [np.zeros(0, np.uint32)])
        sp = np.concatenate([self.spans[d] for d in which] + [np.zeros((0, 2), np.int64)])
        return ids, sp

    def check(self, which, what):
        """the documents `which` as one batch: ids and spans against the oracle, every document"""
        run_docs(self.b, [self.docs[d] for d in which])
        ids, toff, _, total, _ = download(self.b, len(which))
        e_ids, e_sp = self.expected(which)
        assert ids.size == e_ids.size and (ids == e_ids).all(), what
        got = batch_spans(self.b, total).astype(np.int64)
        if not (got == e_sp).all():
            k = int(np.argwhere((got != e_sp).any(axis=1))[0, 0])
            d = int(np.searchsorted(toff, k, side="right")) - 1
            raise AssertionError("%s: document %d (%d bytes), id %d of it: span %s, the oracle's walk says %s" % (
                what, which[d], len(self.docs[which[d]]), k - int(toff[d]), got[k].tolist(), e_sp[k].tolist()))


def fuzz_docs(rng, capcode, charset, lens):
    import conftest
    docs = []
    for n in lens:
        t = conftest.fuzz_text(rng, capcode, max(n, 1))[:n]
        if charset == 2:
            t = bytes(b for ch in t[: n // 2] for b in (ch, 0)) + (b"a" if n % 2 else b"")
        docs.append(t)
    return docs


def fuzz_case(seed, capcode, charset, unk):
    """a vocabulary as tests/fuzz_cases.py: one builds them, documents on and around the segment and tile boundaries and a few random ones, and
    behind them the documents of the 15-, 16-, 17- and 33-segment batches"""
    import conftest
    _, _, synth = _mods()
    rng = np.random.default_rng(seed)
    toks = conftest.fuzz_vocab_tokens(rng, capcode, int(rng.integers(60, 300)), singles=True)
    if charset == 2:
        toks = sorted({bytes(b for ch in t for b in (ch, 0))[:40] for t in toks if len(t) <= 20})
    img = synth.build_vocab(toks, capcode=capcode, charset=charset, with_unk=unk)
    lens = DOC_LENS + [int(x) for x in rng.integers(0, 6001, size=4)]
    case_lens, groups = list(lens), {"main": list(range(len(lens)))}
    for nseg in SEG_BATCHES:                       # documents of 3, 2 and 1 segments that make `nseg` together
        g = [513, 300] + [256] * (nseg - 6) + [1]
        assert sum((n + 255) // 256 for n in g) == nseg
        groups["segs%d" % nseg] = list(range(len(case_lens), len(case_lens) + len(g)))
        case_lens += g
    c = Case(img, fuzz_docs(rng, capcode, charset, case_lens), unk)
    c.groups = groups
    return c


def wide_or_byte_case(wide):
    """the vocabulary and texts of test_walk_with_an_id_per_byte_and_more (tests/test_gpu_parity.py): an id for every byte and, where delete
    tokens follow, more ids than bytes; wide: 66 000 more tokens, so that the rows carry u32 ids (one plane of words under hook 15)"""
    import conftest
    _, _, synth = _mods()
    rng = np.random.default_rng(4242)
    alphabet = b"qrstuvwx"
    toks = [bytes([c]) for c in alphabet + b" D.\n"] + [b" " + bytes([c]) for c in alphabet] + [b"D " + bytes([c]) for c in alphabet[:4]] + [b"qr", b"st", b" qr", b"D qr"]
    toks = list(dict.fromkeys(toks + conftest.fuzz_vocab_tokens(rng, 2, 60)))
    if wide:
        toks += [bytes([0x7F, 0x30 + k % 40, 0x30 + (k // 40) % 40, 0x30 + k // 1600]) for k in range(66_000)]
    img = synth.build_vocab(toks, capcode=2, charset=1, with_unk=True)
    docs = []
    for n in (1, 64, 255, 256, 257, 513, 1000, 2500):
        docs.append(bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n)))
        docs.append(bytes(rng.choice(np.frombuffer(alphabet + b"   ", dtype=np.uint8), size=n)))
        docs.append(b"".join(bytes(rng.choice([b"D a", b"D b", b"a", b"D", b" ", b"D ab", b"b."])) for _ in range(n))[:max(n, 1)])
        docs.append(conftest.fuzz_text(rng, 2, n))
    c = Case(img, docs, True)
    assert (c.v.n_ids() > 65536) == wide
    c.groups = {"main": list(range(len(docs)))}
    return c


def fixture_case(name):
    import conftest
    g = conftest.load_golden(os.path.join(conftest.GOLDEN_DIR, name))
    img = base64.b64decode(g["vocab_b64"])
    docs = [base64.b64decode(d) for d in g["docs_b64"]]
    tm, _, _ = _mods()
    c = Case(img, docs, tm.Vocab(img).unk_token_id() is not None)
    assert [x.tolist() for x in c.ids] == g["ids"]
    c.groups = {"main": list(range(len(docs)))}
    return c


# (seeds picked on the CPU, from the oracle alone: together the cases show zero-length spans, delete tokens and characters without a token
# with and without an unk token - test_the_oracle_saw_every_kind_of_span)
BUILDERS = {
    "capcode0": lambda: fuzz_case(9101, 0, 1, False),
    "capcode2_unk": lambda: fuzz_case(9102, 2, 1, True),
    "capcode2": lambda: fuzz_case(9103, 2, 1, False),
    "utf16_unk": lambda: fuzz_case(9104, 2, 2, True),
    "utf16": lambda: fuzz_case(9105, 0, 2, False),
    "wide": lambda: wide_or_byte_case(True),
    "id_per_byte": lambda: wide_or_byte_case(False),
    "fixture_fuzz11": lambda: fixture_case("fuzz_capcode0_seed11.json"),
    "fixture_fuzz12": lambda: fixture_case("fuzz_capcode2_seed12.json"),
    "fixture_fuzz13": lambda: fixture_case("fuzz_capcode2_seed13.json"),
    "fixture_englishcode": lambda: fixture_case("englishcode2048.json"),
}
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


ORACLE_PARAMS = [(n, h) for n in ("capcode0", "capcode2_unk", "capcode2", "utf16_unk", "utf16") for h in HOOKS] + \
                [(n, h) for n in ("wide", "id_per_byte") for h in ("plain", "direct", "id_staging")] + \
                [(n, "plain") for n in BUILDERS if n.startswith("fixture_")]


# ---- 1. spans against the oracle recipe ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hook", ORACLE_PARAMS)
def test_spans_against_the_oracle(name, hook):
    c = case(name)
    with hooks(HOOKS[hook]):
        for group, which in c.groups.items():
            c.check(which, "%s under hook %s, batch %s" % (name, hook, group))


def test_the_oracle_saw_every_kind_of_span():
    from span_recipe import SpanStats
    total = SpanStats()
    for name in BUILDERS:
        total.add(case(name).stats)
    assert total.zero >= 1 and total.delete >= 1 and total.missing_unk >= 1 and total.missing_nounk >= 1, total
    assert case("wide").v.n_ids() > 65536


# ---- 2. nothing disturbed ------------------------------------------------------------------------------------------------------------------
def test_a_span_call_leaves_the_run_as_it_was():
    _, N, _ = _mods()
    c = case("capcode2_unk")
    which = c.groups["main"]
    docs = [c.docs[d] for d in which]
    tm, _, _ = _mods()
    text, offs = tm.pack_documents(docs)

    def state():
        ids, toff, miss, total, tmiss = download(c.b, len(docs))
        counts, cmiss = c.v.count_packed(text, offs)
        return ids.copy(), toff.copy(), miss.copy(), total, tmiss, np.asarray(counts).copy(), np.asarray(cmiss).copy()

    run_docs(c.b, docs)
    before = state()
    first = batch_spans(c.b, before[3])
    between = state()
    second = batch_spans(c.b, before[3])
    after = state()
    for other in (between, after):
        for x, y in zip(before, other):
            assert np.array_equal(x, y)
    assert np.array_equal(first, second) and np.array_equal(first.astype(np.int64), c.expected(which)[1])
    assert before[4] == sum(int(x) for x in before[2]) and before[4] > 0


# ---- 3. the raw path -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook", [0, 2048], ids=["slabs", "packed"])
def test_spans_of_raw_text_index_the_normalized_text(hook):
    """upload raw, normalize, run, spans: they index the text tm_batch_download_text returns (left in the normalizer's slabs for the match
    kernel; packed first under test hook 11)"""
    import conftest
    from oracle_bind import Oracle
    from span_recipe import check_order, oracle_spans
    tm, N, synth = _mods()
    rng = np.random.default_rng(9301)
    toks = conftest.fuzz_vocab_tokens(rng, 2, 200, singles=True)
    toks = sorted(set(toks) | {"\u0301".encode(), "\u00e9".encode(), b"C", b"W", b"D", b"Ca", b"W x", b" the", b"ing ", b"D a"})
    img = synth.build_vocab(toks, capcode=2, charset=1, norm_flag=1, with_unk=True)
    v, orc = tm.Vocab(img), Oracle(img)
    words = ["the", "The", "THE", "a", "I", "I'm", "caf\u00e9", "\u00c9cole", "HTTPServer", "x1", "42", "snake_case", "Q", "abc", "dead bee"]
    docs = []
    for n in (0, 1, 3, 255, 257, 1023, 1025, 2049, 4097):
        parts, size = [], 0
        while size < n:
            w = str(rng.choice(words)) + str(rng.choice([" ", " ", "\n", ", ", ""]))
            parts.append(w)
            size += len(w.encode())
        docs.append("".join(parts).encode()[:n])
    raw, offs = tm.pack_documents(docs)
    nd = len(docs)
    b = new_batch(v, int(raw.size) * 4 + 4096, nd + 8)
    try:
        with hooks(hook):
            N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(offs), nd))
            N.check(N.lib.tm_batch_normalize(b, None))
            N.check(N.lib.tm_batch_run(b, None))
            ids, toff, _, total, _ = download(b, nd)
            got = batch_spans(b, total).astype(np.int64)
        n = int(N.lib.tm_batch_normalized_bytes(b))
        text = np.empty(max(n, 1), dtype=np.uint8)
        noff = np.zeros(nd + 1, dtype=np.uint64)
        N.check(N.lib.tm_batch_download_text(b, N.ptr(text), n, N.ptr(noff)))
    finally:
        N.lib.tm_batch_free(b)
    assert n > raw.size          # (capitals became markers: the normalized text is not the raw text)
    for d in range(nd):
        doc = text[int(noff[d]):int(noff[d + 1])].tobytes()
        e_ids, _ = orc.tokenize(doc)
        e_sp = oracle_spans(orc, doc, True)
        check_order(e_sp)
        lo, hi = int(toff[d]), int(toff[d + 1])
        assert np.array_equal(ids[lo:hi], e_ids) and np.array_equal(got[lo:hi], e_sp), (hook, d)


# ---- 4. collated spans ---------------------------------------------------------------------------------------------------------------------
def truncated_index(n, L, bos, eos, flags):
    room = L - (bos is not None) - (eos is not None)
    m = min(n, room)
    return np.arange(n - m, n) if flags & KEEP_TAIL else np.arange(m)


def np_collate_spans(doc_spans, L, bos, eos, flags, dtype):
    """a numpy gather of the ragged spans: the pair of every column that holds a content id, (0, 0) on BOS, EOS and padding"""
    out = np.zeros((len(doc_spans), L, 2), dtype=dtype)
    for r, sp in enumerate(doc_spans):
        idx = truncated_index(len(sp), L, bos, eos, flags)
        n = len(idx) + (bos is not None) + (eos is not None)
        lo = (L - n if flags & PAD_LEFT else 0) + (bos is not None)
        out[r, lo:lo + len(idx)] = sp[idx]
    return out


@pytest.mark.parametrize("L", [1, 2, 3, 7, 64, 65, 257])
def test_collated_spans_are_a_gather_of_the_ragged_ones(L):
    _, N, _ = _mods()
    c = case("capcode2_unk")
    rng = np.random.default_rng(9401)
    # short documents beside the long ones of the case, so that rows are padded as well as cut (row_len shorter than a document: every L here)
    import conftest
    docs = [c.docs[d] for d in c.groups["main"]] + [conftest.fuzz_text(rng, 2, int(n)) for n in rng.integers(0, 40, size=40)]
    run_docs(c.b, docs)
    ids, toff, _, total, _ = download(c.b, len(docs))
    ragged = batch_spans(c.b, total)
    doc_spans = [ragged[int(toff[d]):int(toff[d + 1])] for d in range(len(docs))]
    assert min(len(s) for s in doc_spans) == 0 and max(len(s) for s in doc_spans) > 257
    pad, bos, eos = c.v.n_ids() + 5, c.v.n_ids() + 6, c.v.n_ids() + 7
    k = 0
    for flags in (0, PAD_LEFT, KEEP_TAIL, PAD_LEFT | KEEP_TAIL):
        for b_, e_ in ((None, None), (bos, None), (None, eos), (bos, eos)):
            if L < (b_ is not None) + (e_ is not None):
                continue
            combos = [(4, 0), (4, 1), (8, 0), (8, 1)]
            for span_bytes, shift in (combos if L == 7 else [combos[k % 4]]):          # (every width and both alignments at every L; the full product at 7)
                first, nd = (0, len(docs)) if k % 3 else (3, len(docs) - 5)
                k += 1
                how = Collate(first, nd, L, 4, pad, N.TM_NONE if b_ is None else b_, N.TM_NONE if e_ is None else e_, flags)
                out = Out(nd * L * 2, span_bytes, shift)
                N.check(N.lib.tm_batch_collate_spans(c.b, C.byref(how), None, out.ptr, span_bytes))
                N.check(N.lib.tm_batch_totals(c.b, None, None))
                dt = np.uint32 if span_bytes == 4 else np.uint64
                exp = np_collate_spans(doc_spans[first:first + nd], L, b_, e_, flags, dt)
                got = out.view(dt).reshape(nd, L, 2)
                assert out.sentinels_intact() and np.array_equal(got, exp), (L, flags, b_, e_, span_bytes, shift, first)
    # the ids of the batch are what they were
    assert np.array_equal(download(c.b, len(docs))[0], ids)


# ---- 5. the host-buffer call ---------------------------------------------------------------------------------------------------------------
def test_host_buffer_call_equals_the_batch_path():
    tm, N, _ = _mods()
    c = case("capcode2")
    which = c.groups["main"]
    docs = [c.docs[d] for d in which]
    text, offs = tm.pack_documents(docs)
    e_ids, e_sp = c.expected(which)
    ids, toff, spans, missing = c.v.tokenize_spans_packed(text, offs)
    ids0, toff0, missing0 = c.v.tokenize_packed(text, offs)
    assert np.array_equal(ids, ids0) and np.array_equal(toff, toff0) and np.array_equal(missing, missing0)
    assert np.array_equal(ids, e_ids) and spans.shape == (ids.size, 2) and np.array_equal(spans.astype(np.int64), e_sp)
    run_docs(c.b, docs)
    assert np.array_equal(batch_spans(c.b, ids.size), spans)
    # TM_E_NOSPACE: tok_offsets is filled, tokens_out and spans_out are not touched
    cap = ids.size - 1
    tok, sp = Out(cap, 4), Out(2 * cap, 4)
    toff1 = np.zeros(len(docs) + 1, dtype=np.uint64)
    miss1 = np.zeros(len(docs), dtype=np.uint32)
    rc = N.lib.tm_tokenize_batch_spans(c.v.handle, N.ptr(text), N.ptr(offs), len(docs), tok.ptr, cap, N.ptr(toff1), sp.ptr, N.ptr(miss1))
    assert rc == N.TM_E_NOSPACE and np.array_equal(toff1, toff) and tok.untouched() and sp.untouched()
    # an empty batch
    e = c.v.tokenize_spans_packed(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert e[0].size == 0 and e[2].shape == (0, 2) and int(e[1][0]) == 0


def test_host_buffer_call_from_two_threads():
    tm, _, _ = _mods()
    c = case("capcode2_unk")
    which = c.groups["main"]
    jobs = [[c.docs[d] for d in which], [c.docs[d] for d in reversed(which)]]
    orders = [which, list(reversed(which))]
    res, errs = [None, None], []

    def work(k):
        try:
            for _ in range(3):
                text, offs = tm.pack_documents(jobs[k])
                res[k] = c.v.tokenize_spans_packed(text, offs)
        except Exception:      # noqa: BLE001
            errs.append(traceback.format_exc())

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in range(2):
        e_ids, e_sp = c.expected(orders[k])
        assert np.array_equal(res[k][0], e_ids) and np.array_equal(res[k][2].astype(np.int64), e_sp)


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------
def test_errors():
    tm, N, _ = _mods()
    c = case("capcode2_unk")
    docs = [c.docs[d] for d in c.groups["segs17"]]
    b = new_batch(c.v, 1 << 16, 64)
    try:
        out = Out(2 * 8192, 4)
        how = Collate(0, len(docs), 16, 4, c.v.n_ids() + 1, N.TM_NONE, N.TM_NONE, 0)
        cout = Out(len(docs) * 16 * 2, 4)
        # no run yet: fresh, and after an upload
        assert N.lib.tm_batch_spans(b, None, out.ptr, 8192) == N.TM_E_INVALID
        text, offs = tm.pack_documents(docs)
        N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(offs), len(docs)))
        assert N.lib.tm_batch_spans(b, None, out.ptr, 8192) == N.TM_E_INVALID
        assert N.lib.tm_batch_collate_spans(b, C.byref(how), None, cout.ptr, 4) == N.TM_E_INVALID
        N.check(N.lib.tm_batch_run(b, None))
        ids, toff, _, total, _ = download(b, len(docs))
        assert total > 16
        # too small: TM_E_NOSPACE, nothing written
        assert N.lib.tm_batch_spans(b, None, out.ptr, total - 1) == N.TM_E_NOSPACE
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert out.untouched()
        # argument errors
        assert N.lib.tm_batch_spans(b, None, out.ptr + 4, 8192) == N.TM_E_INVALID             # a pair leaves in one 8-byte store
        assert N.lib.tm_batch_collate_spans(b, C.byref(how), None, cout.ptr, 2) == N.TM_E_INVALID
        assert N.lib.tm_batch_collate_spans(b, C.byref(how), None, None, 4) == N.TM_E_INVALID
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert out.untouched() and cout.untouched()
        # and it works
        N.check(N.lib.tm_batch_spans(b, None, out.ptr, 8192))
        N.check(N.lib.tm_batch_collate_spans(b, C.byref(how), None, cout.ptr, 4))
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert np.array_equal(out.view(np.uint32)[:2 * total].reshape(total, 2).astype(np.int64), c.expected(c.groups["segs17"])[1])
        assert (out.view(np.uint8)[8 * total:] == FILL).all()
        # ids that came from no walk: tm_batch_load_ids
        rows = Out(4 * 8, 4)
        rows.view(np.uint32)[:] = 1
        N.check(N.lib.tm_batch_load_ids(b, rows.ptr, 4, 8, 4, None, N.TM_NONE, N.TM_NONE, N.TM_NONE, None))
        out2 = Out(2 * 64, 4)
        how2 = Collate(0, 4, 8, 4, c.v.n_ids() + 1, N.TM_NONE, N.TM_NONE, 0)
        assert N.lib.tm_batch_spans(b, None, out2.ptr, 64) == N.TM_E_INVALID
        assert N.lib.tm_batch_collate_spans(b, C.byref(how2), None, out2.ptr, 4) == N.TM_E_INVALID
        N.check(N.lib.tm_batch_totals(b, None, None))
        assert out2.untouched()
        # a new run makes them available again
        N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(offs), len(docs)))
        N.check(N.lib.tm_batch_run(b, None))
        assert np.array_equal(batch_spans(b, total).astype(np.int64), c.expected(c.groups["segs17"])[1])
    finally:
        N.lib.tm_batch_free(b)


# ---- 7. torch: encode_batch(return_offsets=True), in a child process that imports torch first (tests/test_gpu_torch_api.py) ---------------------
def torch_child(out_path):
    import torch
    torch.cuda.init()
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    results = {}
    try:
        import conftest
        import tokenmonster_amd as tm
        from tokenmonster_amd import synth, torch_api
        from oracle_bind import Oracle
        from span_recipe import oracle_spans
        rng = np.random.default_rng(9701)
        img = synth.build_vocab(conftest.fuzz_vocab_tokens(rng, 2, 200), capcode=2, charset=1, with_unk=True)
        v, orc = tm.Vocab(img), Oracle(img)
        docs = [conftest.fuzz_text(rng, 2, int(n)).replace(b"\x00", b"q").replace(b"\xff", b"Q") for n in list(rng.integers(0, 400, size=30)) + [0, 1, 3000]]
        norm = [v.normalize(d) for d in docs]
        ids = [orc.tokenize(d)[0] for d in norm]
        spans = [oracle_spans(orc, d, True) for d in norm]
        n = v.n_ids()
        pad, bos, eos = n + 1, n + 2, n + 3
        stream = torch.cuda.Stream()
        L = 48
        for left in (False, True):
            name = "offsets[%s]" % ("left" if left else "right")
            try:
                with torch.cuda.stream(stream):
                    plain = torch_api.encode_batch(v, docs, L, pad_id=pad, bos_id=bos, eos_id=eos, pad_left=left, keep_tail=left)
                    out = torch_api.encode_batch(v, docs, L, pad_id=pad, bos_id=bos, eos_id=eos, pad_left=left, keep_tail=left, return_offsets=True)
                    got = out["offset_mapping"].cpu().numpy()
                    got_ids = out["input_ids"].cpu().numpy()
                flags = (PAD_LEFT | KEEP_TAIL) if left else 0
                assert "offset_mapping" not in plain and sorted(plain) == ["attention_mask", "input_ids", "lengths"]
                assert torch.equal(plain["input_ids"], out["input_ids"]) and torch.equal(plain["lengths"], out["lengths"])
                assert out["offset_mapping"].dtype == torch.int64 and out["offset_mapping"].is_cuda and got.shape == (len(docs), L, 2)
                exp = np_collate_spans(spans, L, bos, eos, flags, np.int64)
                assert (got == exp).all()
                for r, x in enumerate(ids):                       # the ids of the same columns are the oracle's
                    idx = truncated_index(len(x), L, bos, eos, flags)
                    lo = (L - len(idx) - 2 if left else 0) + 1
                    assert (got_ids[r, lo:lo + len(idx)] == x[idx]).all()
                results[name] = "ok"
            except Exception:      # noqa: BLE001
                results[name] = traceback.format_exc()
    except Exception:      # noqa: BLE001
        results["__env__"] = traceback.format_exc()
    with open(out_path, "w") as f:
        json.dump(results, f)


@pytest.fixture(scope="module")
def torch_results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spans_torch") / "results.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and os.path.exists(out), r.stdout.decode(errors="replace")[-4000:]
    res = json.load(open(out))
    assert "__env__" not in res, res["__env__"]
    return res


@pytest.mark.parametrize("side", ["right", "left"])
def test_torch_encode_batch_return_offsets(torch_results, side):
    assert torch_results.get("offsets[%s]" % side) == "ok", torch_results.get("offsets[%s]" % side)


if __name__ == "__main__":
    torch_child(sys.argv[1])

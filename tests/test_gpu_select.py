"""-m gpu: tm_batch_length_order (tm_order.hip) and tm_batch_collate_select (tm_collate.hip) at the C ABI, outputs in tm_host_alloc memory behind sentinels,
against numpy: a stable argsort of the id counts, the collate rule row by row.  Ids from tm_batch_load_ids: every count is chosen exactly.  Twin: tests/test_select_emulated.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N, synth
from conftest import EMULATED
from fixed_shape import Collate, Out, spec, DT, KEEP_TAIL, NONE, PAD_LEFT
from test_gpu_collate import np_collate

PAD, BOS, EOS = 60001, 60002, 60003          # (no document holds them)
T = 2048                                     # ORD_TILE of tm_order.hip: the documents one workgroup of the sort owns
NDOCS = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]
pytestmark = pytest.mark.gpu
sync = lambda b: N.check(N.lib.tm_batch_totals(b, None, None))          # noqa: E731  (everything here runs on the NULL stream, which this waits for)


@pytest.fixture(scope="module")
def batch():
    v = tm.Vocab(synth.build_vocab(sorted(bytes([c]) for c in b"abcdefgh"), capcode=0, charset=1, norm_flag=0, with_unk=True))
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, 1 << 16, 8192, C.byref(b)))
    yield b
    N.lib.tm_batch_free(b)


def load(b, counts, id_bytes=4, fill=True):
    """documents of exactly counts[d] ids, every id telling its document and its place (fill=False: whatever the memory holds) -> list of id arrays"""
    docs = [(np.arange(n, dtype=np.uint32) * 7 + d * 131 + 1) % 60000 for d, n in enumerate(counts)] if fill else None
    W = max(int(max(counts)), 1)
    rows, lens = Out(len(counts) * W, id_bytes), Out(len(counts), 4)
    for d, doc in enumerate(docs or []):
        rows.view(DT[id_bytes]).reshape(len(counts), W)[d, :len(doc)] = doc
    lens.view(np.uint32)[:] = counts
    N.check(N.lib.tm_batch_load_ids(b, rows.ptr, len(counts), W, id_bytes, lens.ptr, NONE, NONE, NONE, None))
    sync(b)
    return docs


def check_order(b, counts, first, nd, desc, with_counts=True):
    c = np.asarray(counts, dtype=np.int64)[first:first + nd]
    exp = np.argsort(-c if desc else c, kind="stable") + first
    o, k = Out(nd, 4), Out(nd, 4)
    N.check(N.lib.tm_batch_length_order(b, first, nd, int(desc), None, o.ptr, k.ptr if with_counts else None))
    sync(b)
    what = (first, nd, desc, with_counts)
    assert o.sentinels_intact() and (o.view(np.uint32) == exp).all(), what
    assert (k.sentinels_intact() and (k.view(np.uint32) == c[exp - first]).all()) if with_counts else k.untouched(), what
    return o


@pytest.mark.parametrize("name", ["zero", "equal", "ascending", "descending", "ties", "byte"])
def test_order_every_size(batch, name):
    """2 T + 1 documents loaded once, every prefix of NDOCS ordered both ways: partial wavefronts, partial and several tiles, no passes to three"""
    n, rng = 2 * T + 1, np.random.default_rng(len(name))
    counts = {"zero": np.zeros(n, dtype=np.int64), "equal": np.full(n, 5), "ascending": np.arange(n), "descending": np.arange(n)[::-1], "ties": rng.integers(0, 4, size=n),
              "byte": np.concatenate([[255], rng.integers(0, 256, size=n - 1)])}[name]
    load(batch, counts, fill=False)
    for nd, desc in itertools.product(NDOCS, (False, True)):
        check_order(batch, counts, 0, nd, desc, with_counts=nd % 2 == 1)
    check_order(batch, counts, 100, T + 5, True)           # a part of the run: absolute document numbers


@pytest.mark.parametrize("name", ["second", "third", "fourth"])
def test_order_digits(batch, name):
    """the second, third and fourth digit of the count decide: 255 / 256 / 257 among 300 documents; 65535 / 65536 / 65537; one document of 2^24 + 1 ids"""
    if name == "fourth" and EMULATED:
        pytest.skip("100 MB of ids through the emulated gather")
    counts = {"second": np.random.default_rng(2).choice([0, 254, 255, 256, 257, 258, 511, 512, 513], size=300), "third": [65536, 3, 65535, 65537, 3],
              "fourth": [5, (1 << 24) + 1, 7]}[name]
    load(batch, counts, id_bytes=2 if name == "fourth" else 4, fill=False)
    for desc in (False, True):
        check_order(batch, counts, 0, len(counts), desc)
    check_order(batch, counts, 1, len(counts) - 1, False, with_counts=False)


def test_order_errors_write_nothing(batch):
    load(batch, [3, 1, 2], fill=False)
    o, k, fresh = Out(3, 4), Out(3, 4), C.c_void_p()
    for first, nd, flags, optr in ((2, 2, 0, o.ptr), (0xFFFFFFFF, 2, 0, o.ptr), (0, 3, 2, o.ptr), (0, 3, 0, None)):      # beyond the run (twice), unknown flags, no order_out
        assert N.lib.tm_batch_length_order(batch, first, nd, flags, None, optr, k.ptr) == N.TM_E_INVALID
    vocab = tm.Vocab(synth.build_vocab([b"a", b"b"], capcode=0, charset=1, norm_flag=0, with_unk=True))
    N.check(N.lib.tm_batch_create(vocab.handle, 1 << 12, 8, C.byref(fresh)))
    assert N.lib.tm_batch_length_order(fresh, 0, 0, 0, None, o.ptr, k.ptr) == N.TM_E_INVALID and b"no ids" in N.lib.tm_last_error()
    N.lib.tm_batch_free(fresh)
    N.check(N.lib.tm_batch_length_order(batch, 0, 0, 0, None, None, None))      # no documents: TM_OK
    sync(batch)
    assert o.untouched() and k.untouched()
    check_order(batch, [3, 1, 2], 0, 3, False)             # the batch is as good as before


def select(b, docs, sel, L, id_bytes, bos, eos, flags, shift, given):
    """tm_batch_collate_select of the rows `sel` against the rule; given: which of mask_out, lengths_out, bad_out are passed -> the ids' Out"""
    rows, isbad = len(sel), np.array([i >= len(docs) for i in sel], dtype=bool)
    e = list(np_collate([docs[i] if i < len(docs) else [] for i in sel], L, PAD, bos, eos, flags, DT[id_bytes]))
    e[0][isbad], e[1][isbad], e[2][isbad] = PAD, 0, 0      # an index that is no document: padding only, whatever the specials
    idx, o = Out(rows, 4), [Out(rows * L, id_bytes, shift), Out(rows * L, 1, shift), Out(rows, 4), Out(1, 4)]
    idx.view(np.uint32)[:] = sel
    how = Collate(0, rows, L, id_bytes, PAD, spec(bos), spec(eos), flags)
    N.check(N.lib.tm_batch_collate_select(b, C.byref(how), idx.ptr, None, o[0].ptr, *[x.ptr if use else None for x, use in zip(o[1:], given)]))
    sync(b)
    what = (len(sel), L, id_bytes, bos, eos, flags, shift, given)
    uses = (rows > 0, given[0] and rows > 0, given[1] and rows > 0, given[2])      # (no rows: nothing but the count is written)
    for x, exp, dt, use in zip(o, e + [np.array([isbad.sum()])], (DT[id_bytes], np.uint8, np.uint32, np.uint32), uses):
        assert (x.sentinels_intact() and (x.view(dt) == exp.reshape(-1)).all()) if use else x.untouched(), what
    return o[0]


@pytest.mark.parametrize("L,id_bytes", list(itertools.product([1, 2, 7, 8, 9, 33], [2, 4, 8])))
def test_select_every_rule(batch, L, id_bytes):
    """documents of 0, 1, L - specials +- 1 and many ids; every specials combination, flag set, output alignment and optional output, through
    the identity (tm_batch_collate's bytes), the reverse, one document in every row, a draw with repeats, 600 rows of 13 documents (more rows than
    one workgroup stages), no rows, and indices that are no documents"""
    counts = sorted({0, 1, 3 * L + 5} | {c for ns in (0, 1, 2) for c in (L - ns - 1, L - ns, L - ns + 1) if c >= 0})
    docs, nd, rng = load(batch, counts), len(counts), np.random.default_rng(L)
    sels = [np.arange(nd), np.arange(nd)[::-1], np.full(5, nd - 1), rng.integers(0, nd, size=2 * nd), rng.integers(0, nd, size=600), np.arange(0),
            np.array([1, nd, 0, nd + 1, 0xFFFFFFFF, nd - 1])]
    for k, ((has_bos, has_eos), flags) in enumerate(itertools.product(itertools.product((False, True), repeat=2), (0, PAD_LEFT, KEEP_TAIL, PAD_LEFT | KEEP_TAIL))):
        if L < has_bos + has_eos:
            continue
        bos, eos = BOS if has_bos else None, EOS if has_eos else None
        for j, sel in enumerate(sels):
            ids = select(batch, docs, sel, L, id_bytes, bos, eos, flags, (k + j) & 1, tuple(bool((k + j) >> i & 1) for i in range(3)))
            if j == 0:
                same = Out(nd * L, id_bytes, (k + j) & 1)
                N.check(N.lib.tm_batch_collate(batch, C.byref(Collate(0, nd, L, id_bytes, PAD, spec(bos), spec(eos), flags)), None, same.ptr, None, None))
                sync(batch)
                assert bytes(same.view(np.uint8)) == bytes(ids.view(np.uint8))
    how, o = Collate(1, 2, L, id_bytes, PAD, NONE, NONE, 0), Out(2 * L, id_bytes)      # first_doc must be 0; a list must be there
    assert N.lib.tm_batch_collate_select(batch, C.byref(how), o.ptr, None, o.ptr, None, None, None) == N.TM_E_INVALID and b"first_doc" in N.lib.tm_last_error()
    how.first_doc = 0
    assert N.lib.tm_batch_collate_select(batch, C.byref(how), None, None, o.ptr, None, None, None) == N.TM_E_INVALID and o.untouched()


def test_rows_through_the_length_order(batch):
    """order by length, select through the order: the lengths come out monotone and every row is its document"""
    counts = np.random.default_rng(9).integers(0, 40, size=300)
    docs, L = load(batch, counts), 24
    for desc in (False, True):
        order = check_order(batch, counts, 0, 300, desc)
        ids, lens = Out(300 * L, 4), Out(300, 4)
        N.check(N.lib.tm_batch_collate_select(batch, C.byref(Collate(0, 300, L, 4, PAD, NONE, NONE, 0)), order.ptr, None, ids.ptr, None, lens.ptr, None))
        sync(batch)
        got = lens.view(np.uint32).astype(np.int64)
        assert (np.diff(got) * (-1 if desc else 1) >= 0).all() and (got == np.minimum(counts[order.view(np.uint32)], L)).all()
        assert (ids.view(np.uint32).reshape(300, L) == np_collate([docs[d] for d in order.view(np.uint32)], L, PAD, None, None, 0, np.uint32)[0]).all()

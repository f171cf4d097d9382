"""-m gpu: whole-document packing - tm_batch_fit_rows / tm_batch_fit (tokenmonster_amd/csrc/tm_fit.hip) at the C ABI, outputs in tm_host_alloc
memory behind sentinels, against the rule of include/tokenmonster_hip.h written out in numpy, one document at a time.  The ids come from
tm_batch_load_ids, so every document's id count is chosen exactly: layout, not tokenization.  tests/test_fit_emulated.py: this file without a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N, synth
from fixed_shape import Collate, Out, DT, NONE

PAD, EOS = 60001, 60002          # (no document holds them)
pytestmark = pytest.mark.gpu


def np_fit(docs, L, eos):
    """the rule: docs (list of id arrays) -> ids u64 [rows, L], doc_index, position, lengths, row_doc, row_start"""
    out = [[]]
    for d, doc in enumerate(docs):
        ent = [int(x) for x in doc] + ([eos] if eos is not None else [])
        for done in range(0, len(ent), L):               # (take is L for every piece but the last: done moves on by it)
            take = min(len(ent) - done, L)
            if len(out[-1]) + take > L:
                out.append([])
            out[-1] += [(ent[j], d, j) for j in range(done, done + take)]
    out = out if out[0] else []
    full = np.zeros((len(out), L, 3), dtype=np.uint64) + np.array([PAD, 0xFFFFFFFF, 0], dtype=np.uint64)
    for r, row in enumerate(out):
        full[r, :len(row)] = row
    first = np.array([row[0][1:] for row in out], dtype=np.uint64).reshape(len(out), 2)
    return full[:, :, 0], full[:, :, 1], full[:, :, 2], np.array([len(row) for row in out], dtype=np.uint64), first[:, 0], first[:, 1]


@pytest.fixture(scope="module")
def batch():
    v = tm.Vocab(synth.build_vocab(sorted(bytes([c]) for c in b"abcdefgh"), capcode=0, charset=1, norm_flag=0, with_unk=True))
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, 1 << 16, 4096, C.byref(b)))
    yield b
    N.lib.tm_batch_free(b)


def load(b, counts):
    """documents of exactly counts[d] ids, every id telling its document and its place -> list of id arrays"""
    docs = [(np.arange(n, dtype=np.uint32) * 7 + d * 131 + 1) % 60000 for d, n in enumerate(counts)]
    W = max(max(counts), 1)
    rows, lens = Out(len(counts) * W, 4), Out(len(counts), 4)
    grid = rows.view(np.uint32).reshape(len(counts), W)
    for d, doc in enumerate(docs):
        grid[d, :len(doc)] = doc
    lens.view(np.uint32)[:] = counts
    N.check(N.lib.tm_batch_load_ids(b, rows.ptr, len(counts), W, 4, lens.ptr, NONE, NONE, NONE, None))
    N.check(N.lib.tm_batch_totals(b, None, None))
    return docs


def check(b, docs, first, nd, L, id_bytes, eos, shift=0, given=(True,) * 5):
    """tm_batch_fit_rows and tm_batch_fit of the documents first .. first + nd against the rule; given: which of the five optional outputs are passed"""
    e = np_fit(docs[first:first + nd], L, eos)
    rows, how = e[0].shape[0], Collate(first, nd, L, id_bytes, PAD, NONE, NONE if eos is None else eos, 0)
    what, need = (first, nd, L, id_bytes, eos, shift, given), C.c_uint64(12345)
    N.check(N.lib.tm_batch_fit_rows(b, C.byref(how), C.byref(need)))
    assert need.value == rows, what
    o = [Out(rows * L, id_bytes, shift), Out(rows * L, 4, shift), Out(rows * L, 4, shift), Out(rows, 4, shift), Out(rows, 4, shift), Out(rows, 4, shift)]
    N.check(N.lib.tm_batch_fit(b, C.byref(how), None, rows, o[0].ptr, *[x.ptr if use else None for x, use in zip(o[1:], given)]))
    N.check(N.lib.tm_batch_totals(b, None, None))          # (everything here runs on the NULL stream, which this waits for)
    for x, exp, use in zip(o, e, (True,) + tuple(given)):
        assert (x.sentinels_intact() and (x.view(DT[x.elem]) == exp.reshape(-1)).all()) if use else x.untouched(), what
    return e


@pytest.mark.parametrize("L", [1, 2, 3, 7, 64, 65, 257])
def test_fit_every_shape(batch, L):
    """id counts 0, 1, L - 1, L, L + 1, 2L - 1, 2L, 2L + 1, 3L + 1, each in front of each; leading empty documents in front of a long one, a long
    one first (first_doc = 3), a run of empty ones in mid-row; with and without eos, ids of 2, 4 and 8 bytes, outputs on and off a 16-byte boundary"""
    S = sorted({0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 1})
    counts = [0, 0, 0, 3 * L + 1] + [n for a in S for c in S for n in (a, c)] + [1, 0, 0, 0, 0, 0, 1]
    docs = load(batch, counts)
    for k, (eos, id_bytes, first) in enumerate(itertools.product((None, EOS), (2, 4, 8), (0, 3))):
        e = check(batch, docs, first, len(counts) - first - (k % 3), L, id_bytes, eos, shift=k % 4)
        assert (e[3] >= 1).all() and (e[5][np.array(counts)[first + e[4].astype(int)] + (eos is not None) <= L] == 0).all()      # no row is empty, no document that fits is cut
    for j in range(5):                                   # each optional output NULL in turn, and all of them
        check(batch, docs, 2, len(counts) - 5, L, 4, EOS, shift=1, given=tuple(i != j for i in range(5)))
    check(batch, docs, 2, len(counts) - 5, L, 8, None, given=(False,) * 5)


@pytest.mark.parametrize("name,L", [("seams", 7), ("jumps", 4096), ("long", 3), ("nothing", 4)])
def test_fit_chains(batch, name, L):
    """seams: 2 500 documents of 0 to 3 ids, openers on both sides of every seam between tiles of 1 024 documents; jumps: 3 000 documents of
    one id, a row swallows more than a tile and whole tiles have no opener; long: one document of more than 1 024 rows; nothing: no entry, no rows"""
    counts = {"seams": np.random.default_rng(5).integers(0, 4, size=2500).tolist(), "jumps": [1] * 3000, "long": [5, 3 * 1100 + 2, 0, 2], "nothing": [0] * 5}[name]
    docs = load(batch, counts)
    for k, eos in enumerate((None, EOS)):
        e = check(batch, docs, 0, len(counts), L, (4, 2)[k], eos, shift=k)
        assert name != "seams" or all(np.isin(np.arange(t - 8, t), e[4]).any() and np.isin(np.arange(t, t + 8), e[4]).any() for t in (1024, 2048))
        assert name != "jumps" or (e[0].shape[0] == 1 + k and not np.isin(np.arange(1024, 2048), e[4]).any())
        assert name != "nothing" or eos is not None or e[0].shape[0] == 0
    check(batch, docs, len(counts) // 2, len(counts) - len(counts) // 2, L, 8, EOS, shift=3)


def test_fit_errors_write_nothing(batch):
    docs, L, need = load(batch, [3, 9, 0, 4, 8, 1]), 4, C.c_uint64()
    rows = np_fit(docs, L, EOS)[0].shape[0]
    o = [Out(rows * L, 8)] + [Out(rows * L, 4) for _ in range(2)] + [Out(rows, 4) for _ in range(3)]

    def both(how, rows_cap=rows):
        rc = [N.lib.tm_batch_fit_rows(batch, C.byref(how), C.byref(need)), N.lib.tm_batch_fit(batch, C.byref(how), None, rows_cap, *[x.ptr for x in o])]
        N.check(N.lib.tm_batch_totals(batch, None, None))
        assert all(x.untouched() for x in o)
        return rc

    for how, word in ((Collate(0, 6, 0, 8, PAD, NONE, EOS, 0), b"row_len"), (Collate(0, 6, L, 8, NONE, NONE, EOS, 0), b"pad_id"),
                      (Collate(0, 6, L, 2, PAD, NONE, 65536, 0), b"two bytes"), (Collate(5, 2, L, 8, PAD, NONE, EOS, 0), b"documents")):      # the last: beyond the run
        assert both(how) == [N.TM_E_INVALID] * 2 and word in N.lib.tm_last_error()
    assert both(Collate(0, 6, L, 8, PAD, NONE, EOS, 0), rows - 1) == [N.TM_OK, N.TM_E_NOSPACE] and str(rows).encode() in N.lib.tm_last_error() and need.value == rows
    assert N.lib.tm_batch_fit(batch, C.byref(Collate(0, 6, L, 8, PAD, NONE, EOS, 0)), None, rows, None, None, None, None, None, None) == N.TM_E_INVALID
    check(batch, docs, 0, 6, L, 8, EOS)                  # the batch is as good as before

"""Every kind of character (tests/boundary_cases.py) at every byte offset across every seam of the device normalizer (tm_norm.hip), against the
host normalizer (synth.normalize_batch: tm_normalize.cpp, ICU - pinned against the reference runtime and the JS capcode by the non-GPU tests).

The seams, stated here as the constants they are - if the kernel's constants move, test_the_kernel_still_has_these_seams fails and the sweep
does not go blind:

  64                a chunk: the ballots and the chg[] bit of a piece are per 64 bytes                      tm_norm.hip:56-58
  1024, 2048        PIECE, the piece boundaries: one wavefront each                                          tm_norm.hip:41
  956, 1092         PIECE -/+ PMARGIN (68): the edges of the margins staged around the first boundary       tm_norm.hip:41, :145-147
  960, 1088         PIECE -/+ 64: the 64 bytes of a margin that k_norm_emit2<false> takes its carries from
                    begin four bytes inside the staged range                                                 tm_norm.hip:41, :557-562
  head              start 0..4: the first piece of a document has no front margin                            tm_norm.hip:145
  end               the construct last in a document of every length mod 4, and 0..4 filler bytes behind
                    it: text is loaded as whole dwords, a partial last dword again byte by byte              tm_norm.hip:148, :165-173

with 0, 3 and 70 bytes behind the construct (the document ends at the seam, inside the margin, beyond it), seven fillers that carry state
across the seam (boundary_cases.FILLERS), and beside the constructs
  the capital-run threshold    62..67 capitals in front of byte 1024 and 1..70 behind it, the run followed by a lower-case letter ('C' mode) and
                               by a space ('W' mode): at more than 64 either side the margins cannot tell, the exact path runs  tm_norm_masks.h:372-382
  the slab                     a document whose one piece normalizes to 2047, 2048 and 2049 bytes (capitals with a marker each): a piece that
                               outgrows its 2 KiB slab takes the second emit                                                    tm_norm.hip:317

The documents of ONE filler are one batch: a piece whose margins cannot tell, or one that outgrows its slab, sends its whole batch down the
exact path, so only the batches of the fillers that cannot do either (ONE_TRIP; test_the_sweep_is_what_it_says) are normalized by the one
pass with the carries taken from the margins - the usual path of the product -, the others by the exact path and its second emit (checked
once by hand with TM_TRACE=1 on the batches less their host documents, as tests/test_gpu_normalize_paths.py was: "one trip" for the first
kind, "summaries" for the second; with its host documents a batch of the first kind is the "host behind" outcome of the one pass).  The
documents whose path hangs on one byte at the far edge of a margin - the block filler around 960 and 1088 - are each a batch of their own.

All of it through seven vocabularies of 256 one-byte tokens and the hooks 0, 256 (the exact path from the start) and 2048 (the text packed), armed as
tests/test_gpu_normalize_paths.py arms them.  Per (vocabulary, hook): offsets equal, bytes equal (whole arrays first; on a mismatch the
first failing documents are named as (construct, seam, start, filler, tail)), tm_batch_host_fallback_docs EXACTLY the number of documents
the construct table says are the host's, and for (2, 1) the ids of the raw path equal the ids of the host-normalized text.  And the (2, 1)
documents at the seams 64 and 1024 through Vocab.tokenize_raw_spans_packed against tests/origin_recipe.py: the origin of a normalized byte
comes from the same piece kernels at the same seams.

On the emulated device (tests/test_normalize_boundaries_emulated.py) the sweep is cut by fixed rule: the seams 64 and 1024, the capital and
mixed fillers and - for the one pass - the words filler, 3 bytes of tail, hook 0 beyond the first vocabulary; the documents normalized alone
are kept, they are what notices a margin that is staged four bytes short."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import boundary_cases as B
import tokenmonster_amd as tm
from conftest import EMULATED
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE, PMARGIN, CHUNK, SLAB = 1024, 68, 64, 2048
SEAMS = (CHUNK, PIECE) if EMULATED else (CHUNK, PIECE - PMARGIN, PIECE - CHUNK, PIECE, PIECE + CHUNK, PIECE + PMARGIN, 2 * PIECE)
TAILS = (3,) if EMULATED else (0, 3, 70)
ONE_TRIP = ("lower", "space", "words")      # fillers without 64 block bytes in a row and without a piece that doubles: the one pass finishes their batches
FILLERS = ("words", "capital", "mixed") if EMULATED else ("lower", "space", "words", "capital", "digit", "mixed", "block")
EDGE = ((PIECE - CHUNK, PIECE + CHUNK), "block", 70)      # seams, filler, tail of edge_cases()
HOOKS = (0, 256, 2048)
FILTER_FLAGS = 2 | 8 | 16 | 32 | 128      # lowercase collapse trim quotemarks unixlines: the filter pass in front
VOCABS = [(2, 1), (2, 3), (2, 0), (0, 0), (0, 1), (0, 2), (2, FILTER_FLAGS)]      # (capcode 1: refused by the host normalizer)
PARAMS = [(cf, h) for cf in VOCABS for h in HOOKS if not EMULATED or h == 0 or cf == VOCABS[0]]

_made = {}


@pytest.fixture(scope="module", autouse=True)
def release_what_was_made():
    """the documents, references and vocabularies of this module are made once and shared by its tests - and given back when the last of them has
    run, so that the rest of the session does not carry a gigabyte of expected text and ids"""
    yield
    for x in list(_made.values()):
        if isinstance(x, tm.Vocab):
            x.close()
    _made.clear()


def kernel_constants():
    src = open(os.path.join(ROOT, "tokenmonster_amd", "csrc", "tm_norm.hip"), encoding="utf-8").read()
    assert "PIECE = %d, PMARGIN = %d" % (PIECE, PMARGIN) in src, "tm_norm.hip no longer says PIECE = 1024, PMARGIN = 68: the seams of this sweep are not the kernel's"
    assert "constexpr int SLAB = 2 * PIECE;" in src, "tm_norm.hip: the slab of a piece is no longer 2 * PIECE"
    assert "uint8_t chg[32]" in src and "NCH = PIECE / 64" in src, "tm_norm.hip: a piece is no longer swept in chunks of 64 bytes"


def test_the_kernel_still_has_these_seams():
    kernel_constants()


def cases():
    """-> [(label, document, the construct or None)], label = (construct, seam, start, filler, tail); made once.  The documents of one filler
    are contiguous, the capital runs and the slab documents come last: groups() names the ranges"""
    if "cases" in _made:
        return _made["cases"]
    out, groups = [], []
    for filler in FILLERS:
        first = len(out)
        for c in B.CONSTRUCTS:
            n = len(c.data)
            for seam in SEAMS:
                for start in B.starts(n, seam):
                    for tail in TAILS:
                        out.append(((c.name, seam, start, filler, tail), B.place(c, seam, start, filler, tail), c))
            for start in range(0, 5):                      # the head: no front margin
                for tail in TAILS:
                    out.append(((c.name, "head", start, filler, tail), B.place(c, 0, start, filler, tail), c))
            for start in range(8, 12):                     # the end: every length mod 4, the construct last; then 1..4 bytes behind it
                for tail in ((0, 1) if EMULATED else range(0, 5)):
                    out.append(((c.name, "end", start, filler, tail), B.place(c, 0, start, filler, tail), c))
        groups.append((filler, first, len(out)))
    first = len(out)
    # the capital-run threshold across byte 1024
    for before in range(62, 68):
        for behind in ((1, 65) if EMULATED else (1, 63, 64, 65, 70)):
            for lead in (b" ", b"."):
                for end, mode in ((b"a", "C"), (b" ", "W")):
                    doc = b"x" * (PIECE - before - 1) + lead + b"Q" * (before + behind) + end + b"zz z"
                    out.append((("Q-run %d+%d %s %s" % (before, behind, lead.decode(), mode), PIECE, PIECE - before, "lower", 5), doc, None))
    # the slab: one piece that normalizes to 2047, 2048, 2049 bytes - as the first piece of a document and as its second
    for extra in range(0, 8):
        body = b"A" * 511 + b"b" + b"c" * extra
        out.append((("slab A*511 b c*%d" % extra, "slab", 0, "lower", extra), body, None))
        out.append((("slab x*1024 A*511 b c*%d" % extra, "slab", PIECE, "lower", extra), b"x" * PIECE + body, None))
    groups.append(("runs and slabs", first, len(out)))
    _made["cases"], _made["groups"] = out, groups
    return out


def groups():
    """-> [(name, first, one past last)]: what goes to the device as ONE batch.  A piece whose margins cannot tell, or one that outgrows its slab,
    sends its whole BATCH down the exact path (tm_norm.hip: batch_normalize_impl): in one batch with the capital filler no document would be
    normalized by the one pass with the carries from the margins - the usual path.  The batches of the fillers in ONE_TRIP take it."""
    cases()
    return _made["groups"]


def edge_cases():
    """the documents whose path hangs on ONE byte at the far edge of a margin: the block filler (one block of capitals and digits, 66 digits and
    a capital behind the construct) around PIECE -/+ 64, each document a batch of its own, so that it takes the path the product gives it alone"""
    if "edge" not in _made:
        _made["edge"] = [((c.name, seam, start) + EDGE[1:], B.place(c, seam, start, *EDGE[1:]), c)
                         for c in B.CONSTRUCTS for seam in EDGE[0] for start in B.starts(len(c.data), seam)]
    return _made["edge"]


def packed():
    if "packed" not in _made:
        _made["packed"] = tm.pack_documents([d for _, d, _ in cases()])
    return _made["packed"]


def vocab(cf):
    if ("v", cf) not in _made:
        _made[("v", cf)] = tm.Vocab(synth.build_vocab([bytes([c]) for c in range(256)], capcode=cf[0], charset=1, norm_flag=cf[1]))
    return _made[("v", cf)]


def expected(cf):
    """the host normalizer's text and offsets (computed once, shared by the hooks)"""
    if ("e", cf) not in _made:
        text, offs = packed()
        _made[("e", cf)] = synth.normalize_batch(text, offs, cf[0], cf[1])
    return _made[("e", cf)]


def expected_edge(cf):
    if ("ee", cf) not in _made:
        text, offs = tm.pack_documents([d for _, d, _ in edge_cases()])
        etext, eoff = synth.normalize_batch(text, offs, cf[0], cf[1])
        _made[("ee", cf)] = [etext[int(eoff[k]):int(eoff[k + 1])].tobytes() for k in range(offs.size - 1)]
    return _made[("ee", cf)]


def table_host_docs(cf, rows):
    """how many of these documents the construct TABLE says are the host's"""
    return sum(1 for _, _, c in rows if c is not None and c.host(cf[0], cf[1]))


def expected_ids(cf):
    if ("ids", cf) not in _made:
        etext, eoff = expected(cf)
        _made[("ids", cf)] = vocab(cf).tokenize_packed(etext, eoff)[:2]
    return _made[("ids", cf)]


def normalize_each(v, docs):
    """every document as a batch of its own, through one workspace -> ([normalized bytes], documents that took the host path)"""
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, 4 * max(len(d) for d in docs) + 4096, 1, C.byref(b)))
    out, nfb = [], 0
    try:
        for d in docs:
            raw, offs = N.as_u8(d), np.array([0, len(d)], dtype=np.uint64)
            N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(offs), 1))
            N.check(N.lib.tm_batch_normalize(b, None))
            n = int(N.lib.tm_batch_normalized_bytes(b))
            text, noff = np.empty(max(n, 1), dtype=np.uint8), np.zeros(2, dtype=np.uint64)
            N.check(N.lib.tm_batch_download_text(b, N.ptr(text), n, N.ptr(noff)))
            assert int(noff[0]) == 0 and int(noff[1]) == n
            out.append(text[:n].tobytes())
            nfb += int(N.lib.tm_batch_host_fallback_docs(b))
    finally:
        N.lib.tm_batch_free(b)
    return out, nfb


BLOCKISH_RUN = re.compile(rb"[A-Z0-9'\x80-\xff]{%d,}" % CHUNK)      # a superset of "64 block bytes in a row" (capitals, digits, apostrophes, marks)


def test_the_sweep_is_what_it_says():
    """the table's side of the sweep, without a device: the slab documents reach 2047, 2048 and 2049 normalized bytes in one piece, the constructs
    straddle every seam at every offset, at most a quarter of the documents are the host's under (2, 1), and the batches meant for the one pass
    have no document that could send them down the exact path: no 64 bytes in a row that may be one block (tm_norm_masks.h: nm_margin_carries),
    and none that grows by more than a piece (so no piece of it outgrows its slab of 2 * PIECE; nothing the normalizer pass does shrinks a text)"""
    etext, eoff = expected((2, 1))
    lens = {}
    for k, (label, doc, c) in enumerate(cases()):
        if label[1] == "slab":      # what the piece that holds the capitals normalizes to: the document less the piece of lower case in front of it
            lens.setdefault(label[2], set()).add(int(eoff[k + 1] - eoff[k]) - len(synth.normalize(doc[:label[2]], 2, 1)))
    for first in (0, PIECE):
        assert {SLAB - 1, SLAB, SLAB + 1} <= lens[first], lens
    for c in B.CONSTRUCTS:
        n = len(c.data)
        for seam in SEAMS:
            assert list(B.starts(n, seam)) == list(range(max(seam - n - 1, 0), seam + 2))
    assert 4 * table_host_docs((2, 1), cases()) <= len(cases())
    assert [g[0] for g in groups()] == list(FILLERS) + ["runs and slabs"] and set(ONE_TRIP) & set(FILLERS)
    for cf in VOCABS:
        _, noff = expected(cf)
        roff = packed()[1]
        for name, a, b in groups():
            if name in ONE_TRIP:
                for k in range(a, b):
                    assert not BLOCKISH_RUN.search(cases()[k][1]), cases()[k][0]
                grow = (noff[a + 1:b + 1] - noff[a:b]).astype(np.int64) - (roff[a + 1:b + 1] - roff[a:b]).astype(np.int64)
                assert int(grow.max()) <= PIECE, (cf, name, int(grow.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("cf,hook", PARAMS, ids=["capcode%d-flags%d-hook%d" % (cf[0], cf[1], h) for cf, h in PARAMS])
def test_every_construct_across_every_seam(cf, hook):
    kernel_constants()
    t0 = time.time()
    v = vocab(cf)
    text, offs = packed()
    etext, eoff = expected(cf)
    eedge = expected_edge(cf)
    eids = expected_ids(cf) if cf == (2, 1) else None
    t1 = time.time()
    what = (cf, hook)
    old = N.lib.tm_debug_flags(hook)
    try:
        assert N.lib.tm_debug_flags(-1) == hook, "test hooks not armed"
        for name, a, b in groups():
            rows = cases()[a:b]
            ra, rb = int(offs[a]), int(offs[b])
            got, goff, nfb = v.normalize_packed_device(text[ra:rb], offs[a:b + 1] - offs[a])
            ea, eb = int(eoff[a]), int(eoff[b])
            if not ((goff == eoff[a:b + 1] - eoff[a]).all() and got.size == eb - ea and got.tobytes() == etext[ea:eb].tobytes()):
                bad = []
                for k, (label, doc, _) in enumerate(rows):
                    if got[int(goff[k]):int(goff[k + 1])].tobytes() != etext[int(eoff[a + k]):int(eoff[a + k + 1])].tobytes():
                        bad.append((label, len(doc)))
                raise AssertionError("%s, batch '%s': %d documents are not the host normalizer's; first (construct, seam, start, filler, tail), raw length: %s" % (
                    what, name, len(bad), bad[:6]))
            host_docs = table_host_docs(cf, rows)
            assert nfb == host_docs, "%s, batch '%s': %d documents took the host path, the construct table says %d" % (what, name, nfb, host_docs)
            if eids is not None:
                ids = v.tokenize([d for _, d, _ in rows])
                ta, tb = int(eids[1][a]), int(eids[1][b])
                flat = np.concatenate(ids)
                sizes = np.cumsum(np.array([g.size for g in ids], dtype=np.uint64))
                if not ((sizes == eids[1][a + 1:b + 1] - eids[1][a]).all() and flat.size == tb - ta and (flat == eids[0][ta:tb]).all()):
                    bad = [rows[k][0] for k in range(len(ids)) if ids[k].tobytes() != eids[0][int(eids[1][a + k]):int(eids[1][a + k + 1])].tobytes()]
                    raise AssertionError("%s, batch '%s': the ids of the raw path are not those of the host-normalized text: %s" % (what, name, bad[:6]))
        t2 = time.time()
        got, nfb = normalize_each(v, [d for _, d, _ in edge_cases()])
    finally:
        N.lib.tm_debug_flags(old)
    t3 = time.time()
    host_all = table_host_docs(cf, cases())
    print("%s: %d documents, %d raw bytes, %d expected on the host (%.1f %%) in %d batches, and %d documents alone; reference %.2f s, batches %.2f s, alone %.2f s" % (
        what, offs.size - 1, text.size, host_all, 100.0 * host_all / (offs.size - 1), len(groups()), len(eedge), t1 - t0, t2 - t1, t3 - t2))
    bad = [(edge_cases()[k][0], len(edge_cases()[k][1])) for k in range(len(eedge)) if got[k] != eedge[k]]
    assert not bad, "%s: %d documents normalized alone are not the host normalizer's; first (construct, seam, start, filler, tail), raw length: %s" % (what, len(bad), bad[:6])
    assert nfb == table_host_docs(cf, edge_cases()), "%s: %d documents normalized alone took the host path, the construct table says %d" % (what, nfb, table_host_docs(cf, edge_cases()))


# ---- raw spans over the same documents -----------------------------------------------------------------------------------------------------------
def lib_origins(doc, capcode, flag):
    d = N.as_u8(doc)
    out, own, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    N.check(N.lib.tm_normalize_origins(N.ptr(d), d.size, capcode, flag, C.byref(out), C.byref(n), C.byref(own)))
    o = np.frombuffer(C.string_at(own.value, 4 * n.value), dtype=np.uint32).astype(np.int64) if n.value else np.zeros(0, dtype=np.int64)
    N.lib.tm_free(own)
    return N.take(out, n.value), o


def recipe_constructs():
    """the constructs the sequential model of tests/origin_recipe.py is for: well-formed, marks in canonical order"""
    import unicodedata
    if "recipe" not in _made:
        ok = set()
        for c in B.CONSTRUCTS:
            if c.well_formed():
                t = c.data.decode()
                if unicodedata.normalize("NFD", t) == "".join(unicodedata.normalize("NFD", ch) for ch in t):
                    ok.add(c.name)
        _made["recipe"] = ok
    return _made["recipe"]


def test_the_owners_of_the_constructs_are_the_recipes():
    """what the raw-span sweep below takes its owners from - tm_normalize_origins, the host's - equals the sequential model of
    tests/origin_recipe.py for every construct the model is for (well-formed, marks in canonical order), alone and inside the mixed filler"""
    import origin_recipe as R
    import unicodedata
    n = 0
    for c in B.CONSTRUCTS:
        if not c.well_formed():
            continue
        s = c.data.decode()
        if unicodedata.normalize("NFD", s) != "".join(unicodedata.normalize("NFD", ch) for ch in s):
            continue
        for doc in (c.data, B.place(c, 0, 7, "mixed", 9), B.place(c, 0, 70, "capital", 70)):
            nb, own = R.normalize_with_owners(doc, 2, 1)
            lb, lown = lib_origins(doc, 2, 1)
            assert bytes(lb) == nb and (lown == own).all(), (c.name, doc)
            n += 1
    assert n >= 3 * (len(B.CONSTRUCTS) - 12)


@pytest.mark.gpu
@pytest.mark.parametrize("filler", FILLERS)
def test_raw_spans_across_the_seams(filler):
    """(2, 1), hook 0, the seams 64 and 1024: ids and raw spans of Vocab.tokenize_raw_spans_packed == origin_recipe.raw_spans of the
    normalized spans through the host's owners; the documents mapped on the host are those the table says"""
    import origin_recipe as R
    kernel_constants()
    cf = (2, 1)
    v = vocab(cf)
    which = [k for k, (label, _, c) in enumerate(cases()) if c is not None and label[1] in (CHUNK, PIECE) and label[3] == filler]
    assert len(which) >= len(B.CONSTRUCTS) * 2 * len(TAILS) * 3
    docs = [cases()[k][1] for k in which]
    t0 = time.time()
    raw, roff = tm.pack_documents(docs)
    etext, eoff = synth.normalize_batch(raw, roff, *cf)
    eids, etoff, nsp, _ = v.tokenize_spans_packed(etext, eoff)
    exp = np.zeros((eids.size, 2), dtype=np.int64)
    modelled = 0
    for j, doc in enumerate(docs):
        label, _, c = cases()[which[j]]
        if (label[1] == CHUNK or label[4] == 3) and c.name in recipe_constructs():
            # the short documents, and of the long ones those with three bytes behind the construct: the owners of the sequential model itself,
            # nothing of the product in the reference
            nb, own = R.normalize_with_owners(doc, *cf)
            modelled += 1
        else:
            # the other long ones (the model in Python takes a few seconds per megabyte) and those the model is not for: the host's owners, which
            # test_the_owners_of_the_constructs_are_the_recipes and tests/test_origin_recipe.py tie to the model
            nb, own = lib_origins(doc, *cf)
        assert bytes(nb) == etext[int(eoff[j]):int(eoff[j + 1])].tobytes(), label
        a, b = int(etoff[j]), int(etoff[j + 1])
        exp[a:b] = R.raw_spans(nsp[a:b], own, len(doc))
    assert modelled >= len(recipe_constructs()) * len(TAILS) * 3
    t1 = time.time()
    ids, toff, spans, hd = v.tokenize_raw_spans_packed(raw, roff)
    print("raw spans, filler %s: %d documents, %d raw bytes; reference %.2f s, device %.2f s" % (filler, len(docs), raw.size, t1 - t0, time.time() - t1))
    assert (toff == etoff).all() and ids.size == eids.size and (ids == eids).all(), filler
    spans = spans.astype(np.int64)
    if not (spans == exp).all():
        k = int(np.argwhere((spans != exp).any(axis=1))[0, 0])
        j = int(np.searchsorted(toff, k, side="right")) - 1
        raise AssertionError("raw spans: (construct, seam, start, filler, tail) %s, id %d of it: %s, the owners say %s" % (
            cases()[which[j]][0], k - int(toff[j]), spans[k].tolist(), exp[k].tolist()))
    assert hd == sum(1 for k in which if cases()[k][2].host(*cf)), hd

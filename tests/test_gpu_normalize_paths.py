"""The five outcomes of tm_batch_normalize (tm_norm.hip) on one small set of batches of a few dozen documents of at most a few KiB:

  one trip          every document normalized by the one pass, one wait for the host                       (a), (f)
  host behind       one pass; the documents the device leaves to the host normalizer placed behind it      (b)
  exact             a piece whose margins cannot tell (more than 64 capitals across a 1 KiB piece
                    boundary): summaries, carries, the emit kernel with the carries given                  (c)
  exact, re-emit    a piece that outgrows its 2 KiB slab: the exact path and its second emit               (d), and with host documents (e)
  per-lane rules    capcode 0, or hook 8 (256), through k_norm_emit<2>                                     every batch under 256; the capcode-0 vocabulary

under the hooks 0, 256 (the exact path from the start) and 2048 (the text packed instead of staying in the slabs), on a capcode-2 NFD
vocabulary, one with a filter pass in front (lowercase collapse trim quotemarks unixlines) and a capcode-0 one with the lowercase flag; and
(c) and (d) as raw text through a streaming encoder of 4 KiB pieces, whose normalizer call builds no group tree (piece_normalize_on).

Which path a batch takes was checked once by hand with TM_TRACE=1 on the library of the commit BEFORE the one that added this file (the
test passes there unchanged): (a) prints the "[tm_batch_normalize] one trip" line, (c) and (d) - and every raw piece of the streaming
cases - print the "[tm_batch_normalize] summaries ..." line.  The test does not read stderr.

Of (d), b"A" * 3000 + b"b" is the document that outgrows its slabs (every capital gets a marker: 12 001 normalized bytes); b"Q" * 5000
normalizes to 5 003 bytes and takes the exact path for its runs of capitals across the piece boundaries, like (c).  It is one line without
a separator, which an encoder of 4 KiB pieces refuses by contract (test_gpu_stream_encoder_raw.py, test_long_lines): through the encoder
it goes as two raw pieces, b"Q" * 2499 + b"." + b"Q" * 2500, which take the exact path as well; the re-emit of a raw piece (one_piece) is
covered by b"A" * 3000 + b"b"."""
import unicodedata

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth

HOOKS = (0, 256, 2048)
HOST_DOCS = ["ẞ große".encode(), "ＡＢ".encode()]      # left to the host normalizer by every vocabulary here
RUN_C = b"x" * 1023 + b" " + b"Q" * 130
SLAB_D = [b"Q" * 5000, b"A" * 3000 + b"b"]
FILTER_FLAGS = 2 | 8 | 16 | 32 | 128      # lowercase collapse trim quotemarks unixlines

_made = {}


def plain_docs():
    if "plain" not in _made:
        raw, offs = synth.synth_corpus(synth.ENGLISHCODE, 160_000, seed=77)
        docs = [raw[int(offs[d]):int(offs[d + 1])].tobytes()[:2500].rsplit(b" ", 1)[0] for d in range(offs.size - 1)]
        _made["plain"] = [d for d in docs if d][:30]
        assert len(_made["plain"]) >= 24
    return _made["plain"]


def batches():
    a = plain_docs()
    c = a[:10] + [RUN_C, b"y" * 2046 + b"AB" + b"C" * 70 + b"d"] + a[10:]
    d = a[:7] + SLAB_D + a[7:]
    return {"a": a,
            "b": a[:12] + HOST_DOCS[:1] + a[12:20] + HOST_DOCS[1:] + a[20:],
            "c": c,
            "d": d,
            "e": c[:14] + HOST_DOCS[:1] + SLAB_D + a[14:] + HOST_DOCS[1:],
            "f0": [],
            "f1": [b""] * 5,
            "f2": [b"a"]}


def vocab(kind):
    """-> (Vocab, capcode, normalization flags), made once per session"""
    if kind not in _made:
        if kind == "nfd":
            img, cf = synth.synth_vocab(synth.ENGLISHCODE, 1200, capcode=2, norm_flag=1, level=3, seed=7), (2, 1)
        elif kind == "filter":
            img, cf = synth.build_vocab([bytes([c]) for c in range(256)], capcode=2, charset=1, norm_flag=FILTER_FLAGS), (2, FILTER_FLAGS)
        else:
            img, cf = synth.build_vocab([bytes([c]) for c in range(256)], capcode=0, charset=1, norm_flag=3), (0, 3)
        _made[kind] = (tm.Vocab(img),) + cf
    return _made[kind]


def expected(kind, name):
    """the host normalizer's text and offsets of a batch, and the ids of that text (computed once, shared by the hooks)"""
    if (kind, name) not in _made:
        v, capcode, flags = vocab(kind)
        docs = batches()[name]
        text, offs = tm.pack_documents(docs)
        etext, eoff = synth.normalize_batch(text, offs, capcode, flags)
        ids = v.tokenize_normalized([etext[int(eoff[k]):int(eoff[k + 1])].tobytes() for k in range(len(docs))])[0] if docs else []
        _made[(kind, name)] = (text, offs, etext, eoff, ids)
    return _made[(kind, name)]


def check(kind, name, hook, host_docs):
    v, capcode = vocab(kind)[:2]
    docs = batches()[name]
    if capcode == 0:      # without capcode the device pass keeps lengths: a document with a character that NFD decomposes is the host's as well
        host_docs += sum(1 for d in docs if d not in HOST_DOCS and unicodedata.normalize("NFD", d.decode()) != d.decode())
    text, offs, etext, eoff, eids = expected(kind, name)
    old = N.lib.tm_debug_flags(hook)
    try:
        assert N.lib.tm_debug_flags(-1) == hook, "test hooks not armed"
        got, goff, nfb = v.normalize_packed_device(text, offs)
        ids = v.tokenize(docs) if docs else []
    finally:
        N.lib.tm_debug_flags(old)
    what = (kind, name, hook)
    assert (goff == eoff).all(), what
    assert got.size == etext.size and got.tobytes() == etext.tobytes(), what
    assert nfb == host_docs, what + (nfb,)
    assert len(ids) == len(eids), what
    for k, (g, h) in enumerate(zip(ids, eids)):
        assert g.size == h.size and (g == h).all(), what + (k,)


@pytest.mark.gpu
@pytest.mark.parametrize("hook", HOOKS)
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f0", "f1", "f2"])
def test_every_outcome_of_the_normalizer(name, hook):
    check("nfd", name, hook, 2 if name in ("b", "e") else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("hook", HOOKS)
@pytest.mark.parametrize("kind", ["filter", "capcode0"])
def test_filter_pass_and_capcode_0(kind, hook):
    for name in "abcd":
        check(kind, name, hook, 2 if name == "b" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("hook", HOOKS)
def test_raw_pieces_of_the_streaming_encoder(hook):
    """(c) and (d) through tm_encoder_feed_raw with 4 KiB pieces: the ids of the one-shot call"""
    v = vocab("nfd")[0]
    old = N.lib.tm_debug_flags(hook)
    try:
        enc = v.encoder(4096)
        for doc in (RUN_C, SLAB_D[1], b"Q" * 2499 + b"." + b"Q" * 2500):
            parts = [enc.feed_raw(doc)]
            last, missing = enc.finish()
            got = np.concatenate(parts + [last])
            exp = v.tokenize([doc])[0]
            assert got.size == exp.size and (got == exp).all(), (hook, doc[:8], len(doc))
            assert missing == v.tokenize_normalized(bytes(v.normalize(doc)))[1], (hook, doc[:8], len(doc))
        enc.close()
    finally:
        N.lib.tm_debug_flags(old)

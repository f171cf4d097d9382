"""Every kind of character (tests/boundary_cases.py) at every byte offset across every seam of the device capcode decoder (tm_decode.hip:
k_dec_capcode), against the host streaming decoder.

What is swept is where the construct's NORMALIZED bytes lie in the gathered text buffer, because the decoder's blocks and chunks are aligned
there and not in the document (tm_decode.hip:239): every document of the sweep is preceded by a document of lower-case filler whose length puts
the construct's first byte at seam - n - 1 .. seam + 1 (n = the bytes of its normalized form, markers included), for the seams

  16                 a store: the gather writes the text in 16-byte stores aligned in the buffer             tm_decode.hip:20-27
  64, 128, 192, 256  a chunk, and the four positions of the group of DEC_ILP = 4 chunks that are decoded at
                     once when all four are ASCII: the construct is the one chunk of the group that is not   tm_decode.hip:211, :264-323
  1024               DEC_BLK, a block of the LDS ring                                                        tm_decode.hip:211, :254-263

in two shapes of document - the construct three bytes behind the document's start (the chunk begins with positions that are not the
document's), and in the middle of four chunks of the document's own ASCII (the state, kept_in and cap_in are carried from chunk to chunk).
Beside the raw constructs, normalized by the host normalizer for capcode 2 + NFD, the sweep places marker forms written out as normalized text
(DEC_EXTRA): a marker 'C', 'W' or 'D' as the last byte of a chunk and of a block, 'W' and a word that ends exactly at the seam, 'D' in front of
a space at the seam, and capitalised letters of two bytes and with marks whose bytes straddle the seam (kept_in / cap_in).  And every
construct - raw ones and marker forms alike - once in a document of 4095, 4096, 16383 and 16384 bytes - gathered bytes, which the length classes go by (tm_decode.hip:212, :235),
and decoded bytes.

The vocabulary is the one of test_decode_tiles_blocks_and_length_classes (tests/test_gpu_parity.py).  Per document: the bytes of the host
streaming decoder, and NFD of the raw text for the well-formed constructs; tm_decode_host_docs() EXACTLY the count the table gives
(boundary_cases.DECODER_HOST); and the same from tm_batch_decode, resident, on one pass of the whole set.

On the emulated device (tests/test_decode_boundaries_emulated.py): the seams 64 and 1024, and the long documents for every eighth construct."""
import ctypes as C
import os
import time
import unicodedata

import numpy as np
import pytest

import boundary_cases as B
import tokenmonster_amd as tm
from conftest import EMULATED
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEC_BLK, DEC_ILP, CHUNK, STORE, DEC_MID, DEC_LONG = 1024, 4, 64, 16, 4096, 16384
SEAMS = (CHUNK, DEC_BLK) if EMULATED else (STORE, CHUNK, 2 * CHUNK, 3 * CHUNK, DEC_ILP * CHUNK, DEC_BLK)
LENGTHS = (DEC_MID - 1, DEC_MID, DEC_LONG - 1, DEC_LONG)
PREFIX = {"short": b"ab.", "long": b"x" * 190 + b"."}
SUFFIX = {"short": b" yz", "long": b" " + b"y" * 190}
# marker forms, as NORMALIZED text (what the ids spell), with why
DEC_EXTRA = [
    ("C hello", b"C hello", "'C' capitalises the next character: the marker as the last byte of a chunk, the letter as the first of the next"),
    ("W hello", b"W hello", "'W' and a word that ends exactly at the seam"),
    ("W hello world", b"W hello world", "the space straight after 'W' does not end the word, the next one does"),
    ("W it's 2nd", b"W it's2nd x", "digits and an apostrophe keep a capitalised word going"),
    ("D x", b"D x", "'D' in front of a space at the seam: the space is deleted"),
    ("DC e", b"DC e", "a marker behind a marker: delete and capitalise-next across the seam"),
    ("DW hello", b"DW hello", "delete and capitalise-word"),
    ("C é", "C \u00e9".encode(), "a capitalised two-byte letter: both bytes replaced, the second through cap_in"),
    ("C ж", "C \u0436".encode(), "a capitalised Cyrillic letter"),
    ("C р", "C \u0440".encode(), "р D1 80 -> Р D0 A0: the capital changes the lead byte too"),
    ("W жук", "W \u0436\u0443\u043a".encode(), "a capitalised word of two-byte letters"),
    ("C e+0302+0301", "C e\u0302\u0301".encode(), "what Ế normalizes to: the marks are kept with their letter"),
    ("W e+0301 t e+0301", "W e\u0301te\u0301 x".encode(), "marks keep a capitalised word going"),
    ("D 世", "D \u4e16".encode(), "a three-byte character behind a deleted space: kept_in carries two bytes"),
    ("D 😀", "D \U0001f600".encode(), "a four-byte character behind a deleted space: kept_in carries three bytes"),
]

_made = {}


@pytest.fixture(scope="module", autouse=True)
def release_what_was_made():
    """the documents, references and vocabularies of this module are made once and shared by its tests - and given back when the last of them has
    run, so that the rest of the session does not carry the sweeps' documents and expected text"""
    yield
    for x in list(_made.values()):
        if isinstance(x, tm.Vocab):
            x.close()
    _made.clear()


def kernel_constants():
    src = open(os.path.join(ROOT, "tokenmonster_amd", "csrc", "tm_decode.hip"), encoding="utf-8").read()
    assert "DEC_BLK = %d" % DEC_BLK in src and "DEC_ILP = %d" % DEC_ILP in src, "tm_decode.hip no longer says DEC_BLK = 1024, DEC_ILP = 4: the seams of this sweep are not the kernel's"
    assert "DEC_LONG = %d, DEC_MID = %d" % (DEC_LONG, DEC_MID) in src, "tm_decode.hip: the length classes are no longer 16384 and 4096"


def test_the_kernel_still_has_these_seams():
    kernel_constants()


def vocab():
    if "v" not in _made:
        toks = [bytes([c]) for c in range(256)] + [b"D", b"C", b"W", b"the", b" the", b"ing", b"D ", b"x" * 40, b"y" * 39 + b"C", "é".encode(), "ж".encode(), "世".encode(), "😀".encode()]
        _made["v"] = tm.Vocab(synth.build_vocab(sorted(set(toks)), capcode=2, charset=1, norm_flag=1))
    return _made["v"]


def norm(data):
    return bytes(synth.normalize(data, 2, 1))


def pad(m):
    """the normalized form of m bytes of lower-case filler"""
    if ("pad", m) not in _made:
        _made[("pad", m)] = norm(b"x" * m)
    return _made[("pad", m)]


def constructs():
    """-> [(name, normalized bytes per shape {shape: (document, p0, n)}, raw document per shape or None, on the host, NFD is a reference)]"""
    if "constructs" in _made:
        return _made["constructs"]
    out = []
    for c in B.CONSTRUCTS:
        per, raws = {}, {}
        for shape in PREFIX:
            p0 = len(norm(PREFIX[shape]))
            raw = PREFIX[shape] + c.data + SUFFIX[shape]
            doc = norm(raw)
            assert doc.startswith(norm(PREFIX[shape]))
            per[shape] = (doc, p0, len(norm(PREFIX[shape] + c.data)) - p0)
            raws[shape] = raw
        out.append((c.name, per, raws, c.name in B.DECODER_HOST, c.well_formed() and c.name not in B.NO_ROUND_TRIP, c.data))
    for name, data, why in DEC_EXTRA:
        assert why
        per = {}
        for shape in PREFIX:
            pre = norm(PREFIX[shape])
            per[shape] = (pre + data + SUFFIX[shape], len(pre), len(data))
        out.append((name, per, None, False, False, None))
    _made["constructs"] = out
    return out


class Batch:
    """normalized documents, their labels, which the table says are the host's, and what the references say of each (made once, never changed)"""

    def __init__(self):
        self.docs, self.labels, self.host, self.nfd = [], [], [], []
        self.cum = 0

    def add(self, label, doc, host=False, raw=None):
        self.docs.append(doc)
        self.labels.append(label)
        self.host.append(host)
        self.nfd.append(unicodedata.normalize("NFD", raw.decode()).encode() if raw is not None else None)
        self.cum += len(doc)

    def add_at(self, label, doc, p0, target, host, raw):
        """... behind a document of filler that puts byte p0 of `doc` at `target` (mod DEC_BLK) of the gathered text"""
        over = len(pad(1)) - 1
        m = (target - p0 - self.cum - over) % DEC_BLK or DEC_BLK
        self.add(("filler", m), pad(m))
        assert (self.cum + p0) % DEC_BLK == target % DEC_BLK
        self.add(label, doc, host, raw)

    def finish(self):
        v = vocab()
        self.text, self.offs = tm.pack_documents(self.docs)
        self.ids, self.toff, miss = v.tokenize_packed(self.text, self.offs)
        assert int(miss.sum()) == 0
        self.expect = []
        for k in range(len(self.docs)):
            dec = v.decoder()
            self.expect.append(dec.decode(self.ids[int(self.toff[k]):int(self.toff[k + 1])]) + dec.flush())
            assert self.nfd[k] is None or self.nfd[k] == self.expect[k], (self.labels[k], "the host decoder does not give NFD of the raw text back")
        return self

    def check(self, out, ooff, host_docs, what):
        assert ooff.size == len(self.docs) + 1
        bad = [(self.labels[k], len(e)) for k, e in enumerate(self.expect) if out[int(ooff[k]):int(ooff[k + 1])].tobytes() != e]
        assert not bad, "%s: %d documents differ from the host decoder; first (construct, shape, seam, first byte): %s" % (what, len(bad), bad[:6])
        assert host_docs == sum(self.host), "%s: %d documents were left to the host decoder, the table says %d" % (what, host_docs, sum(self.host))


def sweep(seam):
    if ("sweep", seam) not in _made:
        b = Batch()
        for name, per, raws, host, nfd, _ in constructs():
            for shape in (("short", "long") if seam in (STORE, CHUNK, DEC_BLK) else ("long",)):
                doc, p0, n = per[shape]
                for first in range(seam - n - 1, seam + 2):
                    b.add_at((name, shape, seam, first), doc, p0, first, host, raws[shape] if raws and nfd else None)
        _made[("sweep", seam)] = b.finish()
    return _made[("sweep", seam)]


def host_decode(doc):
    """normalized text -> what the host streaming decoder makes of its ids"""
    v = vocab()
    ids, miss = v.tokenize_normalized(doc)
    assert miss == 0
    dec = v.decoder()
    return dec.decode(ids) + dec.flush()


def classes():
    """every construct - the raw ones and the marker forms of DEC_EXTRA - once in a document of each length of LENGTHS, in gathered and in decoded
    bytes, behind a thousand bytes of the document's own: it straddles a block, and the state is carried over the 4 to 16 blocks behind it"""
    if "classes" not in _made:
        b = Batch()
        for j, (name, per, raws, host, nfd, data) in enumerate(constructs()):
            for L in LENGTHS:
                if EMULATED and (L >= DEC_LONG - 1 and j % 8):
                    continue
                for unit in ("gathered", "decoded"):
                    head = b"x" * (1000 + j % 48) + b"."
                    if data is not None:      # a raw construct: the host normalizer's text of the raw document
                        def make(k):
                            return norm(head + data + b" " + b"y" * k)
                    else:                     # a marker form: already normalized text, between normalized filler
                        form = per["short"][0][per["short"][1]:len(per["short"][0]) - len(SUFFIX["short"])]
                        def make(k, form=form):
                            return norm(head) + form + b" " + b"y" * k
                    measure = make(1) if unit == "gathered" else host_decode(make(1))
                    doc = make(1 + L - len(measure))
                    got = len(doc) if unit == "gathered" else len(host_decode(doc))
                    assert got == L, (name, L, unit, got)
                    raw = head + data + b" " + b"y" * (1 + L - len(measure)) if data is not None and nfd else None
                    b.add((name, unit, L, len(head)), doc, host, raw)
        assert {lb[0] for lb in b.labels} == {c.name for c in B.CONSTRUCTS} | {name for name, _, _ in DEC_EXTRA}
        _made["classes"] = b.finish()
    return _made["classes"]


@pytest.mark.gpu
@pytest.mark.parametrize("seam", SEAMS)
def test_every_construct_across_a_seam_of_the_decoder(seam):
    kernel_constants()
    t0 = time.time()
    b = sweep(seam)
    t1 = time.time()
    out, ooff = vocab().decode_packed(b.ids, b.toff)
    hd = N.lib.tm_decode_host_docs()
    print("seam %d: %d documents, %d gathered bytes, %d expected on the host; references %.2f s, device %.2f s" % (seam, len(b.docs), b.text.size, sum(b.host), t1 - t0, time.time() - t1))
    b.check(out, ooff, hd, "seam %d" % seam)


@pytest.mark.gpu
def test_every_construct_in_every_length_class():
    kernel_constants()
    t0 = time.time()
    b = classes()
    t1 = time.time()
    out, ooff = vocab().decode_packed(b.ids, b.toff)
    hd = N.lib.tm_decode_host_docs()
    print("length classes: %d documents, %d gathered bytes, %d expected on the host; references %.2f s, device %.2f s" % (len(b.docs), b.text.size, sum(b.host), t1 - t0, time.time() - t1))
    lens = {int(b.offs[k + 1] - b.offs[k]) for k in range(len(b.docs))}
    assert set(LENGTHS) <= lens
    b.check(out, ooff, hd, "length classes")


@pytest.mark.gpu
def test_resident_decode_of_the_whole_set():
    """tm_batch_decode on the ids a batch holds: every sweep and the length classes in ONE pass, the documents in the same places of the gathered text"""
    kernel_constants()
    v = vocab()
    parts = [sweep(s) for s in SEAMS] + [classes()]
    docs, expect, host = [], [], 0
    for p in parts:      # every part begins on a block of the gathered text, as it did alone: a document of filler in front of it
        m = (-sum(len(d) for d in docs) - (len(pad(1)) - 1)) % DEC_BLK or DEC_BLK
        docs += [pad(m)] + p.docs
        expect += [(("filler", m), b"x" * m)] + list(zip(p.labels, p.expect))
        host += sum(p.host)
        assert (sum(len(d) for d in docs) - p.cum) % DEC_BLK == 0
    text, offs = tm.pack_documents(docs)
    nd = len(docs)
    t0 = time.time()
    bh = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, int(text.size + 4096), nd, C.byref(bh)))
    try:
        N.check(N.lib.tm_batch_upload(bh, N.ptr(text), N.ptr(offs), nd))
        N.check(N.lib.tm_batch_run(bh, None))
        nbytes, host_docs = C.c_uint64(), C.c_uint32()
        N.check(N.lib.tm_batch_decode(bh, 0, None, C.byref(nbytes), C.byref(host_docs)))
        ooff = np.zeros(nd + 1, dtype=np.uint64)
        out = np.empty(int(text.size + 64), dtype=np.uint8)
        N.check(N.lib.tm_batch_decoded_download(bh, N.ptr(out), out.size, N.ptr(ooff)))
    finally:
        N.lib.tm_batch_free(bh)
    print("resident: %d documents, %d gathered bytes; device %.2f s" % (nd, text.size, time.time() - t0))
    bad = [(label, len(e)) for j, (label, e) in enumerate(expect) if out[int(ooff[j]):int(ooff[j + 1])].tobytes() != e]
    assert not bad, "resident: %d documents differ from the host decoder; first: %s" % (len(bad), bad[:6])
    assert host_docs.value == host, "resident: %d documents were left to the host decoder, the table says %d" % (host_docs.value, host)

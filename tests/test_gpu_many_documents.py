"""-m gpu: the document-count axis - batches of thousands to a million TINY documents, every output of every document compared.  What is indexed
or scanned by the number of documents changes form with it: k_doc_nseg, the binary searches of k_segments, DocCursor and the window rows,
k_dec_doc_tile and k_dec_gather's document loop, k_doc_events, the normalizer's piece counts, and scan_u32 with its three code paths
(tokenmonster_amd/csrc/tm_kernels.hip).  The counts below are where scan_u32 changes form.

Expected values: a pool of about a dozen distinct documents - the empty one (drawn most often), documents of 1 to 7 bytes, a byte the
vocabulary lacks, capcode markers, one of about 300 bytes (two segments among the tiny ones) - is tokenized ONCE per entry by the oracle
(spans: tests/span_recipe.py, raw spans: tests/origin_recipe.py, capcode-decoded text: the host's streaming decoder); a batch is a seeded
draw from the pool and everything expected of it follows by numpy indexing.  No sampling: every id, offset, count, byte and pair is compared.
tests/test_many_documents_emulated.py runs this file (less the million-document sizes) on the emulated device (tools/emu), without a GPU."""
import ctypes as C

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth
from tokenmonster_amd.vocab import PinnedBuffer
from conftest import EMULATED, fuzz_text, fuzz_vocab_tokens
from oracle_bind import Oracle
from span_recipe import oracle_spans
import origin_recipe
from test_gpu_collate import Collate, Out, DT, np_collate, np_pack
from test_gpu_windows import np_windows

pytestmark = pytest.mark.gpu

# tokenmonster_amd/csrc/tm_pipeline.h, tm_kernels.hip (scan_u32)
SCAN_CH = 4096                       # elements per block of the three-phase scan; the one-past-the-end total takes the last slot of a block or a block of its own
SCAN1_MAX = 1 << 14                  # up to here k_scan_single, above it the three-phase form
SCAN_SUMS_TRIP = 256 * SCAN_CH       # from here on k_scan_sums makes a second trip of its loop (more than 256 blocks)
COUNTS = [SCAN_CH - 1, SCAN_CH, SCAN_CH + 1, SCAN1_MAX - 1, SCAN1_MAX, SCAN1_MAX + 1, 5 * SCAN_CH - 1, 5 * SCAN_CH]
MILLION = [SCAN_SUMS_TRIP - 1, SCAN_SUMS_TRIP]
assert COUNTS == [4095, 4096, 4097, 16383, 16384, 16385, 20479, 20480] and MILLION == [1048575, 1048576]
DEC_TILE = 2048                      # ids of a tile of the decoder (tm_decode.hip)
EMPTY_RUN = 40
# count -> (the first document is empty, the last document is not - else the batch ends in a run of empty ones): the multiples of 256 end in a
# document (the grid of k_dec_doc_tile covers ndocs + 1 entries)
FORMS = {4095: (True, False), 4096: (True, True), 4097: (False, True), 16383: (False, False), 16384: (False, True), 16385: (True, False),
         20479: (True, True), 20480: (False, True), 1048575: (False, False), 1048576: (True, True)}
NONE = N.TM_NONE


def gather(flat, poff, idx):
    """the ragged rows idx of (flat, poff) one behind the other -> (flat', offsets u64, index of every element in flat)"""
    poff = poff.astype(np.int64)
    lens = (poff[1:] - poff[:-1])[idx]
    off = np.zeros(idx.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    src = np.repeat(poff[:-1][idx] - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]), dtype=np.int64)
    return flat[src], off, src


def ragged(rows, dtype):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    flat = np.concatenate([np.asarray(r, dtype=dtype).reshape(-1) for r in rows]) if rows else np.zeros(0, dtype)
    return flat.astype(dtype), off


class Pool:
    """the distinct documents of one vocabulary and what the oracle says about each"""

    def __init__(self, v, orc, docs, weights, raw):
        self.v, self.orc, self.docs, self.raw = v, orc, docs, raw
        self.weights = np.asarray(weights, dtype=np.float64) / sum(weights)
        self.long = max(range(len(docs)), key=lambda k: len(docs[k]))
        assert docs[0] == b"" and len(docs[self.long]) > 256
        has_unk = v.unk_token_id() is not None
        norm = [v.normalize(d) for d in docs] if raw else docs
        tok = [orc.tokenize(d) for d in norm]
        ids = [t[0] for t in tok]
        self.one = next(k for k, x in enumerate(ids) if len(x) == 1)            # a document of exactly one id
        self.text, self.text_off = ragged([np.frombuffer(d, dtype=np.uint8) for d in docs], np.uint8)
        self.ids, self.ids_off = ragged(ids, np.uint32)
        self.nids = np.array([len(x) for x in ids], dtype=np.int64)
        self.missing = np.array([t[1] for t in tok], dtype=np.uint32)
        cnt = [orc.count(d) for d in norm]
        self.count = np.array([c[0] for c in cnt], dtype=np.uint64)
        self.count_missing = np.array([c[1] for c in cnt], dtype=np.uint32)
        spans = [oracle_spans(orc, d, has_unk) for d in norm]
        assert all(len(s) == len(x) for s, x in zip(spans, ids))
        if raw:
            mapped = []
            for d, nd, s in zip(docs, norm, spans):
                nb, own = origin_recipe.normalize_with_owners(d, v.capcode(), v.normalization_code())
                assert nb == nd, d
                mapped.append(origin_recipe.raw_spans(s, own, len(d)))
            spans = mapped
        self.spans = np.concatenate(spans).astype(np.uint32).reshape(-1, 2)
        self.dec_raw, self.dec_raw_off = ragged([np.frombuffer(orc.decode_raw(x), dtype=np.uint8) for x in ids], np.uint8)
        dec = []
        for x in ids:
            d = v.decoder()
            dec.append(np.frombuffer(d.decode(x) + d.flush(), dtype=np.uint8))
        self.dec, self.dec_off = ragged(dec, np.uint8)
        assert self.missing.any() and any(len(norm[k]) > 256 for k in range(len(docs)))

    def draw(self, count, seed, first_empty, last_doc, empty=None):
        """-> pool index of every document.  first_empty: document 0 is the empty one, else it is not; last_doc: the batch ends in the
        long document, placed so that its ids straddle two tiles of the decoder - else in a run of empty documents behind a document
        that is not.  empty: the share of empty documents (None: the pool's weights)"""
        rng = np.random.default_rng(seed)
        w = self.weights
        if empty is not None:
            w = np.append(empty, w[1:] / w[1:].sum() * (1 - empty))
        idx = rng.choice(len(self.docs), size=count, p=w)
        idx[0] = 0 if first_empty else 3
        if last_doc:
            idx[-1] = self.long
            # ids in front of the last document: a multiple of the tile less half of that document's ids, by turning empty documents into one-id ones
            before = int(self.nids[idx[:-1]].sum())
            want = (-(before + int(self.nids[self.long]) // 2)) % DEC_TILE
            free = np.nonzero(idx[1:-1] == 0)[0] + 1
            assert free.size >= want
            idx[free[:want]] = self.one
            before = int(self.nids[idx[:-1]].sum())
            assert before // DEC_TILE != (before + int(self.nids[self.long])) // DEC_TILE
        else:
            idx[-EMPTY_RUN:] = 0
            idx[-EMPTY_RUN - 1] = self.long
        return idx


class Batch:
    """a draw and everything expected of it"""

    def __init__(self, pool, idx):
        p = self.pool = pool
        self.idx, self.nd = idx, int(idx.size)
        self.text, self.offs, _ = gather(p.text, p.text_off, idx)
        self.ids, self.toff, src = gather(p.ids, p.ids_off, idx)
        self.spans = p.spans[src]
        self.missing, self.count, self.count_missing = p.missing[idx], p.count[idx], p.count_missing[idx]
        self.dec_raw, self.dec_raw_off, _ = gather(p.dec_raw, p.dec_raw_off, idx)
        self.dec, self.dec_off, _ = gather(p.dec, p.dec_off, idx)
        for a in (self.text, self.offs, self.ids, self.toff, self.spans, self.missing, self.count, self.count_missing, self.dec_raw, self.dec_raw_off, self.dec, self.dec_off):
            a.setflags(write=False)
        self.text = np.ascontiguousarray(self.text)

    def docs(self):
        """the documents' expected ids as a list of arrays (what np_collate / np_pack / np_windows take)"""
        off = self.pool.ids_off
        rows = [self.pool.ids[off[k]:off[k + 1]] for k in range(len(self.pool.docs))]
        return [rows[k] for k in self.idx]


class Env:
    def __init__(self):
        rng = np.random.default_rng(440_001)
        # normalized text, capcode 2 with an unk token: a byte without a token is an id and a missing count
        img = synth.build_vocab(fuzz_vocab_tokens(rng, 2, 200), capcode=2, charset=1, with_unk=True)
        self.v, self.orc = tm.Vocab(img), Oracle(img)
        long_doc = fuzz_text(rng, 2, 300)
        docs = [b"", b"a", b" b", b"abc", b" abc", b"ab cd", b" a.b,c", b"abcde 1", b"x", b"ay\xffb", b"D abc", b"W abc de", b"C a", long_doc]
        self.norm = Pool(self.v, self.orc, docs, [40, 6, 5, 5, 5, 4, 4, 4, 3, 3, 3, 3, 3, 1], raw=False)
        # raw text, capcode 2 / NFD (tests/fuzz_cases.py: one_raw): capitals and an accented letter in the pool
        toks = sorted(set(fuzz_vocab_tokens(rng, 2, 300)) | {"\u0301".encode(), "\u00e9".encode(), b"C", b"W", b"D", b"Ca", b"W x", b" the", b"ing ", b"D a", b"t", b"h"})
        rimg = synth.build_vocab(toks, capcode=2, charset=1, norm_flag=1, with_unk=True)
        self.rv, self.rorc = tm.Vocab(rimg), Oracle(rimg)
        words = ["the", "The", "THE", "a", "I", "I'm", "caf\u00e9", "\u00c9cole", "HTTPServer", "x1", "42", "abc", "Bad", "dEb", "q"]
        long_raw = b""
        while len(long_raw) < 300:
            long_raw += str(rng.choice(words)).encode() + b" "
        rdocs = [b"", b"a", b"A", b"ab", b"The", b" cab", b"I'm a", "caf\u00e9".encode(), "\u00c9a".encode(), b"ABC de", b"q", b"x1 42", b"Ab Cd.", long_raw]
        self.raw = Pool(self.rv, self.rorc, rdocs, [40, 6, 5, 5, 5, 4, 4, 4, 3, 3, 3, 3, 3, 1], raw=True)
        n_ids = max(self.v.n_ids(), self.rv.n_ids())
        self.pad, self.bos, self.eos = n_ids + 5, n_ids + 6, n_ids + 7
        self._batches = {}
        self._runs = {}

    def batch(self, count, raw=False):
        """the draw of `count` documents in its form (FORMS), kept for the count being tested"""
        key = (count, raw)
        if key not in self._batches:
            for k in [k for k in self._batches if k[0] != count]:
                del self._batches[k]
            for k in [k for k in self._runs if k != count]:
                N.lib.tm_batch_free(self._runs.pop(k))
            pool = self.raw if raw else self.norm
            self._batches[key] = Batch(pool, pool.draw(count, 9_000 + count, *FORMS[count], 0.999 if count >= MILLION[0] else None))
        return self._batches[key]

    def run(self, count):
        """one tm_batch per count that holds the run of the normalized batch: collate, pack and the windows read it"""
        if count not in self._runs:
            bt = self.batch(count)
            b = C.c_void_p()
            N.check(N.lib.tm_batch_create(self.v.handle, max(int(bt.text.size), 1024), bt.nd, C.byref(b)))
            N.check(N.lib.tm_batch_upload(b, N.ptr(bt.text), N.ptr(bt.offs), bt.nd))
            N.check(N.lib.tm_batch_run(b, None))
            self._runs[count] = b
        return self._runs[count]


_env = None


@pytest.fixture(scope="module")
def env():
    global _env
    if _env is None:
        _env = Env()
    return _env


def test_the_draws_cover_both_ends(env):
    firsts, lasts = set(), set()
    for count in COUNTS + MILLION:
        idx = env.norm.draw(count, 9_000 + count, *FORMS[count], 0.999 if count >= MILLION[0] else None)
        firsts.add(bool(idx[0] == 0))
        lasts.add(bool(idx[-1] == 0))
        assert (idx[-EMPTY_RUN:] == 0).all() or idx[-1] == env.norm.long
        assert (idx == 0).mean() > (0.99 if count >= MILLION[0] else 0.2) and len(set(idx.tolist())) == len(env.norm.docs)
    assert firsts == {True, False} and lasts == {True, False}


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, "%s: shape %s != %s" % (what, got.shape, exp.shape)
    bad = np.nonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))[0] if got.size else np.zeros(0, np.int64)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: %s != %s" % (what, bad.size, got.shape[0], bad[0], got[bad[0]], exp[bad[0]])


def check_tokenize(v, bt):
    ids, toff, missing = v.tokenize_packed(bt.text, bt.offs)
    same(toff, bt.toff, "id offsets")
    same(ids, bt.ids, "ids")
    same(missing, bt.missing, "missing")


def check_count(v, bt):
    counts, cmiss = v.count_packed(bt.text, bt.offs)
    same(counts, bt.count, "counts")
    same(cmiss, bt.count_missing, "missing of the count")


def ids_of(blob, enc, n):
    w = np.zeros((n, 4), dtype=np.uint8)
    w[:, :enc] = np.asarray(blob[: n * enc]).reshape(n, enc)
    return w.view(np.uint32).ravel()


# ---- up to 20 480 documents: every path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_tokenize_and_count(env, count):
    bt = env.batch(count)
    check_tokenize(env.v, bt)
    check_count(env.v, bt)


@pytest.mark.parametrize("count", COUNTS)
def test_serialized(env, count):
    bt = env.batch(count)
    for width in (2, 4):
        blob, boff, missing, enc = env.v.tokenize_serialized_packed(bt.text, bt.offs, encoding_length=width)
        assert enc == width
        same(boff, bt.toff * np.uint64(width), "byte offsets at width %d" % width)
        same(ids_of(blob, enc, bt.ids.size), bt.ids, "ids at width %d" % width)
        same(missing, bt.missing, "missing")


@pytest.mark.parametrize("count", COUNTS)
def test_spans(env, count):
    bt = env.batch(count)
    ids, toff, spans, missing = env.v.tokenize_spans_packed(bt.text, bt.offs)
    same(toff, bt.toff, "id offsets")
    same(ids, bt.ids, "ids")
    same(spans, bt.spans, "spans")
    same(missing, bt.missing, "missing")


@pytest.mark.parametrize("count", COUNTS)
def test_raw_text_and_raw_spans(env, count):
    """tm_batch_upload_raw + tm_batch_normalize + tm_batch_run + tm_batch_raw_spans: the normalizer's pieces per document and the owners"""
    bt = env.batch(count, raw=True)
    ids, toff, spans, _ = env.rv.tokenize_raw_spans_packed(bt.text, bt.offs)
    same(toff, bt.toff, "id offsets")
    same(ids, bt.ids, "ids")
    same(spans, bt.spans, "raw spans")


@pytest.mark.parametrize("count", COUNTS)
def test_decode(env, count):
    bt = env.batch(count)
    for raw, exp, exp_off in ((True, bt.dec_raw, bt.dec_raw_off), (False, bt.dec, bt.dec_off)):
        out, ooff = env.v.decode_packed(bt.ids, bt.toff, raw=raw)
        same(ooff, exp_off, "text offsets (raw %d)" % raw)
        same(out, exp, "text (raw %d)" % raw)


@pytest.mark.parametrize("count", COUNTS)
def test_pipeline_lanes_and_ring(env, count):
    """tm_tokenize_pipeline of raw text: the lanes (pageable buffers) with chunks of thousands of documents, the ring (page-locked buffers)"""
    bt = env.batch(count, raw=True)
    chunk = max(4096, int(bt.text.size) // 4)
    blob, boff, missing, enc, st = env.rv.tokenize_pipeline(bt.text, bt.offs, raw=True, chunk_bytes=chunk, lanes=2)
    assert st["ring"] == 0 and 1 < st["chunks"] <= bt.nd // 500, st
    same(boff, bt.toff * np.uint64(enc), "byte offsets (lanes)")
    same(ids_of(blob, enc, bt.ids.size), bt.ids, "ids (lanes)")
    same(missing, bt.missing, "missing (lanes)")
    pin, pout = PinnedBuffer(max(int(bt.text.size), 16)), PinnedBuffer(4 * bt.ids.size + 64)
    pin.array[: bt.text.size] = bt.text
    blob, boff, missing, enc, st = env.rv.tokenize_pipeline(pin.array[: bt.text.size], bt.offs, raw=True, chunk_bytes=chunk, lanes=2, out=pout.array)
    assert st["ring"] == 1 and st["chunks"] > 1, st
    same(boff, bt.toff * np.uint64(enc), "byte offsets (ring)")
    same(ids_of(blob, enc, bt.ids.size), bt.ids, "ids (ring)")
    same(missing, bt.missing, "missing (ring)")


def sync(b):
    N.check(N.lib.tm_batch_totals(b, None, None))


@pytest.mark.parametrize("count", COUNTS)
def test_collate_and_pack(env, count):
    bt, b, L = env.batch(count), env.run(count), 8
    docs = bt.docs()
    for id_bytes in (2, 4):
        e_ids, e_mask, e_lens = np_collate(docs, L, env.pad, env.bos, env.eos, 0, DT[id_bytes])
        how = Collate(0, bt.nd, L, id_bytes, env.pad, env.bos, env.eos, 0)
        ids, mask, lens = Out(bt.nd * L, id_bytes), Out(bt.nd * L, 1), Out(bt.nd, 4)
        N.check(N.lib.tm_batch_collate(b, C.byref(how), None, ids.ptr, mask.ptr, lens.ptr))
        sync(b)
        same(ids.view(DT[id_bytes]).reshape(bt.nd, L), e_ids, "rows of %d-byte ids" % id_bytes)
        same(mask.view(np.uint8).reshape(bt.nd, L), e_mask, "mask")
        same(lens.view(np.uint32), e_lens, "lengths")
        assert ids.sentinels_intact() and mask.sentinels_intact() and lens.sentinels_intact()
    for id_bytes, eos in ((2, env.eos), (4, None)):
        e_ids, e_di, e_po, stream_len = np_pack(docs, L, env.pad, eos, DT[id_bytes])
        how = Collate(0, bt.nd, L, id_bytes, env.pad, NONE, NONE if eos is None else eos, 0)
        need = C.c_uint64()
        N.check(N.lib.tm_batch_pack_rows(b, C.byref(how), C.byref(need)))
        assert need.value == e_ids.shape[0] == (stream_len + L - 1) // L
        rows = int(need.value)
        ids, di, po = Out(rows * L, id_bytes), Out(rows * L, 4), Out(rows * L, 4)
        N.check(N.lib.tm_batch_pack(b, C.byref(how), None, rows, ids.ptr, di.ptr, po.ptr))
        sync(b)
        same(ids.view(DT[id_bytes]).reshape(rows, L), e_ids, "packed rows of %d-byte ids" % id_bytes)
        same(di.view(np.uint32).reshape(rows, L), e_di, "document of every position")
        same(po.view(np.uint32).reshape(rows, L), e_po, "position inside the document")
        assert ids.sentinels_intact() and di.sentinels_intact() and po.sentinels_intact()


@pytest.mark.parametrize("count", COUNTS)
def test_windows(env, count):
    """tm_batch_window_rows / tm_batch_windows: every document is at least a row, the long ones many (room 3, overlap 1)"""
    bt, b, L, overlap = env.batch(count), env.run(count), 4, 1
    e_ids, e_mask, e_lens, e_doc, e_start, _ = np_windows(bt.docs(), L, env.pad, env.bos, None, overlap, False)
    rows = e_ids.shape[0]
    assert rows > bt.nd and (rows > SCAN1_MAX or count < SCAN1_MAX)
    how = Collate(0, bt.nd, L, 4, env.pad, env.bos, NONE, 0)
    need = C.c_uint64(12345)
    N.check(N.lib.tm_batch_window_rows(b, C.byref(how), overlap, C.byref(need)))
    assert need.value == rows
    o = [Out(rows * L, 4), Out(rows * L, 1), Out(rows, 4), Out(rows, 4), Out(rows, 4)]
    N.check(N.lib.tm_batch_windows(b, C.byref(how), overlap, None, rows, *[x.ptr for x in o]))
    sync(b)
    same(o[0].view(np.uint32).reshape(rows, L), e_ids, "window rows")
    same(o[1].view(np.uint8).reshape(rows, L), e_mask, "mask")
    for x, e, what in zip(o[2:], (e_lens, e_doc, e_start), ("lengths", "document of every row", "start of every row")):
        same(x.view(np.uint32), e, what)
    assert all(x.sentinels_intact() for x in o)


# ---- a million documents, 99.9 % of them empty ------------------------------------------------------------------------------------------------
big = pytest.mark.skipif(EMULATED, reason="a million documents through the emulated device take minutes")


@big
@pytest.mark.parametrize("count", MILLION)
def test_a_million_documents_tokenize_count_decode(env, count):
    bt = env.batch(count)
    assert bt.nd == count
    check_tokenize(env.v, bt)
    check_count(env.v, bt)
    out, ooff = env.v.decode_packed(bt.ids, bt.toff, raw=True)
    same(ooff, bt.dec_raw_off, "text offsets")
    same(out, bt.dec_raw, "text")


@big
@pytest.mark.parametrize("count", MILLION)
def test_a_million_raw_documents(env, count):
    bt = env.batch(count, raw=True)
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(env.rv.handle, int(bt.text.size) * 4 + 16 * bt.nd + 1024, bt.nd, C.byref(b)))
    try:
        N.check(N.lib.tm_batch_upload_raw(b, N.ptr(bt.text), N.ptr(bt.offs), bt.nd))
        N.check(N.lib.tm_batch_normalize(b, None))
        N.check(N.lib.tm_batch_run(b, None))
        n = C.c_uint64()
        N.check(N.lib.tm_batch_totals(b, C.byref(n), None))
        assert n.value == bt.ids.size
        ids, toff, missing = np.zeros(max(n.value, 1), dtype=np.uint32), np.zeros(bt.nd + 1, dtype=np.uint64), np.zeros(bt.nd, dtype=np.uint32)
        N.check(N.lib.tm_batch_download(b, N.ptr(ids), n.value, N.ptr(toff), N.ptr(missing)))
        same(toff, bt.toff, "id offsets")
        same(ids[: n.value], bt.ids, "ids")
        same(missing, bt.missing, "missing")
    finally:
        N.lib.tm_batch_free(b)


@big
@pytest.mark.parametrize("count", MILLION)
def test_a_million_documents_window_rows(env, count):
    """tm_batch_window_rows and the document of every row (tm_batch_windows), the rule of include/tokenmonster_hip.h in numpy"""
    bt, b, L, overlap = env.batch(count), env.run(count), 4, 1
    room, step = L - 1, L - 1 - overlap
    n = (bt.toff[1:] - bt.toff[:-1]).astype(np.int64)
    w = np.where(n <= room, 1, 1 + -(-(n - room) // step))
    rows = int(w.sum())
    first = np.cumsum(w) - w
    e_doc = np.repeat(np.arange(bt.nd, dtype=np.int64), w)
    e_start = (np.arange(rows, dtype=np.int64) - first[e_doc]) * step
    e_lens = np.minimum(n[e_doc] - e_start, room) + 1
    how = Collate(0, bt.nd, L, 4, env.pad, env.bos, NONE, 0)
    need = C.c_uint64(12345)
    N.check(N.lib.tm_batch_window_rows(b, C.byref(how), overlap, C.byref(need)))
    assert need.value == rows > count
    o = [Out(rows * L, 4), Out(rows, 4), Out(rows, 4), Out(rows, 4)]
    N.check(N.lib.tm_batch_windows(b, C.byref(how), overlap, None, rows, o[0].ptr, None, o[1].ptr, o[2].ptr, o[3].ptr))
    sync(b)
    for x, e, what in zip(o[1:], (e_lens, e_doc, e_start), ("lengths", "document of every row", "start of every row")):
        same(x.view(np.uint32), e, what)
    # the ids of every row: the bos, then the document's ids from the row's start
    got = o[0].view(np.uint32).reshape(rows, L)
    col = np.arange(L - 1, dtype=np.int64)[None, :]
    pos = e_start[:, None] + col
    exp = np.full((rows, L), env.pad, dtype=np.uint32)
    exp[:, 0] = env.bos
    inside = pos < n[e_doc][:, None]
    exp[:, 1:][inside] = bt.ids[(bt.toff[:-1].astype(np.int64)[e_doc][:, None] + pos)[inside]]
    same(got, exp, "window rows")
    assert all(x.sentinels_intact() for x in o)

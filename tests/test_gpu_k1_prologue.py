"""-m gpu: the prologue of k_match_branch.  A wavefront learns everything about its segment from ONE 16-byte record (k_seg_fill: where its
text begins, how far it may look, how many positions it owns, whether the next segment is its document's, whether text follows) and asks
for all of its text at once.  These tests put every field of the record at its edges, on both places the text can lie in: document
lengths around the segment size, the halo (NPOS = 296) and the staged text (352 bytes) at each of the four wavefront places of a
workgroup, last segments of a batch that are full and one byte long, text staged from the normalizer's slabs with words across the end of
a piece at every alignment, byte ranges of one scoring walk that see the text behind them, and a host-to-host call whose segment count
only the device knows.  ids and missing counts per document against the oracle (and the reference's own runtime where it has been
built); histograms against Oracle.score_mt."""
import ctypes as C

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N, synth
from conftest import fuzz_text, fuzz_vocab_tokens
from oracle_bind import Oracle, Reference, have_ref

SEG, WAVES, PIECE, TEXT_LEN = 256, 4, 1024, 352
LENGTHS = [0, 1, 2, 255, 256, 257, 295, 296, 297, 511, 512, 513, 1023, 1024, 1025]

_cases = {}


def micro(capcode):
    """a micro vocabulary (tests/conftest.py), its oracle and - where built - the reference runtime: made once per capcode mode"""
    if capcode not in _cases:
        rng = np.random.default_rng(9100 + capcode)
        img = synth.build_vocab(fuzz_vocab_tokens(rng, capcode, 160), capcode=capcode, charset=1, with_unk=True)
        _cases[capcode] = (tm.Vocab(img), Oracle(img), Reference(img) if have_ref() else None)
    return _cases[capcode]


def check_ids(orc, ref, docs, ids, toff, missing, what):
    assert toff[0] == 0 and toff[-1] == ids.size
    for d, doc in enumerate(docs):
        got = ids[int(toff[d]):int(toff[d + 1])]
        exp, miss = orc.tokenize(doc)
        assert got.size == exp.size and (got == exp).all(), "%s doc %d (%d bytes): ids differ from the oracle's" % (what, d, len(doc))
        assert int(missing[d]) == miss, "%s doc %d: missing %d != %d" % (what, d, int(missing[d]), miss)
        if ref is not None:
            rexp, _ = ref.tokenize_normalized(doc)
            assert got.size == rexp.size and (got == rexp).all(), "%s doc %d (%d bytes): ids differ from the reference's" % (what, d, len(doc))


def shuffled_lengths(last):
    """LENGTHS in shuffled order (fixed seed), as many rounds as it takes until the FIRST and the LAST segment of a document of every length
    have sat at each of the four wavefront places of a workgroup; then one more document of `last` bytes, which ends the batch"""
    rng = np.random.default_rng(9201)
    want = {(n, place, end) for n in LENGTHS if n for place in range(WAVES) for end in (0, 1)}
    order, seen, g = [], set(), 0
    for _ in range(64):
        for n in rng.permutation(LENGTHS):
            n = int(n)
            nseg = (n + SEG - 1) // SEG
            if nseg:
                seen.add((n, g % WAVES, 0))
                seen.add((n, (g + nseg - 1) % WAVES, 1))
            g += nseg
            order.append(n)
        if seen >= want:
            break
    assert seen >= want, sorted(want - seen)
    return order + [last]


@pytest.mark.gpu
@pytest.mark.parametrize("capcode", [0, 2])
@pytest.mark.parametrize("last", [SEG, 2 * SEG + 1])
def test_document_lengths_at_every_wavefront_place(capcode, last):
    """packed text (tm_batch_upload of host-normalized text, here through tm_tokenize_batch): the record's look-ahead below NPOS, below
    NPOS + the longest token and above; its segment length; the same-document bit at document ends and at the edge of a workgroup; the last
    segment of the batch a full one (last = 256) and a one-byte one (last = 513)"""
    v, orc, ref = micro(capcode)
    rng = np.random.default_rng(9300 + capcode)
    lens = shuffled_lengths(last)
    assert (lens[-1] - 1) % SEG + 1 == (SEG if last == SEG else 1)
    docs = [fuzz_text(rng, capcode, n)[:n] for n in lens]
    text, offs = tm.pack_documents(docs)
    ids, toff, missing = v.tokenize_packed(text, offs)
    check_ids(orc, ref, docs, ids, toff, missing, "packed, last segment of %d bytes" % ((last - 1) % SEG + 1))


def raw_documents(rng):
    """ASCII documents of several 1 KiB pieces for the device normalizer: a blank, then lower-case words, `caps` of those in the first piece
    with a capital first letter.  Such a capital becomes a marker and its small letter - one byte more -, so the first piece's normalized
    bytes end `caps` bytes behind a multiple of 256 (the test checks where, with the host normalizer)."""
    docs = []
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"a", b"lazy", b"dog", b"and", b"on"]
    for caps in (0, 1, 2, 3, 5, 6, 7, 33, 94, 97):
        body = bytearray(b" ")
        while len(body) < 4 * PIECE + 300:
            body += words[int(rng.integers(len(words)))] + b" "
        body = body[: 4 * PIECE + 300 + caps]
        at = [i for i in range(8, PIECE - 8) if body[i - 1] == 32 and 97 <= body[i] <= 122 and 97 <= body[i + 1] <= 122]
        for i in rng.choice(at, size=caps, replace=False):
            body[int(i)] -= 32
        docs.append(bytes(body))
    return docs


@pytest.mark.gpu
def test_text_staged_from_the_normalizer_slabs():
    """the slab path (tm_batch_upload_raw + tm_batch_normalize leave the normalized text in one slab per 1 KiB piece of raw text; ASCII text
    keeps it there: every document is normalized on the device and no piece is short): segments that begin 1, 2 and 3 bytes in front of
    the end of a piece, words of both halves of a lane's text across that end, segments whose 352 bytes lie in two slabs.  Also with
    the text packed first (test hook 11)."""
    rng = np.random.default_rng(9401)
    toks = sorted(set(fuzz_vocab_tokens(rng, 2, 200)) | {b"C", b"W", b"D", b" the", b"C q", b" qu", b"ick", b" a", b"og ", b"D a", b"Cb", b" C", b"o", b"v", b"r"})
    img = synth.build_vocab(toks, capcode=2, charset=1, norm_flag=1, with_unk=True)
    v, orc, ref = tm.Vocab(img), Oracle(img), (Reference(img) if have_ref() else None)
    docs = raw_documents(rng)
    norm = [v.normalize(d) for d in docs]
    # where the pieces end in the normalized text, from the host normalizer; which cases the segments (every 256 bytes) meet
    first_word, second_word, begins_before, two_slabs = set(), set(), set(), 0
    for d, n in zip(docs, norm):
        for cut in range(PIECE, len(d), PIECE):
            head = v.normalize(d[:cut])
            assert bytes(n[: len(head)]) == bytes(head), "the normalized text of a document's first pieces is not a prefix of the document's"
            end = len(head)
            for begin in range(0, len(n), SEG):
                k = end - begin                     # bytes of the segment's text in the piece it begins in
                if 0 < k < TEXT_LEN and begin + k < len(n):
                    two_slabs += 1
                    if k % 4:
                        (first_word if k < SEG else second_word).add(k % 4)
                    if k < 4:
                        begins_before.add(k)
    assert begins_before == {1, 2, 3} and first_word == {1, 2, 3} and second_word == {1, 2, 3} and two_slabs > 20, (begins_before, first_word, second_word, two_slabs)
    for flags in (0, 2048):
        old = N.lib.tm_debug_flags(flags)
        try:
            got = v.tokenize(docs)
        finally:
            N.lib.tm_debug_flags(old)
        for d, (g, doc) in enumerate(zip(got, norm)):
            exp, _ = orc.tokenize(doc)
            assert g.size == exp.size and (g == exp).all(), "hook %d doc %d: ids differ from the oracle's" % (flags, d)
            if ref is not None:
                rexp, _ = ref.tokenize_normalized(doc)
                assert g.size == rexp.size and (g == rexp).all(), "hook %d doc %d: ids differ from the reference's" % (flags, d)


@pytest.mark.gpu
@pytest.mark.parametrize("capcode", [0, 2])
def test_scoring_ranges_that_see_the_text_behind_them(capcode):
    """the scoring pass over byte ranges of ONE walk (tm_score_begin / tm_score_finish, tokenmonster_amd/dist.py): a range may look at the
    text behind its end (the record's look-ahead is larger than its segment, and `text follows` is set on its last segment).  Ranges that end
    on, one byte before and one byte after a multiple of 256; their histograms together == Oracle.score_mt of the whole text.  And tm_score
    over the same ranges as independent strips (nothing visible behind them) == the oracle's walk of each strip."""
    from tokenmonster_amd import dist as tmdist
    v, orc, _ = micro(capcode)
    rng = np.random.default_rng(9500 + capcode)
    data = np.frombuffer(fuzz_text(rng, capcode, 60_000)[:60_000], dtype=np.uint8)
    cuts = [0, 256, 767, 1281, 4096, 9983, 20_225, 33_024, 47_103, 59_905, 60_000]
    assert {c % SEG for c in cuts[1:-1]} == {0, 1, SEG - 1}
    exp_s, exp_t, exp_m, _ = orc.score_mt(data, 3, strip=8192, warm=512)
    all_exits, hists, handles = [], [], []
    try:
        for a, b in zip(cuts, cuts[1:]):
            own = np.ascontiguousarray(data[a:min(b + tmdist.HALO, data.size)])
            ds = C.c_void_p()
            N.check(N.lib.tm_dataset_upload(N.ptr(own), own.size, C.byref(ds)))
            handles.append(ds)
            eng = tmdist.HipRange(v, ds, b - a, continues=b < data.size, text_ends_in_halo=data.size - b < tmdist.HALO)
            all_exits.append(eng.begin())
            eng.finish(tmdist.resolve_entry(all_exits, len(all_exits) - 1))
            s_ = np.zeros(v.n_ids(), dtype=np.uint32)
            t_ = C.c_uint64()
            m_ = np.zeros(32, dtype=np.uint8)
            N.check(N.lib.tm_score_read(v.handle, ds, N.ptr(s_), C.byref(t_), N.ptr(m_)))
            hists.append((s_, t_.value, m_))
    finally:
        for ds in handles:
            N.lib.tm_dataset_free(ds)
    assert (sum(h[0].astype(np.uint64) for h in hists) == exp_s).all() and sum(h[1] for h in hists) == exp_t
    assert (np.bitwise_or.reduce(np.stack([h[2] for h in hists])) == exp_m).all()
    # independent strips
    strips = [(a, b - a) for a, b in zip(cuts, cuts[1:])]
    ds = C.c_void_p()
    N.check(N.lib.tm_dataset_upload(N.ptr(data), data.size, C.byref(ds)))
    try:
        so, sl = np.array([a for a, _ in strips], dtype=np.uint64), np.array([n for _, n in strips], dtype=np.uint64)
        got_s, got_t, got_m = np.zeros(v.n_ids(), dtype=np.uint32), C.c_uint64(), np.zeros(32, dtype=np.uint8)
        N.check(N.lib.tm_score(v.handle, ds, N.ptr(so), N.ptr(sl), len(strips), N.ptr(got_s), C.byref(got_t), N.ptr(got_m)))
    finally:
        N.lib.tm_dataset_free(ds)
    exp_s, exp_t, exp_m = np.zeros(orc.n_ids(), dtype=np.uint32), 0, np.zeros(32, dtype=np.uint8)
    for a, n in strips:
        s, t, m = orc.score(data[a:a + n])
        exp_s += s
        exp_t += t
        exp_m |= m
    assert (got_s == exp_s).all() and got_t.value == exp_t and (got_m == exp_m).all()


@pytest.mark.gpu
def test_segment_count_of_the_device():
    """tm_tokenize_pipeline on page-locked buffers: a chunk's kernels are launched over a bound and take the number of segments from the
    device (the control words of the ring), k_seg_fill and k_match_branch among them.  ids == the resident pass over the same text."""
    from conftest import EMULATED
    img = synth.synth_vocab(synth.ENGLISHCODE, 3000, capcode=2, norm_flag=1, level=3, seed=0x52494E47)
    raw, roffs = synth.synth_corpus(synth.ENGLISHCODE, 200_000 if EMULATED else 1 << 20, seed=91)
    v = tm.Vocab(img)
    docs = [raw[int(roffs[d]):int(roffs[d + 1])].tobytes() for d in range(roffs.size - 1)]
    resident = v.tokenize(docs)
    ids = np.concatenate(resident) if resident else np.zeros(0, np.uint32)
    pin = tm.PinnedBuffer(raw.size)
    pin.array[: raw.size] = raw
    pout = tm.PinnedBuffer(4 * ids.size + 64)
    blob, boff, _, enc, st = v.tokenize_pipeline(pin.array[: raw.size], roffs, raw=True, encoding_length=4, chunk_bytes=100_000, lanes=2, out=pout.array)
    assert st["ring"] == 1 and st["chunks"] > 1, st
    assert enc == 4 and int(boff[-1]) == 4 * ids.size
    assert (np.frombuffer(np.asarray(blob[: 4 * ids.size]).tobytes(), dtype="<u4") == ids).all()
    toff = np.zeros(len(docs) + 1, dtype=np.uint64)
    toff[1:] = np.cumsum([r.size for r in resident])
    assert (boff == toff * np.uint64(4)).all()

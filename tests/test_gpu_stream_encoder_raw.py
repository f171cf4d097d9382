"""-m gpu: RAW text through the streaming encoder (tm_encoder_feed_raw, Encoder.feed_raw).  One raw document fed in pieces cut anywhere -
inside a UTF-8 character, inside a run of capitals, between '\\r' and '\\n' - must give the ids and `missing` of the whole text normalized at
once and tokenized as one document.  The expectation never comes from the code under test: it is tm_tokenize_batch (tokenize_packed) of
synth.normalize(whole raw text) - the HOST normalizer - and the CPU oracle's walk over the same normalized bytes.
Where nothing else is said the vocabulary is a synthetic capcode-2 NFD one and max_piece_bytes = 4096, so that a small text takes many passes.
test_raw_on_the_emulated_device runs the split-invariance and every-cut cases on the emulated device (tools/emu) without a GPU; that run is no
evidence for the device, the -m gpu run is."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth
from conftest import fuzz_vocab_tokens
from oracle_bind import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMULATED = os.environ.get("TM_EMU") == "1"
PIECE = 4096
NFD, LOWER, ACCENTS, COLLAPSE, UNIXLINES = 1, 2, 4, 16, 128

# what the device normalizer keeps to itself: capital runs, digits, both apostrophes, accented Latin composed and with combining marks,
# Cyrillic, CJK, voiced kana, Hangul, emoji
WORDS = ["HELLO", "Hello", "hello", "A.B", "WORLD", "World", "abc", "de", "ab", "a", "I", "USA", "iPhone", "1", "23", "4567", "'", "\u2019",
         "don't", "DON'T", "it\u2019s", "IT\u2019S", "caf\xe9", "CAF\xc9", "\xe9", "\xc9cole", "nin\u0303o", "e\u0301", "E\u0301",
         "\xfc", "\xdc", "\u043f\u0440\u0438\u0432\u0435\u0442", "\u041c\u0418\u0420", "\u041c\u0438\u0440",
         "\u6f22\u5b57", "\u65e5\u672c", "\ud55c\uae00", "\uac00", "\U0001F600", "\U0001F680"]
# voiced kana: NFD splits them into a kana and a three-byte mark.  The device normalizer does that itself - except under `accents`, where the
# mark would have to go again and the piece is the host normalizer's (tm_norm.hip, norm_tables): under that flag they are no part of the
# text that must stay on the device, and get a run of their own in which only the ids are compared
KANA = ["\u304c", "\u30d1", "\u3054\u306f\u3093"]
SEPS = [" ", " ", " ", " ", "  ", ", ", ". ", "; ", "-", "/", " (", ") ", "\t", ""]
ENDS = ["\n", "\n", "\n", "\r\n", "\r\n", "\r", "\n\n", " \n"]
VOCAB_WORDS = ["hello", " hello", " world", "world", "abc", "de", "ab", " i", "usa", "phone", "caf", "e", "\u0301", "\u0303", "\u0308", "n", "o",
               "\u043f\u0440\u0438", "\u0432\u0435\u0442", "\u043c\u0438\u0440", "\u6f22", "\u5b57", "\u304b", "\u3099", "\u1112", "\u1161", "\u11ab",
               "\n", "\r", "\r\n", "\t", "1", "2", "3", "4", "23", "'", "\u2019", "don", "t", "it", "s", ".", ",", ";", "-", "/", "(", ")", " ", "  "]


def raw_text(seed, n, words=None):
    words = words or WORDS + KANA
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        line = "".join(words[int(rng.integers(len(words)))] + SEPS[int(rng.integers(len(SEPS)))] for _ in range(int(rng.integers(1, 15))))
        out += (line + ENDS[int(rng.integers(len(ENDS)))]).encode()
    return bytes(out)


_vocabs = {}


def vocab(capcode=2, flags=NFD):
    """-> (Vocab, Oracle) of a small synthetic vocabulary with these normalization settings (made once per session)"""
    if (capcode, flags) not in _vocabs:
        rng = np.random.default_rng(8300 + capcode)
        toks = fuzz_vocab_tokens(rng, 2 if capcode == 2 else 0, 160) + [w.encode() for w in VOCAB_WORDS]
        if capcode == 2:
            toks += [b"D", b"C", b"W", b"D ", b"C ", b"W "]
        img = synth.build_vocab(list(dict.fromkeys(toks)), capcode=capcode, charset=1, norm_flag=flags, with_unk=True)
        _vocabs[(capcode, flags)] = (tm.Vocab(img), Oracle(img), img)
    return _vocabs[(capcode, flags)][:2]


def expected(v, orc, raw):
    """ids and missing of the whole text: host normalizer, then the one-call tokenizer - and the oracle must agree with that"""
    norm = np.frombuffer(bytes(synth.normalize(raw, v.capcode(), v.normalization_code())), dtype=np.uint8)
    ids, _, miss = v.tokenize_packed(norm, np.array([0, norm.size], dtype=np.uint64))
    exp = (ids, int(miss[0]) if norm.size else 0)
    oids, omiss = orc.tokenize(norm)
    assert oids.size == ids.size and (oids == ids).all() and omiss == exp[1], "tokenize_packed and the oracle disagree on the expectation"
    return exp


def stream_raw(v, raw, sizes, max_piece_bytes=PIECE, enc=None, watch=None):
    """feeds `raw` in pieces of `sizes` (the rest in one piece) -> (ids, missing)"""
    e = enc or v.encoder(max_piece_bytes)
    parts, pos = [], 0
    for s in sizes:
        parts.append(e.feed_raw(raw[pos:pos + s]))
        pos = min(pos + s, len(raw))
        if watch:
            watch(e)
    if pos < len(raw):
        parts.append(e.feed_raw(raw[pos:]))
    last, missing = e.finish()
    if watch:
        watch(e)
    if enc is None:
        e.close()
    return np.concatenate(parts + [last]), missing


def same(got, exp, what):
    ids, missing = got
    eids, emiss = exp
    assert ids.size == eids.size, "%s: %d ids, the whole document has %d" % (what, ids.size, eids.size)
    bad = np.nonzero(ids != eids)[0]
    assert bad.size == 0, "%s: ids differ from id %d on" % (what, int(bad[0]))
    assert missing == emiss, "%s: missing %d != %d" % (what, missing, emiss)


def random_sizes(rng, n, hi=1 << 16):
    sizes, left = [], n
    while left > 0:
        s = min(int(rng.integers(1, hi + 1)), left)
        sizes.append(s)
        left -= s
    return sizes


def split_invariance(capcode, flags, n=200_000, n_bytewise=6_000):
    v, orc = vocab(capcode, flags)
    assert v.encoder_raw_supported()
    raw = raw_text(41, n, WORDS if flags & ACCENTS else WORDS + KANA)
    exp = expected(v, orc, raw)
    assert exp[0].size > n // 16
    rng = np.random.default_rng(78)
    host = []
    watch = lambda e: host.append(e.host_pieces)
    for rep in range(2):
        same(stream_raw(v, raw, random_sizes(rng, len(raw)), watch=watch), exp, "capcode %d flags %d, random pieces %d" % (capcode, flags, rep))
    same(stream_raw(v, raw, random_sizes(rng, len(raw), 300), watch=watch), exp, "capcode %d flags %d, pieces of at most 300 bytes" % (capcode, flags))
    short = raw[:n_bytewise]
    same(stream_raw(v, short, [1] * len(short), watch=watch), expected(v, orc, short), "capcode %d flags %d, one byte at a time" % (capcode, flags))
    assert max(host) == 0, "the device normalizer left %d pieces to the host: this text is meant to stay on the device" % max(host)
    if flags & ACCENTS:
        raw = raw_text(42, n // 4, WORDS + KANA)
        enc = v.encoder(PIECE)
        same(stream_raw(v, raw, random_sizes(rng, len(raw)), enc=enc), expected(v, orc, raw), "capcode %d flags %d, voiced kana: host pieces among the device's" % (capcode, flags))
        assert enc.host_pieces > 0
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("capcode,flags", [(2, NFD), (2, NFD | LOWER), (2, NFD | ACCENTS | COLLAPSE | UNIXLINES), (0, 0), (0, COLLAPSE | UNIXLINES)])
def test_split_invariance(capcode, flags):
    split_invariance(capcode, flags)


@pytest.mark.gpu
def test_every_cut_in_a_window():
    """3 KB in two feeds, [0, c) and [c, end), for each of 300 consecutive c: the window holds a '\\r\\n', a capital run followed by a lower-case
    letter, a letter with three marks that NFD reorders, and a four-byte character"""
    v, orc = vocab()
    window = "one HELLO WORLd two\r\nABCdef e\u0301\u0308\u0327 x \U0001F600\U0001F680 y CAF\u00c9 DON'T\r\n\r\nend Of The WINDOW. AND On\n".encode()
    head = raw_text(51, 1400)
    raw = head + window * 4 + raw_text(52, 3000 - len(head) - 4 * len(window))
    assert 2900 <= len(raw) <= 3300 and 4 * len(window) >= 300
    exp = expected(v, orc, raw)
    enc = v.encoder(PIECE)
    for c in range(len(head) - 10, len(head) + 290):
        first = enc.feed_raw(raw[:c])
        assert enc.raw_held == c - (raw.rfind(b"\n", 0, c) + 1)
        rest = enc.feed_raw(raw[c:])
        last, missing = enc.finish()
        same((np.concatenate([first, rest, last]), missing), exp, "cut at %d (%r | %r)" % (c, raw[c - 4:c], raw[c:c + 4]))
        assert enc.state == 0 and enc.raw_held == 0
    enc.close()


@pytest.mark.gpu
def test_short_and_empty_documents():
    v, orc = vocab()
    enc = v.encoder(PIECE)
    assert enc.feed_raw(b"").size == 0
    ids, missing = enc.finish()
    assert ids.size == 0 and missing == 0
    for doc in (b"\n", b"Hello World", "Hello\nWORLD e\u0301\n".encode(), b"A", "\xc9".encode(), b"\r\n", b"x\r"):
        assert len(bytes(synth.normalize(doc, 2, NFD))) < 192
        same(stream_raw(v, doc, [len(doc)], enc=enc), expected(v, orc, doc), "%r" % doc)             # one document after the other on one encoder
        same(stream_raw(v, doc, [1] * len(doc), enc=enc), expected(v, orc, doc), "%r byte by byte" % doc)
        assert enc.state == 0 and enc.raw_held == 0
    a, b = raw_text(61, 9000), raw_text(62, 5000)[:-1] + b"tail without a line end"
    same(stream_raw(v, a, [1000, 5000], enc=enc), expected(v, orc, a), "first of two documents")
    same(stream_raw(v, b, [3000], enc=enc), expected(v, orc, b), "second of two documents, no final line feed")
    same(v.tokenize_raw_stream([a[:700], b"", a[700:]]), expected(v, orc, a), "tokenize_raw_stream")
    enc.close()


@pytest.mark.gpu
def test_long_lines():
    v, orc = vocab()
    sentence = "Hello WORLD this is A Sentence of caf\xe9 and 123. ".encode()
    doc = (sentence * (10_000 // len(sentence) + 1))[:10_000]
    assert b"\n" not in doc
    held = []
    rng = np.random.default_rng(91)
    same(stream_raw(v, doc, random_sizes(rng, len(doc), 3000), watch=lambda e: held.append(e.raw_held)), expected(v, orc, doc), "10 KB without a line feed")
    same(stream_raw(v, doc, [1] * len(doc), watch=lambda e: held.append(e.raw_held)), expected(v, orc, doc), "10 KB without a line feed, byte by byte")
    assert max(held) <= PIECE and max(held) > PIECE // 2, max(held)
    enc = v.encoder(PIECE)
    with pytest.raises(N.TokenMonsterHipError) as ei:
        enc.feed_raw(b"a" * 10_000)
    assert ei.value.code == N.TM_E_LIMIT and "without a separator" in str(ei.value)
    for call in (lambda: enc.feed_raw(b"more\n"), lambda: enc.feed(b" more"), enc.finish):      # refused until reset
        with pytest.raises(N.TokenMonsterHipError) as ei:
            call()
        assert ei.value.code == N.TM_E_INVALID
    enc.reset()
    assert enc.raw_held == 0 and enc.state == 0
    ok = raw_text(92, 7000)
    same(stream_raw(v, ok, [2500, 2500], enc=enc), expected(v, orc, ok), "after the reset")
    enc.close()


@pytest.mark.gpu
def test_refusals():
    raw = raw_text(71, 6000)
    for capcode, flags, word in ((2, NFD | 32, "trim"), (2, NFD | 8, "quotemarks"), (1, 0, "capcode 1")):
        v, orc = vocab(capcode, flags)
        assert not v.encoder_raw_supported()
        assert N.lib.tm_encoder_raw_supported(v.handle) == 0
        enc = v.encoder(PIECE)
        with pytest.raises(N.TokenMonsterHipError) as ei:
            enc.feed_raw(raw)
        assert ei.value.code == N.TM_E_INVALID and word in str(ei.value), str(ei.value)
        assert enc.raw_held == 0 and enc.state == 0
        if capcode != 1:      # (the host normalizer writes capcode 0 and 2) the encoder is still good for normalized text
            norm = bytes(synth.normalize(raw, capcode, flags))
            parts = [enc.feed(norm[:2000]), enc.feed(norm[2000:])]
            last, missing = enc.finish()
            same((np.concatenate(parts + [last]), missing), expected(v, orc, raw), "normalized feed after the refusal (%s)" % word)
        else:
            ids = [enc.feed(b" abc de"), enc.finish()[0]]
            assert sum(i.size for i in ids) > 0
        enc.close()
    # one document is fed either raw or normalized
    v, orc = vocab()
    enc = v.encoder(PIECE)
    first = enc.feed_raw(raw[:3000])
    with pytest.raises(N.TokenMonsterHipError) as ei:
        enc.feed(b" abc")
    assert ei.value.code == N.TM_E_INVALID
    n = C.c_uint64(77)
    assert N.lib.tm_encoder_feed(enc._h, None, 0, None, 0, C.byref(n)) == N.TM_OK and n.value == 0      # n = 0 only fetches: free
    rest = enc.feed_raw(raw[3000:])
    last, missing = enc.finish()
    same((np.concatenate([first, rest, last]), missing), expected(v, orc, raw), "raw document with a refused normalized feed in the middle")
    norm = bytes(synth.normalize(raw, 2, NFD))
    first = enc.feed(norm[:3000])                                                                        # finish lifted the restriction
    with pytest.raises(N.TokenMonsterHipError) as ei:
        enc.feed_raw(b"Abc\n")
    assert ei.value.code == N.TM_E_INVALID and enc.raw_held == 0
    rest = enc.feed(norm[3000:])
    last, missing = enc.finish()
    same((np.concatenate([first, rest, last]), missing), expected(v, orc, raw), "normalized document with a refused raw feed in the middle")
    enc.feed_raw(raw[:100])
    enc.reset()                                                                                          # so does reset
    assert enc.feed(norm[:50]).size == 0
    enc.close()


@pytest.mark.gpu
def test_host_pieces():
    """chunks of whole lines of at most a piece, one feed each: every feed is one raw piece.  One chunk in eight has a line of full-width
    Latin, one a malformed sequence: those - and no others - go to the host normalizer inside the call"""
    v, orc = vocab()
    rng = np.random.default_rng(81)
    chunks, special = [], 0
    for k in range(64):
        c = raw_text(8100 + k, int(rng.integers(800, 3000)))
        c += b"" if c.endswith(b"\n") else b"\n"
        if k % 8 == 3:
            c += "\uff21\uff22 fullwidth \uff41\uff42\n".encode()
            special += 1
        if k == 30:
            c += b"malformed \xe2\x82 and \xff\xfe here\n"
            special += 1
        assert len(c) <= PIECE and c.endswith(b"\n")
        chunks.append(c)
    raw = b"".join(chunks)
    exp = expected(v, orc, raw)
    enc = v.encoder(PIECE)
    parts = [enc.feed_raw(c) for c in chunks]
    assert enc.raw_held == 0
    last, missing = enc.finish()
    same((np.concatenate(parts + [last]), missing), exp, "one piece per feed")
    assert 0 < enc.host_pieces <= len(chunks) // 4 and enc.host_pieces == special, (enc.host_pieces, special, len(chunks))
    same(stream_raw(v, raw, random_sizes(rng, len(raw)), enc=enc), exp, "random pieces")
    assert enc.host_pieces > 0
    same(stream_raw(v, chunks[0], [len(chunks[0])], enc=enc), expected(v, orc, chunks[0]), "a device-only document behind it")
    assert enc.host_pieces == 0                          # counted per document
    enc.close()


@pytest.mark.gpu
def test_output_too_small_keeps_the_ids():
    v, orc = vocab()
    raw = raw_text(95, 30_000)[:30_000]
    exp = expected(v, orc, raw)
    arr = np.frombuffer(raw, dtype=np.uint8)
    h = C.c_void_p()
    N.check(N.lib.tm_encoder_new(v.handle, 8192, C.byref(h)))
    try:
        n = C.c_uint64()
        small = np.full(100, 0xFFFFFFFF, dtype=np.uint32)
        got = []
        assert N.lib.tm_encoder_feed_raw(h, N.ptr(arr[:20_000]), 20_000, N.ptr(small), small.size, C.byref(n)) == N.TM_E_NOSPACE
        need1 = int(n.value)
        assert need1 > small.size
        held = int(N.lib.tm_encoder_raw_held(h))
        assert held == 20_000 - (raw.rfind(b"\n", 0, 20_000) + 1)                  # the text HAS been consumed
        assert N.lib.tm_encoder_feed_raw(h, N.ptr(arr[20_000:25_000]), 5_000, None, 0, C.byref(n)) == N.TM_E_NOSPACE
        need2 = int(n.value)
        assert need2 > need1
        assert N.lib.tm_encoder_feed_raw(h, None, 0, N.ptr(small), small.size, C.byref(n)) == N.TM_E_NOSPACE and int(n.value) == need2
        buf = np.empty(need2, dtype=np.uint32)
        N.check(N.lib.tm_encoder_feed_raw(h, None, 0, N.ptr(buf), buf.size, C.byref(n)))
        assert int(n.value) == need2
        got.append(buf.copy())
        N.check(N.lib.tm_encoder_feed_raw(h, None, 0, N.ptr(buf), buf.size, C.byref(n)))      # fetched once: nothing is handed out twice
        assert int(n.value) == 0
        N.check(N.lib.tm_encoder_feed_raw(h, N.ptr(arr[25_000:]), 5_000, N.ptr(buf), buf.size, C.byref(n)))
        got.append(buf[:int(n.value)].copy())
        missing = C.c_uint32(12345)
        assert N.lib.tm_encoder_finish(h, None, 0, C.byref(n), C.byref(missing)) == N.TM_E_NOSPACE
        assert missing.value == exp[1] and 0 < int(n.value) <= buf.size
        N.check(N.lib.tm_encoder_feed(h, None, 0, N.ptr(buf), buf.size, C.byref(n)))
        got.append(buf[:int(n.value)].copy())
        same((np.concatenate(got), int(missing.value)), exp, "ids kept over TM_E_NOSPACE")
        assert N.lib.tm_encoder_state(h) == 0 and N.lib.tm_encoder_raw_held(h) == 0
    finally:
        N.lib.tm_encoder_free(h)


# tm_encoder_device_bytes of an encoder of the benchmark's vocabulary (32 000 ids) with max_piece_bytes = 65536 that has only seen normalized text, as the commit
# before the raw path reports it (the text buffer, the pipeline's per-segment arrays, the id buffer): the raw path must not add to it
NORMALIZED_ONLY_DEVICE_BYTES = 894034


@pytest.mark.gpu
def test_bounded_memory():
    """4 MiB of raw text (1 MiB on the emulated device) through an encoder of 64 KiB pieces, with the benchmark's vocabulary (whose ids per byte
    are those of real text: the id buffer, which grows on demand, stays as it was made)"""
    total, piece = (1 << 20 if EMULATED else 4 << 20), 65536
    img = synth.config_vocab("englishcode-32000-consistent")
    v, orc = tm.Vocab(img), Oracle(img)
    assert v.capcode() == 2 and v.normalization_code() == NFD and v.encoder_raw_supported()
    text, _ = synth.synth_corpus(synth.ENGLISHCODE, total + (1 << 16), seed=6)
    raw = text[:total].tobytes()
    assert raw.count(b"\n") > total // 400
    exp = expected(v, orc, raw)
    plain = v.encoder(piece)
    before = plain.device_bytes()
    norm = bytes(synth.normalize(raw[:200_000], 2, NFD))
    plain.feed(norm[:100_000]), plain.feed(norm[100_000:]), plain.finish()
    assert plain.device_bytes() == before == NORMALIZED_ONLY_DEVICE_BYTES, (plain.device_bytes(), before)
    plain.close()
    enc = v.encoder(piece)
    assert enc.device_bytes() == before                  # the normalizer's workspace comes with the first raw feed
    parts, sizes, pos = [], [], 0
    rng = np.random.default_rng(98)
    while pos < len(raw):
        s = int(rng.integers(1, 200_000))
        parts.append(enc.feed_raw(raw[pos:pos + s]))
        sizes.append(enc.device_bytes())
        assert enc.raw_held <= piece
        pos += s
    last, missing = enc.finish()
    sizes.append(enc.device_bytes())
    same((np.concatenate(parts + [last]), missing), exp, "%d bytes of raw text" % len(raw))
    assert len(set(sizes)) == 1 and sizes[0] > before, (before, sorted(set(sizes)))
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, 4 << 20, 1, C.byref(b)))
    try:
        whole = int(N.lib.tm_batch_device_bytes(b))
    finally:
        N.lib.tm_batch_free(b)
    assert sizes[0] < whole, (sizes[0], whole)
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [256, 2048, 4096])
def test_rare_paths_give_the_same_ids(flags):
    """test hooks (tm_debug_flags): 256 = the normalizer's exact path with the per-lane rules, 2048 = the normalized text packed instead of
    staying in the slabs, 4096 = a document is long from 9 segments on"""
    old = N.lib.tm_debug_flags(flags)
    try:
        assert N.lib.tm_debug_flags(-1) == flags, "test hooks not armed"
        split_invariance(2, NFD, n=60_000, n_bytewise=2_000)
    finally:
        N.lib.tm_debug_flags(old)


@pytest.mark.gpu
def test_two_encoders_on_two_threads():
    v, orc = vocab()
    docs = [raw_text(9901 + k, 150_000 + 1234 * k) for k in range(2)]
    exps = [expected(v, orc, d) for d in docs]
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def run(k):
        try:
            rng = np.random.default_rng(9911 + k)
            enc = v.encoder(1 << 14)
            gate.wait()
            results[k] = stream_raw(v, docs[k], random_sizes(rng, len(docs[k]), 9000), enc=enc)
            enc.close()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
            gate.abort()

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for k in range(2):
        same(results[k], exps[k], "encoder %d" % k)


@pytest.mark.gpu
def test_c_example_streams_a_raw_file(tmp_path):
    """examples/tokenize_stream --raw on a raw file writes the ids file it writes for the normalized file"""
    from conftest import example_env
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    v, orc = vocab()
    img = _vocabs[(2, NFD)][2]
    raw = raw_text(99, (1 << 18) + 777 if EMULATED else (3 << 20) + 777)
    exp = expected(v, orc, raw)
    (tmp_path / "v.vocab").write_bytes(bytes(img))
    (tmp_path / "raw.txt").write_bytes(raw)
    (tmp_path / "norm.txt").write_bytes(bytes(synth.normalize(raw, 2, NFD)))
    exe = os.path.join(ROOT, "examples", "tokenize_stream")
    for args, out in ((["--raw", str(tmp_path / "v.vocab"), str(tmp_path / "raw.txt")], "raw.bin"), ([str(tmp_path / "v.vocab"), str(tmp_path / "norm.txt")], "norm.bin")):
        r = subprocess.run([exe] + args + ["1", str(tmp_path / out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=example_env())
        assert r.returncode == 0, r.stderr.decode(errors="replace")
    got = np.fromfile(str(tmp_path / "raw.bin"), dtype="<u4")
    same((got, exp[1]), exp, "tokenize_stream --raw, ids file")
    assert (tmp_path / "raw.bin").read_bytes() == (tmp_path / "norm.bin").read_bytes()


def test_raw_on_the_emulated_device():
    """the split-invariance and every-cut cases above on the emulated device (tools/emu: the kernel sources compiled for the host, tests/conftest.py TM_EMU=1)"""
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_stream_encoder_raw.py", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_split_invariance or test_every_cut_in_a_window"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=3000)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert "6 passed" in out and " failed" not in out, out[-2000:]

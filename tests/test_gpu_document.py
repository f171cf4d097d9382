"""-m gpu: tm_tokenize_document (Vocab.tokenize_document): ONE document in hand as a whole, tokenized in pieces that run through several
device workspaces at once, must give the ids - and `missing` - of the whole document tokenized at once (the oracle's one-shot walk), whatever
the piece size, the number of slots and the width of the serialized ids: piece sizes around the 64-byte minimum range, the 128-byte
look-ahead and the 256-byte segments, every length of a window, the group tree inside a piece, raw text cut behind line feeds and normalized
piece by piece, vocabularies whose normalizer needs the whole document, the error paths, bounded device memory, two calls at once, pinned and
pageable buffers, and the C example.  test_document_on_the_emulated_device runs the same file on the emulated device (tools/emu) without a
GPU; that run is no evidence for the device - streams and events do nothing there -, the -m gpu run is."""
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
from conftest import fuzz_text, fuzz_vocab_tokens
from oracle_bind import Oracle
from test_gpu_stream_encoder import fd_dense_text, fd_dense_vocab, make_case, same
import test_gpu_stream_encoder_raw as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMULATED = os.environ.get("TM_EMU") == "1"
PIECES = [64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 1000, 4096, 70_000]
SLOTS = [2, 3, 8]
ENCS = [0, 2, 3, 4]
HALO, MIN_RANGE = 128, 64
LONG, SHORT = (40_000, 3_000) if EMULATED else (300_000, 6_000)      # document sizes: pieces of 1 000 bytes and more / the small pieces


def pieces_of(n, piece):
    """pieces of a normalized document: whole pieces, a tail shorter than the minimum range folded into the piece before it"""
    if n == 0:
        return 0
    k = -(-n // piece)
    if k > 1 and n - (k - 1) * piece < MIN_RANGE:
        k -= 1
    return k


def as_enc(ids, enc, n_ids):
    """what ids look like in `enc` bytes: two-byte ids of a larger vocabulary are cut (go/tokenmonster.go:1545)"""
    used = enc or (2 if n_ids <= 65536 else 3)
    return (ids & 0xFFFF) if used == 2 else ids, used


def check(v, data, exp, what, raw=False, **kw):
    ids, missing, st = v.tokenize_document(data, raw=raw, **kw)
    want, used = as_enc(exp[0], kw.get("encoding_length", 0), v.n_ids())
    assert st["encoding_length"] == used, what
    assert ids.dtype == (np.uint16 if used == 2 else np.uint32), what
    same((ids.astype(np.uint32), missing), (want, exp[1]), what)
    return st


_cases = {}


def case(kind, n):
    """-> (Vocab, document, its expected (ids, missing) from the oracle's one-shot walk): made once, shared, never changed"""
    if (kind, n) not in _cases:
        img, data = make_case(kind, n)
        _cases[(kind, n)] = (tm.Vocab(img), data, Oracle(img).tokenize(data))
    return _cases[(kind, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fd-dense", "capcode0", "len40", "wide"])
def test_split_invariance_normalized(kind):
    """every piece size with every number of slots and every id width (each piece size: all slots, then all widths - 6 calls)"""
    for piece in PIECES:
        v, data, exp = case(kind, LONG if piece >= 1000 else SHORT)
        assert exp[0].size > len(data) // 8
        combos = [(s, ENCS[(i + PIECES.index(piece)) % 4]) for i, s in enumerate(SLOTS)] + [(SLOTS[(i + PIECES.index(piece)) % 3], e) for i, e in enumerate(ENCS)]
        for slots, enc in dict.fromkeys(combos):
            st = check(v, data, exp, "%s, pieces of %d, %d slots, %d-byte ids" % (kind, piece, slots, enc), piece_bytes=piece, slots=slots, encoding_length=enc)
            assert st["pieces"] == pieces_of(len(data), piece) and st["slots"] == slots
            assert st["normalized_bytes"] == len(data) and st["host_pieces"] == 0 and st["host_normalized"] == 0
    if kind == "wide":
        assert v.n_ids() > 65536


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [64, 256])
def test_every_length_of_a_window(piece):
    """every document length 0 .. 700: the empty document, documents shorter than the look-ahead, a document of one byte, last pieces of every
    length from the minimum range on, and tails folded into the piece before them"""
    img = fd_dense_vocab(1)
    v, orc = tm.Vocab(img), Oracle(img)
    text = fd_dense_text(np.random.default_rng(9601), 6000)
    folded = 0
    for n in range(0, 701, 7 if EMULATED else 1):
        doc = text[:n]
        st = check(v, doc, orc.tokenize(doc), "%d bytes in pieces of %d" % (n, piece), piece_bytes=piece, slots=3, encoding_length=4)
        assert st["pieces"] == pieces_of(n, piece)
        folded += n > piece and 0 < n % piece < MIN_RANGE
    assert folded > (10 if EMULATED else 100)


@pytest.mark.gpu
def test_group_tree_inside_a_piece():
    v, data, exp = case("fd-dense", LONG)
    old = N.lib.tm_debug_flags(4096)
    try:
        assert N.lib.tm_debug_flags(-1) == 4096, "test hooks not armed"
        check(v, data, exp, "group tree from 9 segments on, pieces of 4096", piece_bytes=4096)      # 16 segments a piece
    finally:
        N.lib.tm_debug_flags(old)
    if not EMULATED:
        st = check(v, data, exp, "pieces of 200 000: 782 segments", piece_bytes=200_000)
        assert st["pieces"] == 2


def raw_document(seed, n):
    """the raw encoder tests' text (ASCII, two-byte scripts, Hangul, CRLF) with runs of blank lines and lines longer than a small piece"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    k = 0
    while len(out) < n:
        out += R.raw_text(seed * 100 + k, int(rng.integers(200, 1500)))
        if k % 4 == 0:
            out += b"\n" * int(rng.integers(2, 40))
        elif k % 4 == 1:
            out += b"\r\n" * int(rng.integers(2, 20))
        elif k % 4 == 2:
            out += R.raw_text(seed * 100 + 50 + k, 900).replace(b"\n", b" ").replace(b"\r", b" ") + b"\n"      # one line of 900 bytes
        k += 1
    return bytes(out)


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [64, 200, 1000, 70_000])
def test_raw(piece):
    v, orc = R.vocab()
    raw = raw_document(7, LONG if piece >= 1000 else SHORT)
    assert b"\r\n" in raw and b"\n\n\n" in raw and "한".encode() in raw
    exp = R.expected(v, orc, raw)
    for slots in SLOTS:
        st = check(v, raw, exp, "raw, pieces of %d, %d slots" % (piece, slots), raw=True, piece_bytes=piece, slots=slots)
        assert st["normalized_bytes"] == len(v.normalize(raw)) and st["host_normalized"] == 0 and st["host_pieces"] == 0, st
        assert st["pieces"] >= len(raw) // piece
    check(v, raw, exp, "raw, pieces of %d, four-byte ids" % piece, raw=True, piece_bytes=piece, encoding_length=4)


@pytest.mark.gpu
def test_raw_pieces_for_the_host_normalizer_and_pieces_that_own_nothing():
    v, orc = R.vocab()
    raw = R.raw_text(8, 3000) + "ＡＢ fullwidth ａｂ\n".encode() + R.raw_text(9, 3000)
    st = check(v, raw, R.expected(v, orc, raw), "a full-width Latin line", raw=True, piece_bytes=1000)
    assert st["host_pieces"] >= 1 and st["host_normalized"] == 0
    # blank lines for more than three pieces on end: passes of 64 bytes each, too short to own anything, roll into the next one
    for piece in (64, 200):
        raw = R.raw_text(10, 2000) + b"\n" * (3 * piece + 50) + R.raw_text(11, 2000) + b"\n" * 70
        st = check(v, raw, R.expected(v, orc, raw), "blank lines for more than three pieces of %d" % piece, raw=True, piece_bytes=piece)
        assert st["normalized_bytes"] == len(v.normalize(raw))
    for doc in (b"", b"\n", b"\n" * 500, b"Hello World", b"x\r"):
        check(v, doc, R.expected(v, orc, doc), "%r" % doc[:20], raw=True, piece_bytes=64)


@pytest.mark.gpu
@pytest.mark.parametrize("flag,word", [(32, "trim"), (8, "quotemarks"), (64, "leadingspace")])
def test_flags_that_need_the_whole_document(flag, word):
    v, orc = R.vocab(2, R.NFD | flag)
    raw = b"  \n " + R.raw_text(12, 20_000).replace(b"'", b"\"") + b" \n \n"
    exp = R.expected(v, orc, raw)
    st = check(v, raw, exp, word, raw=True, piece_bytes=1000)
    assert st["host_normalized"] == 1 and st["normalized_bytes"] == len(v.normalize(raw)) and st["pieces"] == pieces_of(st["normalized_bytes"], 1000)


@pytest.mark.gpu
def test_raw_text_without_a_byte_to_cut_behind_and_capcode_1():
    v, orc = R.vocab()
    raw = R.raw_text(13, 3000) + b"Abc def " + b"abcde " * 400 + b"\n" + R.raw_text(14, 3000)      # 2 400 bytes of letters and blanks
    st = check(v, raw, R.expected(v, orc, raw), "no cut within a piece", raw=True, piece_bytes=1000)
    assert st["host_normalized"] == 1
    st = check(v, raw, R.expected(v, orc, raw), "the same text in larger pieces", raw=True, piece_bytes=4096)
    assert st["host_normalized"] == 0
    v1, _ = R.vocab(1, 0)
    with pytest.raises(N.TokenMonsterHipError) as ei:
        v1.tokenize_document(raw, raw=True)
    assert ei.value.code == N.TM_E_INVALID and "capcode 1" in str(ei.value)
    ids, _, _ = v1.tokenize_document(b" abc de" * 100, raw=False, piece_bytes=64)
    assert ids.size > 0


def call(v, arr, out, raw=0, enc=4, piece=4096, slots=0):
    need, miss = C.c_uint64(12345), C.c_uint32()
    rc = N.lib.tm_tokenize_document(v.handle, N.ptr(arr) if arr.size else None, arr.size, raw, enc, piece, slots, N.ptr(out) if out is not None else None,
                                    out.size if out is not None else 0, C.byref(need), C.byref(miss), None, None)
    return rc, int(need.value), int(miss.value)


@pytest.mark.gpu
def test_output_too_small_and_bad_arguments():
    v, data, exp = case("fd-dense", LONG)
    arr = np.frombuffer(data, dtype=np.uint8)
    for out in (None, np.zeros(1000, dtype=np.uint8), np.zeros(exp[0].size * 4 - 1, dtype=np.uint8)):
        rc, need, _ = call(v, arr, out)
        assert rc == N.TM_E_NOSPACE and need == exp[0].size * 4
    out = np.zeros(need, dtype=np.uint8)
    rc, need2, miss = call(v, arr, out)
    assert rc == N.TM_OK and need2 == need
    same((out.view("<u4"), miss), exp, "the capacity TM_E_NOSPACE asked for")
    check(v, data, exp, "a call behind TM_E_NOSPACE", piece_bytes=4096)
    for kw in (dict(piece=63), dict(piece=(1 << 36) + 1), dict(slots=1), dict(slots=9), dict(enc=1), dict(enc=5)):
        rc, need, _ = call(v, arr, out, **kw)
        assert rc == N.TM_E_INVALID and need == 0, kw
    assert N.lib.tm_tokenize_document(v.handle, N.ptr(arr), arr.size, 0, 4, 0, 0, N.ptr(out), out.size, None, None, None, None) == N.TM_E_INVALID
    rc, need, _ = call(v, arr[:0], None)
    assert rc == N.TM_OK and need == 0


@pytest.mark.gpu
def test_more_ids_than_a_slot_holds():
    """one-byte tokens only: an id per byte, twice what a slot's id buffers are made for - the emit stage is repeated into larger ones"""
    img = synth.build_vocab([bytes([c]) for c in b"abcdefgh "], capcode=0, charset=1, with_unk=False)
    v, orc = tm.Vocab(img), Oracle(img)
    data = bytes(np.random.default_rng(5).choice(np.frombuffer(b"abcdefgh ", dtype=np.uint8), size=30_000))
    exp = orc.tokenize(data)
    assert exp[0].size == len(data)
    for enc in (2, 3, 4):
        for piece in (4096, 20_000):
            for rep in range(2):
                check(v, data, exp, "an id per byte, pieces of %d, %d-byte ids, call %d" % (piece, enc, rep), piece_bytes=piece, encoding_length=enc)


def _utf16(bs):
    return b"".join(bytes([c, 0]) for c in bs)


@pytest.mark.gpu
def test_utf16_dead_end_in_the_third_of_five_pieces():
    """the vocabulary and the 2 975-byte text of test_gpu_parity.test_utf16_cut_character_ends_the_walk_with_an_error - it ends in half a
    character, where the walk stops advancing - between 6 000 bytes of whole characters and more text: pieces of 3 000 bytes, the dead end
    in the third of five.  That it lies there is the streaming encoder's word: its third pass of 3 000 bytes is the one that fails."""
    rng = np.random.default_rng(913)
    toks8 = fuzz_vocab_tokens(rng, 2, 100)
    toks = sorted(set(_utf16(t) for t in toks8 if len(t) <= 20) | {b"D", b" ", b"a"})
    v = tm.Vocab(synth.build_vocab(toks, capcode=2, charset=2))
    docs = []
    for n in rng.integers(0, 1800, size=40):
        doc = _utf16(fuzz_text(rng, 2, int(n)))
        docs.append(doc[:-1] if n % 3 == 0 else doc)
    bad = [d for d in docs if len(d) == 2975]
    assert len(bad) == 1
    found = None
    for seed in range(40):
        r2 = np.random.default_rng(9700 + seed)
        doc = _utf16(fuzz_text(r2, 2, 3000)[:3000]) + bad[0] + _utf16(fuzz_text(r2, 2, 3100))[:6025]
        assert len(doc) == 15_000
        enc = v.encoder(3000)
        try:
            enc.feed(doc[:3128])
            enc.feed(doc[3128:6128])
            try:
                enc.feed(doc[6128:9128])
            except N.TokenMonsterHipError as e:
                assert e.code == N.TM_E_INPUT
                found = doc
        except N.TokenMonsterHipError:
            pass
        enc.close()
        if found:
            break
    assert found is not None, "no text puts the dead end into the third piece"
    for slots in SLOTS:
        with pytest.raises(N.TokenMonsterHipError) as ei:
            v.tokenize_document(found, raw=False, piece_bytes=3000, slots=slots)
        assert ei.value.code == N.TM_E_INPUT
        good = found[:6000]
        ids, _, miss = v.tokenize_packed(*tm.pack_documents([good]))
        check(v, good, (ids, int(miss[0])), "a call behind the dead end, %d slots" % slots, piece_bytes=3000, slots=slots)


@pytest.mark.gpu
def test_bounded_memory():
    v, data, exp = case("fd-dense", LONG)
    orc = Oracle(fd_dense_vocab(1))
    sizes = [check(v, d, orc.tokenize(d), "%d bytes" % len(d), piece_bytes=4096)["device_bytes"] for d in (data[:LONG // 3], data + data[:LONG // 3])]
    assert sizes[0] == sizes[1] > 0, sizes
    assert check(v, data, exp, "two slots", piece_bytes=4096, slots=2)["device_bytes"] < sizes[0]


def steady_state_child():
    """(run in a process of its own with TM_TRACE set: see test_second_call_of_a_shape_allocates_nothing)"""
    v, orc = R.vocab()
    raw = R.raw_text(15, 100_000)
    norm = v.normalize(raw)
    for text, kw in ((raw, dict(raw=True, piece_bytes=4096)), (norm, dict(raw=False, piece_bytes=8192, slots=4))):
        for mark in ("FIRST", "SECOND"):
            sys.stderr.write(mark + "\n")
            sys.stderr.flush()
            v.tokenize_document(text, **kw)


@pytest.mark.gpu
def test_second_call_of_a_shape_allocates_nothing():
    """TM_TRACE names every buffer that is replaced by a larger one ([grow]): none during the second call of a shape, raw or normalized"""
    code = "import sys; sys.path.insert(0, 'tests'); import conftest; import test_gpu_document as t; t.steady_state_child()"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, TM_TRACE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    parts = err.split("SECOND\n")
    assert len(parts) == 3, err[-3000:]
    grows = [l for p in parts[1:] for l in p.split("FIRST\n")[0].splitlines() if "[grow]" in l]
    assert not grows, grows


@pytest.mark.gpu
def test_two_calls_at_once_and_one_beside_an_encoder():
    img = fd_dense_vocab(1)
    v, orc = tm.Vocab(img), Oracle(img)
    docs = [fd_dense_text(np.random.default_rng(9901 + k), 200_000 + 1234 * k) for k in range(2)]
    exps = [orc.tokenize(d) for d in docs]
    for second in ("document", "encoder"):
        results, errors = [None, None], []
        gate = threading.Barrier(2)

        def run(k):
            try:
                gate.wait()
                if k == 1 and second == "encoder":
                    enc = v.encoder(1 << 16)
                    parts = [enc.feed(docs[k][a:a + 5000]) for a in range(0, len(docs[k]), 5000)]
                    last, missing = enc.finish()
                    enc.close()
                    results[k] = (np.concatenate(parts + [last]), missing)
                else:
                    for _ in range(3):
                        ids, missing, _ = v.tokenize_document(docs[k], raw=False, encoding_length=4, piece_bytes=4096)
                        results[k] = (ids, missing)
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
            same(results[k], exps[k], "%s %d" % (second, k))


@pytest.mark.gpu
def test_pinned_and_pageable_buffers():
    v, data, exp = case("fd-dense", LONG)
    pin_in, pin_out = tm.PinnedBuffer(len(data)), tm.PinnedBuffer(len(data) * 2)
    pin_in.array[:] = np.frombuffer(data, dtype=np.uint8)
    first = None
    for inp, out in ((data, None), (pin_in, None), (data, pin_out), (pin_in, pin_out)):
        ids, missing, st = v.tokenize_document(inp, raw=False, encoding_length=2, piece_bytes=4096, out=out)
        assert (st["input_pinned"], st["output_pinned"]) == (int(inp is pin_in), int(out is pin_out)), st
        same((ids.astype(np.uint32), missing), exp, "pinned %s" % st)
        first = ids.tobytes() if first is None else first
        assert ids.tobytes() == first
    v2, orc2 = R.vocab()
    raw = R.raw_text(16, 100_000)
    pin_raw = tm.PinnedBuffer(len(raw))
    pin_raw.array[:] = np.frombuffer(raw, dtype=np.uint8)
    exp2 = R.expected(v2, orc2, raw)
    for inp in (raw, pin_raw):
        st = check(v2, inp, exp2, "raw, pinned input %s" % (inp is pin_raw), raw=True, piece_bytes=4096, out=pin_out)
        assert st["input_pinned"] == int(inp is pin_raw)


@pytest.mark.gpu
def test_c_example_gives_the_ids_of_the_streaming_example(tmp_path):
    from conftest import example_env
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    v, orc = R.vocab()
    raw = R.raw_text(17, 300_000)
    (tmp_path / "v.vocab").write_bytes(bytes(R._vocabs[(2, R.NFD)][2]))
    (tmp_path / "t.txt").write_bytes(raw)
    for prog in ("tokenize_document", "tokenize_stream"):
        r = subprocess.run([os.path.join(ROOT, "examples", prog), "--raw", str(tmp_path / "v.vocab"), str(tmp_path / "t.txt"), "1", str(tmp_path / (prog + ".bin"))],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=example_env())
        assert r.returncode == 0, r.stderr.decode(errors="replace")
    a, b = (tmp_path / "tokenize_document.bin").read_bytes(), (tmp_path / "tokenize_stream.bin").read_bytes()
    assert a == b and len(a) > 0
    same((np.frombuffer(a, dtype="<u4"), 0), (R.expected(v, orc, raw)[0], 0), "tokenize_document, ids file")


def test_document_on_the_emulated_device():
    """the -m gpu tests above on the emulated device (tools/emu: the kernel sources compiled for the host, tests/conftest.py TM_EMU=1)"""
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_document.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=3000)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert " passed" in out and " failed" not in out, out[-2000:]

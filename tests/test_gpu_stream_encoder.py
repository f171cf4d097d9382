"""-m gpu: the streaming encoder (tm_encoder_*, Vocab.encoder): ONE document fed piece by piece must give the ids - and `missing` - of the
whole document tokenized at once (the oracle's one-shot walk), however the text is cut: random and fixed piece sizes around the 64-byte
minimum range, the 128-byte look-ahead and the 256-byte segments, every cut of a window, documents shorter than the look-ahead, a long
document in bounded device memory, TM_E_NOSPACE, the UTF-16 dead end, the rarely taken paths of the pipeline (test hooks, a vocabulary of
more than 65 536 ids) and two encoders side by side.  test_stream_encoder_on_the_emulated_device runs the same file on the emulated
device (tools/emu), without a GPU; that run is no evidence for the device, the -m gpu run is."""
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
from oracle_bind import Oracle, oracle_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMULATED = os.environ.get("TM_EMU") == "1"
FIXED = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
MARKERS = [b"D a", b"D b", b"Da", b"D ab", b"C a", b"W b", b" a", b"a", b"D", b" "]
LONG_TOKENS = [(b"abcde" * 8)[:40], (b"edcba" * 8)[:40], (b" " + b"abcde" * 8)[:40], (b"abcde" * 8)[:39], (b"aabbccddee" * 4)[:40]]


def fd_dense_vocab(seed):
    """the capcode-2 vocabulary of test_gpu_exit_maps.test_text_dense_in_forward_delete_states: 'D x' / ' x' pairs, so (p,1) states abound"""
    rng = np.random.default_rng(8200 + seed)
    toks = fuzz_vocab_tokens(rng, 2, 160)
    toks = list(dict.fromkeys(toks + [b"D " + bytes([c]) for c in b"abcde"] + [b" " + bytes([c]) for c in b"abcde"] + [b"D", b" "]))
    return synth.build_vocab(toks, capcode=2, charset=1, with_unk=True)


def fd_dense_text(rng, n):
    out = bytearray()
    while len(out) < n:
        k = int(rng.integers(20, 400))
        out += b"".join(bytes(rng.choice(MARKERS)) for _ in range(k)) if rng.random() < 0.25 else fuzz_text(rng, 2, k)
    return bytes(out[:n])


def make_case(kind, n):
    """-> (vocabulary image, a document of n bytes)"""
    if kind == "fd-dense":
        return fd_dense_vocab(1), fd_dense_text(np.random.default_rng(9101), n)
    if kind == "capcode0":
        rng = np.random.default_rng(9102)
        return synth.build_vocab(fuzz_vocab_tokens(rng, 0, 200), capcode=0, charset=1, with_unk=False), fuzz_text(rng, 0, n)
    if kind == "len40":
        rng = np.random.default_rng(9103)
        img = synth.build_vocab(list(dict.fromkeys(fuzz_vocab_tokens(rng, 2, 150) + LONG_TOKENS)), capcode=2, charset=1, with_unk=True)
        out = bytearray()
        while len(out) < n:      # the 40-byte tokens whole, cut short and run together, between ordinary text
            r = rng.random()
            out += fuzz_text(rng, 2, int(rng.integers(1, 120))) if r < 0.5 else bytes(LONG_TOKENS[int(rng.integers(len(LONG_TOKENS)))])[:40 if r < 0.9 else int(rng.integers(1, 40))]
        return img, bytes(out[:n])
    if kind == "wide":      # more than 65 536 ids: u32 rows, k_emit_list<true> (and the one-plane rows of k_emit_tiles<false> under hook 15)
        rng = np.random.default_rng(9104)
        toks = fuzz_vocab_tokens(rng, 2, 160) + [b"D " + bytes([c]) for c in b"abcde"] + [b" " + bytes([c]) for c in b"abcde"]
        toks = list(dict.fromkeys(toks)) + [bytes([0x7F, 0x30 + k % 40, 0x30 + (k // 40) % 40, 0x30 + k // 1600]) for k in range(66_000)]
        return synth.build_vocab(toks, capcode=2, charset=1, with_unk=True), fd_dense_text(rng, n)
    raise ValueError(kind)


def mixed_sizes(rng, n):
    """piece sizes that sum to n: seeded random ones in 1 .. 70 000, three of the fixed sizes behind each (all of them within the first
    four, so before 300 000 bytes are through)"""
    fixed = list(FIXED)
    rng.shuffle(fixed)
    sizes, left = [], n
    while left > 0:
        for s in [int(rng.integers(1, 70_001))] + [fixed.pop() for _ in range(min(3, len(fixed)))]:
            s = min(s, left)
            sizes.append(s)
            left -= s
    return sizes


def stream(v, data, sizes, max_piece_bytes=0, enc=None):
    """feeds `data` in pieces of `sizes` (the rest in one piece) -> (ids, missing)"""
    e = enc or v.encoder(max_piece_bytes)
    parts, pos = [], 0
    for s in sizes:
        parts.append(e.feed(data[pos:pos + s]))
        pos = min(pos + s, len(data))
    if pos < len(data):
        parts.append(e.feed(data[pos:]))
    last, missing = e.finish()
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


def split_invariance(kind, n=300_000, n_bytewise=6_000):
    img, data = make_case(kind, n)
    v, orc = tm.Vocab(img), Oracle(img)
    exp = orc.tokenize(data)
    assert exp[0].size > n // 8
    rng = np.random.default_rng(77)
    for rep in range(2):
        sizes = mixed_sizes(rng, n)
        assert sum(sizes) == n and set(FIXED) <= set(sizes)
        same(stream(v, data, sizes), exp, "%s, mixed pieces %d" % (kind, rep))
    same(stream(v, data, [n]), exp, kind + ", one feed")
    same(stream(v, data, [n], max_piece_bytes=50_000), exp, kind + ", one feed split inside")
    short = data[:n_bytewise]
    same(stream(v, short, [1] * len(short)), orc.tokenize(short), kind + ", one byte at a time")
    same(stream(v, short, [len(short)], max_piece_bytes=64), orc.tokenize(short), kind + ", split inside into the smallest ranges")
    return v, orc, data, exp


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fd-dense", "capcode0", "len40"])
def test_split_invariance(kind):
    oracle_stats(reset=True)
    split_invariance(kind)
    if kind == "fd-dense":
        st = oracle_stats()
        assert st["s1b"] + st["s2b"] + st["s3b"] > 0, st          # the walk took forward-delete branches


@pytest.mark.gpu
def test_every_cut_in_a_window():
    """A document of 2 000 bytes in two feeds, [0, c) and [c, end), for every c in 1 .. 600 (two segment boundaries with the look-ahead on
    either side).  After a first feed of c >= 192 bytes the encoder has walked [0, c - 128); its state must be the oracle's exit state of
    that range.  With this seed the oracle's exit states over c = 192 .. 600 hold 85 odd ones (a forward delete pending at the cut) and
    175 of 2 or more (a token straddles the cut) - checked below: a condition on the input, not on the code."""
    img = fd_dense_vocab(1)
    v, orc = tm.Vocab(img), Oracle(img)
    data = fuzz_text(np.random.default_rng(9201), 2, 2000)
    exp = orc.tokenize(data)
    arr = np.frombuffer(data, dtype=np.uint8)
    want = {c: int(orc.score_range(arr, 0, c - 128, 0)[3]) for c in range(192, 601)}
    assert sum(1 for s in want.values() if s & 1) >= 10 and sum(1 for s in want.values() if s >= 2) >= 50, sorted(want.values())
    enc = v.encoder(1 << 16)
    states = {}
    for c in range(1, 601):
        first = enc.feed(data[:c])
        if c >= 192:
            states[c] = enc.state
        else:
            assert first.size == 0 and enc.state == 0
        rest = enc.feed(data[c:])
        last, missing = enc.finish()
        same((np.concatenate([first, rest, last]), missing), exp, "cut at %d" % c)
        assert enc.state == 0
    assert states == want, {c: (states[c], want[c]) for c in want if states[c] != want[c]}
    assert any(s & 1 for s in states.values()) and any(s >= 2 for s in states.values())


@pytest.mark.gpu
def test_short_and_empty_documents():
    img = fd_dense_vocab(1)
    v, orc = tm.Vocab(img), Oracle(img)
    rng = np.random.default_rng(9301)
    enc = v.encoder(1 << 16)
    ids, missing = enc.finish()
    assert ids.size == 0 and missing == 0
    assert enc.feed(b"").size == 0
    ids, missing = enc.finish()
    assert ids.size == 0 and missing == 0
    for n in (1, 63, 127, 128, 129, 191, 192, 193):
        doc = fd_dense_text(rng, n)
        same(stream(v, doc, [n], enc=enc), orc.tokenize(doc), "%d bytes" % n)             # a second, third ... document after finish
        same(stream(v, doc, [n // 2], enc=enc), orc.tokenize(doc), "%d bytes in two" % n)
        assert enc.state == 0
    # reset in mid-document: what was fed is forgotten, ids that were not fetched included
    doc, other = fd_dense_text(rng, 5000), fd_dense_text(rng, 3000)
    assert enc.feed(other[:2500]).size > 0 and enc.feed(other[2500:2600]).size >= 0
    enc.reset()
    assert enc.state == 0
    same(stream(v, doc, [1000, 3000], enc=enc), orc.tokenize(doc), "after reset")
    same(v.tokenize_normalized_stream([doc[:700], b"", doc[700:]]), orc.tokenize(doc), "tokenize_normalized_stream")
    same(v.tokenize_normalized_stream(iter([])), (np.zeros(0, np.uint32), 0), "tokenize_normalized_stream of nothing")
    h = C.c_void_p()
    assert N.lib.tm_encoder_new(v.handle, 63, C.byref(h)) == N.TM_E_INVALID and not h.value


@pytest.mark.gpu
def test_one_long_document_in_bounded_memory():
    """64 MiB of synthetic text (1 MiB on the emulated device) in 8 MiB pieces (128 KiB) through an encoder of that piece size: the ids of the
    oracle's one-shot walk and of tokenize_packed, device memory that does not grow with the document and is smaller than a batch's for the whole"""
    total, piece = (1 << 20, 128 << 10) if EMULATED else (64 << 20, 8 << 20)
    img = synth.config_vocab("englishcode-32000-consistent")
    v, orc = tm.Vocab(img), Oracle(img)
    raw, offs = synth.synth_corpus(synth.ENGLISHCODE, total + (1 << 16), seed=5)
    ntext, _ = synth.normalize_batch(raw, offs, v.capcode(), v.normalization_code())
    data = np.ascontiguousarray(ntext[:total])
    assert data.size == total
    exp = orc.tokenize(data)
    enc = v.encoder(piece)
    parts, sizes = [], []
    for a in range(0, total, piece):
        parts.append(enc.feed(data[a:a + piece]))
        sizes.append(enc.device_bytes())
    last, missing = enc.finish()
    sizes.append(enc.device_bytes())
    same((np.concatenate(parts + [last]), missing), exp, "long document")
    assert all(p.size > 0 for p in parts)
    assert len(set(sizes)) == 1, sizes
    ids, toff, miss = v.tokenize_packed(data, np.array([0, total], dtype=np.uint64))
    same((ids, int(miss[0])), exp, "tokenize_packed of the same bytes")
    b = C.c_void_p()
    N.check(N.lib.tm_batch_create(v.handle, total, 1, C.byref(b)))
    try:
        whole = int(N.lib.tm_batch_device_bytes(b))
    finally:
        N.lib.tm_batch_free(b)
    assert sizes[0] < whole, (sizes[0], whole)
    enc.close()


@pytest.mark.gpu
def test_output_too_small_keeps_the_ids():
    img = fd_dense_vocab(1)
    v, orc = tm.Vocab(img), Oracle(img)
    data = fd_dense_text(np.random.default_rng(9501), 30_000)
    exp = orc.tokenize(data)
    h = C.c_void_p()
    N.check(N.lib.tm_encoder_new(v.handle, 8192, C.byref(h)))
    try:
        arr = np.frombuffer(data, dtype=np.uint8)
        n = C.c_uint64()
        small = np.full(100, 0xFFFFFFFF, dtype=np.uint32)
        got = []
        # 20 000 bytes = three passes inside: the first 100 ids would fit, the rest does not - everything is kept, in order
        assert N.lib.tm_encoder_feed(h, N.ptr(arr[:20_000]), 20_000, N.ptr(small), small.size, C.byref(n)) == N.TM_E_NOSPACE
        need1 = int(n.value)
        assert need1 > small.size
        # more text while ids are waiting: consumed too, the count grows
        assert N.lib.tm_encoder_feed(h, N.ptr(arr[20_000:25_000]), 5_000, None, 0, C.byref(n)) == N.TM_E_NOSPACE
        need2 = int(n.value)
        assert need2 > need1
        assert N.lib.tm_encoder_feed(h, None, 0, N.ptr(small), small.size, C.byref(n)) == N.TM_E_NOSPACE and int(n.value) == need2
        buf = np.empty(need2, dtype=np.uint32)
        N.check(N.lib.tm_encoder_feed(h, None, 0, N.ptr(buf), buf.size, C.byref(n)))
        assert int(n.value) == need2
        got.append(buf.copy())
        N.check(N.lib.tm_encoder_feed(h, None, 0, N.ptr(buf), buf.size, C.byref(n)))        # fetched once: nothing is handed out twice
        assert int(n.value) == 0
        N.check(N.lib.tm_encoder_feed(h, N.ptr(arr[25_000:]), 5_000, N.ptr(buf), buf.size, C.byref(n)))
        got.append(buf[:int(n.value)].copy())
        missing = C.c_uint32(12345)
        assert N.lib.tm_encoder_finish(h, None, 0, C.byref(n), C.byref(missing)) == N.TM_E_NOSPACE
        assert missing.value == exp[1] and 0 < int(n.value) <= buf.size
        N.check(N.lib.tm_encoder_feed(h, None, 0, N.ptr(buf), buf.size, C.byref(n)))
        got.append(buf[:int(n.value)].copy())
        same((np.concatenate(got), int(missing.value)), exp, "ids kept over TM_E_NOSPACE")
        assert N.lib.tm_encoder_state(h) == 0
    finally:
        N.lib.tm_encoder_free(h)


def _utf16(bs):
    return b"".join(bytes([c, 0]) for c in bs)


@pytest.mark.gpu
def test_utf16_dead_end_is_an_error():
    """the vocabulary and texts of test_gpu_exit_maps.test_utf16_self_successor_is_a_dead_end: where the one-shot call reports TM_E_INPUT
    (the reference does not terminate there) the encoder does too - never a hang, never ids -, and where it tokenizes the ids agree"""
    rng = np.random.default_rng(913)
    toks8 = fuzz_vocab_tokens(rng, 2, 100)
    toks = sorted(set(_utf16(t) for t in toks8 if len(t) <= 20) | {b"D", b" ", b"a"})
    v = tm.Vocab(synth.build_vocab(toks, capcode=2, charset=2))
    enc = v.encoder(1 << 16)
    dead = 0
    for n in (300, 700, 1100, 1487, 1500, 1800):
        whole = _utf16(fuzz_text(rng, 2, n)[:n])
        for doc in (whole[:-1], whole, whole[:-2]):
            try:
                ids, _, miss = v.tokenize_packed(*tm.pack_documents([doc]))
                exp = (ids, int(miss[0]))
            except N.TokenMonsterHipError as e:
                assert e.code == N.TM_E_INPUT
                exp = None
            if exp is not None:
                same(stream(v, doc, [len(doc) // 3, 500], enc=enc), exp, "utf-16, %d bytes" % len(doc))
                continue
            dead += 1
            with pytest.raises(N.TokenMonsterHipError) as ei:
                stream(v, doc, [len(doc) // 3, 500], enc=enc)
            assert ei.value.code == N.TM_E_INPUT
            with pytest.raises(N.TokenMonsterHipError) as ei:      # the carried state means nothing now: refused until reset
                enc.feed(b"a\x00")
            assert ei.value.code == N.TM_E_INVALID
            enc.reset()
    assert dead > 0


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [32, 4096, 1024, 32768])
def test_rare_paths_give_the_same_ids(flags):
    """test hooks (tm_debug_flags): 32 = the wide exit map for every segment, 4096 = group tree from 9 segments on, 1024 = K4 stores every id
    directly, 32768 = K4's id-staging walk"""
    old = N.lib.tm_debug_flags(flags)
    try:
        assert N.lib.tm_debug_flags(-1) == flags, "test hooks not armed"
        split_invariance("fd-dense")
    finally:
        N.lib.tm_debug_flags(old)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 32768])
def test_vocabulary_of_more_than_65536_ids(flags):
    old = N.lib.tm_debug_flags(flags)
    try:
        v, _, _, _ = split_invariance("wide")
        assert v.n_ids() > 65536
    finally:
        N.lib.tm_debug_flags(old)


@pytest.mark.gpu
def test_two_encoders_on_two_threads():
    img = fd_dense_vocab(1)
    v, orc = tm.Vocab(img), Oracle(img)
    docs = [fd_dense_text(np.random.default_rng(9801 + k), 200_000 + 1234 * k) for k in range(2)]
    exps = [orc.tokenize(d) for d in docs]
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def run(k):
        try:
            rng = np.random.default_rng(9811 + k)
            enc = v.encoder(1 << 16)
            parts, pos = [], 0
            gate.wait()
            while pos < len(docs[k]):
                s = int(rng.integers(1, 9000))
                parts.append(enc.feed(docs[k][pos:pos + s]))
                pos += s
            last, missing = enc.finish()
            results[k] = (np.concatenate(parts + [last]), missing)
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
def test_c_example_streams_a_file(tmp_path):
    """examples/tokenize_stream.c reads a file in blocks of 1 MiB and gives the ids examples/tokenize_file.c gives for it as one document"""
    from conftest import example_env
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    img, data = make_case("fd-dense", (1 << 18) + 777 if EMULATED else (3 << 20) + 777)
    (tmp_path / "v.vocab").write_bytes(bytes(img))
    (tmp_path / "t.txt").write_bytes(data)
    whole = subprocess.run([os.path.join(ROOT, "examples", "tokenize_file"), str(tmp_path / "v.vocab"), str(tmp_path / "t.txt")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=example_env())
    assert whole.returncode == 0, whole.stderr.decode(errors="replace")
    exp = np.array(whole.stdout.decode().split(), dtype=np.uint32)
    same((exp, 0), (Oracle(img).tokenize(data)[0], 0), "tokenize_file")
    r = subprocess.run([os.path.join(ROOT, "examples", "tokenize_stream"), str(tmp_path / "v.vocab"), str(tmp_path / "t.txt"), "1", str(tmp_path / "ids.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=example_env())
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    same((np.fromfile(str(tmp_path / "ids.bin"), dtype="<u4"), 0), (exp, 0), "tokenize_stream, ids file")
    r = subprocess.run([os.path.join(ROOT, "examples", "tokenize_stream"), str(tmp_path / "v.vocab"), str(tmp_path / "t.txt"), "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=example_env())
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    same((np.array(r.stdout.decode().split(), dtype=np.uint32), 0), (exp, 0), "tokenize_stream, stdout")


def test_stream_encoder_on_the_emulated_device():
    """the -m gpu tests above on the emulated device (tools/emu: the kernel sources compiled for the host, tests/conftest.py TM_EMU=1)"""
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_stream_encoder.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=3000)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert " passed" in out and " failed" not in out, out[-2000:]

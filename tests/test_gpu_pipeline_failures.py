"""-m gpu: what ships to callers is tm_tokenize_pipeline / tm_tokenize_pipeline_multi (tm_host.hip) - host-side orchestration around kernels the
other modules compare with the oracle.  This module tests the two parts of it nothing else reaches:

 a. the RING on more than one device (page-locked buffers, members 1 - 3 on device 0: one issuer / finisher pair per member, one chunk counter,
    one chain of id counts) against the ORACLE on the host normalizer's text - ids, missing counts, offsets, stats;
 b. a chunk that FAILS, in every form (ring, lanes), on 1 - 3 members, at every place test hook 24 offers (include/tokenmonster_hip.h:
    TM_TEST_FAIL = "<place>:<chunk>:<chunks>"), early, behind a full set of slots and at the end: the call returns TM_E_INPUT with the first
    failure's message, writes nothing behind bytes_cap, and the next calls on the same handles give the oracle's ids, on the ring again.
    The bug these cases were written for is a HANG (a failing chunk of the ring left the issuer waiting for a slot nobody handed back and the
    finisher waiting for the issuer), so every group of cases runs in a child process, every call on a thread under the watchdog of
    tests/test_gpu_multi.py (60 s: a hang detector, no performance claim); the first call that does not return ends its child at once, fails
    the test, and the groups behind it are skipped - nothing more is started on a device after a hang;
 c. a failure that needs no hook: a UTF-16 document cut in half a character (the walk's dead end, tests/test_gpu_exit_maps.py) in a middle
    chunk of the lanes' form with normalized text.  No RING case of this kind is here: ring_supported() would take that vocabulary (it asks for
    capcode and flags only), but the ring takes RAW text, and the normalizer rewrites UTF-16 text (a capcode mark behind every 0 byte in front
    of a letter), so the cut document of the lanes' case does not reach the walk as it is; no raw text that ends in a legitimate TM_E_INPUT /
    TM_E_LIMIT on the ring was found while this module was written (none is known, which is less than none exists).  The way a failing exact
    path takes through the ring's finisher is the hook's place `exact`;
 d. test_pipeline_failures_on_the_emulated_device runs all of it on the emulated device (tools/emu), without a GPU.

On the emulated device the corpora are smaller and the chunk sizes of part a a third of those of tests/test_gpu_host_api.py (so that every
member still gets its four chunks); no case is left out."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":                      # a child of part b: what pytest sets up for the parent (tests/conftest.py: paths, TM_TEST_HOOKS, the emulated device)
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N
from tokenmonster_amd import multi, synth
from tokenmonster_amd.vocab import PipelineStats
from conftest import EMULATED, fuzz_text, fuzz_vocab_tokens
from oracle_bind import Oracle

HOOK = 1 << 24
WATCHDOG = 60
CANARY = 0xA5
TAIL = 4096
RING_VOCAB = dict(capcode=2, norm_flag=1, level=3, seed=0x52494E47)          # the vocabulary of test_ring_equals_single_batch
_hung = []                                      # a call did not return: no further group is started


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the oracle's answer, buffers with a canary behind them, one pipeline call
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _pack(docs):
    raw = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
    roffs = np.zeros(len(docs) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(x) for x in docs])
    return raw, roffs


def _unpack(raw, roffs):
    return [bytes(raw[int(roffs[d]):int(roffs[d + 1])]) for d in range(roffs.size - 1)]


def _oracle(img, text, offs):
    """document by document through the oracle -> (ids of all documents, id offsets, missing counts)"""
    orc = Oracle(img)
    ids, toff, miss = [], np.zeros(offs.size, dtype=np.uint64), np.zeros(offs.size - 1, dtype=np.uint32)
    for d in range(offs.size - 1):
        i, m = orc.tokenize(text[int(offs[d]):int(offs[d + 1])])
        ids.append(i)
        toff[d + 1] = toff[d] + np.uint64(i.size)
        miss[d] = m
    return (np.concatenate(ids) if ids else np.zeros(0, np.uint32)).astype(np.uint32), toff, miss


def _serialized(ids, enc):
    """go/tokenmonster.go:990-1060: little-endian ids of `enc` bytes"""
    return np.ascontiguousarray(ids.astype("<u4").view(np.uint8).reshape(-1, 4)[:, :enc]).reshape(-1)


class Buffers:
    """input and output of one caller, page-locked (the ring) or pageable (the lanes' form); the output has room for exactly `cap` bytes - that
    is the bytes_cap the library is told - and a canary behind them"""

    def __init__(self, raw, cap, pinned):
        self.cap, self.pinned = int(cap), pinned
        if pinned:
            self._pin, self._pout = tm.PinnedBuffer(max(int(raw.size), 16)), tm.PinnedBuffer(self.cap + TAIL)
            self.text, self.whole = self._pin.array[: raw.size], self._pout.array
            self.text[:] = raw
        else:
            self.text, self.whole = raw, np.empty(self.cap + TAIL, dtype=np.uint8)
        self.out = self.whole[: self.cap]

    def arm(self):
        self.whole[:] = CANARY

    def canary_intact(self):
        return bool((self.whole[self.cap:] == CANARY).all())


def _call(vs, buf, roffs, chunk, lanes, width=0, raw=True):
    """tm_tokenize_pipeline_multi as it is, no retry -> (rc, message, byte offsets, missing, encoding length, stats)"""
    nd = roffs.size - 1
    boff = np.full(nd + 1, 0xDEAD, dtype=np.uint64)
    miss = np.zeros(max(nd, 1), dtype=np.uint32)
    enc, stats = C.c_uint32(), PipelineStats()
    rc = N.lib.tm_tokenize_pipeline_multi(vs.handle, N.ptr(buf.text), N.ptr(roffs), nd, 1 if raw else 0, width, chunk, lanes, N.ptr(buf.out), buf.cap,
                                          N.ptr(boff), N.ptr(miss), C.byref(enc), C.byref(stats))
    msg = (N.lib.tm_last_error() or b"").decode(errors="replace") if rc != N.TM_OK else ""
    return rc, msg, boff, miss[:nd], enc.value, {k: getattr(stats, k) for k, _ in PipelineStats._fields_}


def _watched(fn, what):
    """fn() on a thread of its own; None if it has not returned within the watchdog's time"""
    box = {}

    def run():
        try:
            box["r"] = fn()
        except BaseException as ex:          # noqa: B902 (reported by the caller)
            box["r"] = ex
    t = threading.Thread(target=run, daemon=True, name=what)
    t.start()
    t.join(WATCHDOG)
    if t.is_alive():
        return None
    if isinstance(box["r"], BaseException):
        raise box["r"]
    return box["r"]


def _assert_good(res, buf, exp, enc_want, what):
    rc, msg, boff, miss, enc, st = res
    ids, toff, emiss = exp
    assert rc == N.TM_OK, "%s: error %d: %s" % (what, rc, msg)
    assert enc == enc_want, (what, enc)
    assert (boff == toff * np.uint64(enc)).all(), "%s: byte offsets" % what
    assert (miss == emiss).all(), "%s: missing counts" % what
    assert int(boff[-1]) == enc * ids.size and buf.out[: int(boff[-1])].tobytes() == _serialized(ids, enc).tobytes(), "%s: ids differ from the oracle's" % what
    assert buf.canary_intact(), "%s: bytes written behind bytes_cap" % what
    return st


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a. the ring on 1, 2, 3 members against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _ring_parity(members, img, raw, roffs, flag, calls, check_stats):
    """every call of `calls` (chunk bytes, lanes, id width) on the ring of `members` members, twice in a row (the slots are used again), then the
    same through the lanes' form: the oracle's ids on the host normalizer's text, which the one-shot batch call gives as well"""
    text, offs = synth.normalize_batch(raw, roffs, 2, flag)
    exp = _oracle(img, text, offs)
    one_ids, one_toff, one_miss = tm.Vocab(img).tokenize_packed(text, offs)
    assert (one_ids == exp[0]).all() and (one_toff == exp[1]).all() and (one_miss == exp[2]).all()
    g = multi.Devices([0] * members)
    try:
        vs = multi.VocabSet(g, img)
        pinned, pageable = Buffers(raw, 4 * exp[0].size, True), Buffers(raw, 4 * exp[0].size, False)
        for chunk, lanes, width in calls:
            enc = width or 2
            pinned.cap = pageable.cap = enc * exp[0].size          # (bytes_cap: exactly what the ids take)
            pinned.out, pageable.out = pinned.whole[: pinned.cap], pageable.whole[: pageable.cap]
            blobs = []
            for turn in range(2):
                pinned.arm()
                st = _assert_good(_call(vs, pinned, roffs, chunk, lanes, width), pinned, exp, enc, "ring, %d members, chunk %d, turn %d" % (members, chunk, turn))
                assert st["ring"] == 1 and st["chunks"] >= 4 * members and st["lanes"] == members, st
                assert st["input_pinned"] == 1 and st["output_pinned"] == 1 and st["normalized_bytes"] == text.size, st
                check_stats(st)
                blobs.append(pinned.out.tobytes())
            pageable.arm()
            st = _assert_good(_call(vs, pageable, roffs, chunk, lanes, width), pageable, exp, enc, "lanes, %d members, chunk %d" % (members, chunk))
            assert st["ring"] == 0 and st["normalized_bytes"] == text.size, st
            assert blobs[0] == blobs[1] == pageable.out.tobytes()
        vs.close()
    finally:
        g.close()


def _plain_stats(st):
    assert st["ring_exact_chunks"] == 0 and st["host_fallback_docs"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("members", [1, 2, 3])
def test_multi_device_ring_equals_the_oracle(members):
    img = synth.synth_vocab(synth.ENGLISHCODE, 3000, **RING_VOCAB)
    raw, roffs = synth.synth_corpus(synth.ENGLISHCODE, 400_000 if EMULATED else 6_000_000, seed=73)
    z = 3 if EMULATED else 1
    calls = ((30_000 // z, 2, 0), (30_000 // z, 4, 3), (90_000 // z, 3, 4), (9_000 // z, 4, 2))
    _ring_parity(members, img, raw, roffs, 1, calls, _plain_stats)


@pytest.mark.gpu
def test_multi_device_ring_hands_chunks_to_the_exact_path():
    """the documents of test_ring_hands_chunks_to_the_exact_path among plain ones, on three members: whichever member draws such a chunk borrows
    a lane of its own replica for it, and the ids land in document order"""
    img = synth.synth_vocab(synth.ENGLISHCODE, 3000, **RING_VOCAB)
    rng = np.random.default_rng(11)
    docs = _unpack(*synth.synth_corpus(synth.ENGLISHCODE, 400_000, seed=74))
    n0 = len(docs)
    docs.insert(n0 // 5, "𐐀𐐨 Deseret has case beyond the BMP: the host normalizer's 𐐁𐐩 ".encode() * 20)          # a cased script of plane 1: host normalizer
    docs.insert(n0 // 2, b"one long document of plain words that goes on and on " * 3200)           # 170 KB: more than 512 segments
    docs.insert(4 * n0 // 5, b".".join(bytes([65 + int(c)]) for c in rng.integers(0, 26, 9_000)))    # grows 2.5 x under capcode
    docs.append(b"")
    raw, roffs = _pack(docs)

    def stats(st):
        assert 3 <= st["ring_exact_chunks"] < st["chunks"] and st["host_fallback_docs"] == 1, st
    _ring_parity(3, img, raw, roffs, 1, ((20_000, 3, 0), (12_000, 2, 3)), stats)


@pytest.mark.gpu
def test_multi_device_ring_with_byte_level_flags():
    """a vocabulary with every flag of the normalizer (255: the filter pass in front of the normalizer pass), on two members"""
    img0 = synth.synth_vocab(synth.ENGLISHCODE, 3000, **RING_VOCAB)
    img = bytes(img0[:2]) + bytes([255]) + bytes(img0[3:])
    docs = _unpack(*synth.synth_corpus(synth.ENGLISHCODE, 200_000 if EMULATED else 3_000_000, seed=76))
    extra = [b"  Hello   World \r\n", "“Quoted”  café  ‘x’ ".encode(), b"", b" \t ", b"one  two \r\n three\r\n\r\n  four  ",
             ("some  plain  words ‘q’ \r\n" * 40).encode(), b" " * 3000 + b"padded  both   ends\r\n" + b" " * 5000, b"x"]
    for i, e in enumerate(extra):
        docs.insert((i * len(docs)) // len(extra), e)
    raw, roffs = _pack(docs)
    _ring_parity(2, img, raw, roffs, 255, ((25_000 if not EMULATED else 12_000, 3, 0),), _plain_stats)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# b. a chunk fails (test hook 24); the cases run in children of their own
# ---------------------------------------------------------------------------------------------------------------------------------------------
PLACES = {"ring": ("finisher", "exact", "issuer", "download"), "lanes": ("exact", "download")}
REPEATS = 2 if EMULATED else 3                                     # which member draws which chunk is a race: every ring case on several members this many times
FAIL_BYTES = 60_000 if EMULATED else 200_000
FAIL_CHUNK, SIDE_CHUNK = (1_500, 2_100) if EMULATED else (5_000, 7_000)           # chunk bytes of the call under test and of the caller beside it (another count of chunks: the hook's third field leaves it alone)


def _failure_cases(form, members, slots, nchunks):
    """(place, chunk): the first chunk, one with more chunks issued in front of it than all members' slots hold, the last"""
    behind = members * (slots + 2)
    assert behind < nchunks - 1, (behind, nchunks)
    return [(p, k) for p in PLACES[form] for k in (0, behind, nchunks - 1)]


def _child(form, members, slots):
    """one group of part b.  Prints a line per case; on the first call that does not return: which one, and exit code 3 at once."""
    def hang(what):
        print("HANG: %s did not return within %d s" % (what, WATCHDOG), flush=True)
        os._exit(3)

    img = synth.synth_vocab(synth.ENGLISHCODE, 3000, **RING_VOCAB)
    raw, roffs = synth.synth_corpus(synth.ENGLISHCODE, FAIL_BYTES, seed=79, median_doc=512)
    text, offs = synth.normalize_batch(raw, roffs, 2, 1)
    exp = _oracle(img, text, offs)
    cap = 2 * exp[0].size
    g = multi.Devices([0] * members)
    vs = multi.VocabSet(g, img)
    ring = form == "ring"
    main, side = Buffers(raw, cap, ring), Buffers(raw, cap, False)

    def good(what, buf=main, chunk=FAIL_CHUNK):
        buf.arm()
        res = _watched(lambda: _call(vs, buf, roffs, chunk, 2), what)
        if res is None:
            hang(what)
        st = _assert_good(res, buf, exp, 2, what)
        if buf is main:
            assert st["ring"] == (1 if ring else 0) and st["ring_exact_chunks"] == 0, (what, st)      # (the ring's busy flag was released: no silent fall-back to the lanes)
        return st

    nchunks = good("the call without a failure")["chunks"]
    assert good("the caller beside it, alone", side, SIDE_CHUNK)["chunks"] != nchunks
    cases = _failure_cases(form, members, slots, nchunks)
    assert max(k for _, k in cases) >= members * (slots + 2)
    done = 0
    for place, k in cases:
        reps = REPEATS if ring and members > 1 else 1
        for rep in range(reps):
            what = "%s, %d members, %d slots: chunk %d of %d fails at '%s' (try %d)" % (form, members, slots, k, nchunks, place, rep)
            os.environ["TM_TEST_FAIL"] = "%s:%d:%d" % (place, k, nchunks)
            old = N.lib.tm_debug_flags(HOOK)
            try:
                assert N.lib.tm_debug_flags(-1) == HOOK, "test hooks not armed"
                main.arm()
                side.arm()
                beside = {}
                t2 = None
                if rep == 0:                    # a second caller on the same vocabularies, through the lanes, while the first one fails
                    t2 = threading.Thread(target=lambda: beside.update(r=_call(vs, side, roffs, SIDE_CHUNK, 2)), daemon=True)
                    t2.start()
                res = _watched(lambda: _call(vs, main, roffs, FAIL_CHUNK, 2), what)
                if res is None:
                    hang(what)
                if t2 is not None:
                    t2.join(WATCHDOG)
                    if t2.is_alive():
                        hang(what + ": the caller beside it")
            finally:
                N.lib.tm_debug_flags(old)
                del os.environ["TM_TEST_FAIL"]
            rc, msg, boff, _, _, _ = res
            assert rc == N.TM_E_INPUT, "%s: returned %d (%s)" % (what, rc, msg)
            assert "test hook 24" in msg and "chunk %d " % k in msg and "'%s'" % place in msg, "%s: not the first failure's message: %s" % (what, msg)
            assert int(boff[0]) == 0 and main.canary_intact(), what
            if t2 is not None:
                _assert_good(beside["r"], side, exp, 2, what + ": the caller beside it")
            for turn in (1, 2) if rep == reps - 1 else (1,):          # (the next two calls; between the tries of one case, one)
                good("%s: call %d behind it" % (what, turn))
            done += 1
            print("ok: " + what, flush=True)
    vs.close()
    g.close()
    print("all %d failing calls returned; %d cases" % (done, len(cases)), flush=True)


GROUPS = [("ring", m, s) for s in (2, 4) for m in (1, 2, 3)] + [("lanes", m, 4) for m in (1, 2, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,members,slots", GROUPS, ids=["%s-%d-members-%d-slots" % g for g in GROUPS])
def test_a_failing_chunk_returns_its_error_and_leaves_the_handle_whole(form, members, slots):
    if _hung:
        pytest.skip("a pipeline call hung (%s): nothing more is started behind it" % _hung[0])
    env = dict(os.environ, TM_RING_SLOTS=str(slots))      # (read once per process: 4 is the library's default)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, str(members), str(slots)], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    except subprocess.TimeoutExpired as ex:
        _hung.append("%s, %d members, %d slots: the child itself" % (form, members, slots))
        pytest.fail("the child did not end:\n" + (ex.stdout or b"").decode(errors="replace")[-3000:])
    out = r.stdout.decode(errors="replace")
    if "HANG:" in out or r.returncode == 3:
        _hung.append([l for l in out.splitlines() if l.startswith("HANG:")][-1:] or out[-300:])
    assert r.returncode == 0 and "HANG:" not in out, out[-4000:]
    n = len(PLACES[form]) * 3
    assert "all %d failing calls returned; %d cases" % (n * (REPEATS if form == "ring" and members > 1 else 1), n) in out, out[-2000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# c. a failure without a hook: the dead end of a UTF-16 walk in a middle chunk
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _utf16(bs):
    return b"".join(bytes([c, 0]) for c in bs)


DEAD_END = "the walk does not advance on this text"


@pytest.mark.gpu
def test_a_dead_end_in_a_middle_chunk_fails_the_call():
    if _hung:
        pytest.skip("a pipeline call hung (%s): nothing more is started behind it" % _hung[0])
    rng = np.random.default_rng(913)                # the vocabulary of test_utf16_self_successor_is_a_dead_end
    toks8 = fuzz_vocab_tokens(rng, 2, 100)
    toks = sorted(set(_utf16(t) for t in toks8 if len(t) <= 20) | {b"D", b" ", b"a"})
    img = synth.build_vocab(toks, capcode=2, charset=2)
    v = tm.Vocab(img)
    docs = [_utf16(fuzz_text(rng, 2, int(n))) for n in rng.integers(40, 900, 160)]
    text, offs = tm.pack_documents(docs)
    exp = _oracle(img, text, offs)
    chunk = int(text.size) // 12
    # the cut documents: every one tried on its own first; those that meet the dead end go into the middle of the batch, one at a time
    cuts, dead = [_utf16(fuzz_text(rng, 2, n)[:n])[:-1] for n in (300, 700, 1100, 1487, 1500, 1800)], []
    for cut in cuts:
        try:
            v.tokenize_packed(*tm.pack_documents([cut]))
        except N.TokenMonsterHipError as e:
            assert e.code == N.TM_E_INPUT and DEAD_END in str(e)
            dead.append(cut)
    assert dead, "no cut document met the dead end"

    def watched(fn, what):
        res = _watched(fn, what)
        if res is None:
            _hung.append(what)
            pytest.fail(what + " did not return within %d s" % WATCHDOG)
        return res

    for members in (1, 2):
        g = multi.Devices([0] * members)
        try:
            vs = multi.VocabSet(g, img)
            for lanes in (1, 2, 4):
                what = "lanes' form, %d members, %d lanes" % (members, lanes)
                buf = Buffers(text, 2 * exp[0].size, False)
                buf.arm()
                st = _assert_good(watched(lambda: _call(vs, buf, offs, chunk, lanes, raw=False), what), buf, exp, 2, what)
                assert st["chunks"] >= 8 and st["ring"] == 0, st
                for cut in dead[:2]:
                    bad_docs = docs[:80] + [cut] + docs[80:]
                    btext, boffs = tm.pack_documents(bad_docs)
                    bbuf = Buffers(btext, 2 * exp[0].size + 4 * len(cut), False)
                    bbuf.arm()
                    rc, msg, boff, _, _, _ = watched(lambda: _call(vs, bbuf, boffs, chunk, lanes, raw=False), what + ", a cut document")
                    assert rc == N.TM_E_INPUT and DEAD_END in msg, (what, rc, msg)
                    assert int(boff[0]) == 0 and bbuf.canary_intact()
                    buf.arm()
                    _assert_good(watched(lambda: _call(vs, buf, offs, chunk, lanes, raw=False), what + ", behind the failure"), buf, exp, 2, what + ", behind the failure")
            vs.close()
        finally:
            g.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# d. all of the above without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_failures_on_the_emulated_device():
    """the -m gpu tests above on the emulated device (tools/emu: the kernel sources compiled for the host, tests/conftest.py TM_EMU=1)"""
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_pipeline_failures.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=2400)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert " passed" in out and " failed" not in out and " skipped" not in out, out[-2000:]


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        _child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        sys.exit("usage: pytest runs this module; its children are started by its own tests")

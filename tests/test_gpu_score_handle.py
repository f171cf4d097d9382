"""-m gpu: ONE tm_dataset handle driven the way trainvocab drives it (tokenmonster_amd/csrc/tm_score.hip): the dataset is uploaded once and many
candidate vocabularies and strip layouts are scored against it, through every entry point, one pass after the other.  What the handle carries
from pass to pass - the workspace, the grow-only histogram (hist_cap, hist_words) and strip arrays (strip_cap), the cache of the strips' device
state (strips_key) - is exercised with something that CHANGED since the pass before.  The reference of every pass is the oracle's score summed
over the strips (Oracle.score_range for a byte range of one walk), computed once per (vocabulary, layout); every pass compares the whole
histogram, tokens_in_text and the missing set, from output arrays that held a sentinel.  The tests of this file share the handle and run in
the order they stand in: each begins where the one before left it.  tests/test_score_handle_emulated.py runs this file on the emulated
device (tools/emu), without a GPU."""
import ctypes as C

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N
from tokenmonster_amd import multi, synth
from tokenmonster_amd.vocab import PinnedBuffer
from conftest import EMULATED, fuzz_text, fuzz_vocab_tokens
from oracle_bind import Oracle

pytestmark = pytest.mark.gpu

DATA_BYTES = 240_000
LONG_STRIP = 140_001            # more than 512 segments of 256 bytes (128 KiB): the group tree of a long strip
SENTINEL = 0xA5A5A5A5
TAIL = 4 + 256                  # tokens_in_text as four 16-bit limbs | one counter per byte value (include/tokenmonster_hip.h: tm_score_device)
# (name, tokens asked for, capcode, unk token): clearly different numbers of ids, so that the histogram grows and shrinks under one hist_cap
VOCABS = [("v60", 60, 2, False), ("v150", 150, 0, True), ("v400", 400, 2, True), ("v900", 900, 2, False), ("v150b", 150, 0, False)]


class Runtime:
    """the HIP runtime calls a caller of the C ABI makes itself for a stream and a device buffer of its own, looked up THROUGH the library under
    test: a symbol search that begins at a library goes on through what it is linked to, so this is the runtime the library itself calls -
    another copy of it in the process (torch ships one) does not see the library's device.  On the emulated device the calls are tools/emu's,
    which are C++ symbols"""

    def __init__(self):
        L = N.lib
        if EMULATED:
            names = dict(malloc="_Z9hipMallocPPvm", free="_Z7hipFreePv", stream_create="_Z15hipStreamCreatePP9emuStream",
                         stream_sync="_Z20hipStreamSynchronizeP9emuStream", stream_destroy="_Z16hipStreamDestroyP9emuStream")
        else:
            names = dict(malloc="hipMalloc", free="hipFree", stream_create="hipStreamCreate", stream_sync="hipStreamSynchronize", stream_destroy="hipStreamDestroy")
        self.f = {k: getattr(L, n) for k, n in names.items()}
        for k, args in (("malloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("free", [C.c_void_p]), ("stream_create", [C.POINTER(C.c_void_p)]),
                        ("stream_sync", [C.c_void_p]), ("stream_destroy", [C.c_void_p])):
            self.f[k].restype, self.f[k].argtypes = C.c_int, args

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.f["malloc"](C.byref(p), nbytes) == 0 and p.value
        return p

    def free(self, p):
        assert self.f["free"](p) == 0

    def stream(self):
        s = C.c_void_p()
        assert self.f["stream_create"](C.byref(s)) == 0 and s.value
        return s

    def sync(self, s):
        assert self.f["stream_sync"](s) == 0

    def destroy(self, s):
        assert self.f["stream_destroy"](s) == 0


def strips_of(pairs):
    return (np.array([a for a, _ in pairs], dtype=np.uint64), np.array([l for _, l in pairs], dtype=np.uint64))


def layouts(n, rng):
    """name -> list of (offset, length), None = n_strips 0 (the whole dataset)"""
    lay = {"whole": None, "one": [(7, n - 3 - 7)]}
    # two layouts of three strips that share no bound; the second with one length changed by 1
    lay["three_a"] = [(0, 30_000), (40_000, 513), (100_000, n - 100_000)]
    lay["three_b"] = [(11, 20_002), (50_003, 60_000), (150_001, 4_095)]
    lay["three_b1"] = [(11, 20_002), (50_003, 60_001), (150_001, 4_095)]
    # a strip without bytes, moved: to another offset, then to another place among the strips
    lay["zero_a"] = [(0, 1_000), (5_000, 0), (6_000, 70_000), (100_000, n - 100_000)]
    lay["zero_b"] = [(0, 1_000), (5_500, 0), (6_000, 70_000), (100_000, n - 100_000)]
    lay["zero_c"] = [(0, 1_000), (6_000, 70_000), (5_500, 0), (100_000, n - 100_000)]
    # one strip that is a byte range of tm_score_begin as well: the two differ only in how far the walk may look
    lay["r1"] = [(1_000, 89_000)]
    lay["r2"] = [(90_000, n - 50 - 90_000)]
    # trainvocab's own rule (training/trainvocab.go:1668-1695) at strips = 100, percentage = 15: bytesPerStrip rounded up to a multiple of 4,
    # offsets dataLen / strips apart from a random start, wrapped at the end of the data
    for name, seed in (("train100", 1), ("train100b", 2)):
        strips = 100
        per = (n * 15 // 100) // strips
        per += 4 - per % 4
        step = n // strips
        assert step + per <= n
        frm = int(np.random.default_rng(seed).integers(0, step))
        t = []
        for _ in range(strips):
            if frm + per > n:
                frm = frm + per - n
            t.append((frm, per))
            frm += step
        lay[name] = t
    assert {a for a, _ in lay["train100"]}.isdisjoint({a for a, _ in lay["train100b"]})
    # about a thousand short strips between sorted random cuts, a fifth of them empty, a few of one byte
    cuts = np.unique(rng.integers(0, n, size=1_000))
    t = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = rng.random()
        t.append((int(a), 0 if r < 0.2 else 1 if r < 0.25 else int(b - a) if r < 0.6 else int(rng.integers(0, b - a + 1))))
    assert len(t) > 900 and sum(1 for _, l in t if l == 0) > 100
    lay["thousand"] = t
    # a strip of more than 512 segments with short strips in front of it and behind it
    lay["long_mid"] = [(0, 255), (300, 256), (1_000, 257), (2_000, LONG_STRIP), (150_000, 1), (150_010, 0), (160_000, 4_096), (n - 5, 5)]
    lay["long_mid_b"] = [(0, 255), (300, 256), (1_000, 257), (2_001, LONG_STRIP), (150_000, 1), (150_010, 0), (160_000, 4_096), (n - 5, 5)]
    for name, t in lay.items():
        if t and len(t) > 1:
            iv = sorted((a, a + l) for a, l in t if l)
            assert all(x[1] <= y[0] for x, y in zip(iv, iv[1:])) and iv[-1][1] <= n, name
    return lay


class Handle:
    """the dataset, the candidates and their oracles, the expected results, a stream and a device buffer of the caller"""

    def __init__(self):
        rng = np.random.default_rng(660_001)
        self.data = np.frombuffer(fuzz_text(rng, 2, DATA_BYTES), dtype=np.uint8)
        self.n = int(self.data.size)
        self.images, self.oracles, self.vocabs = {}, {}, {}
        for name, ntok, capcode, unk in VOCABS:
            self.images[name] = synth.build_vocab(fuzz_vocab_tokens(rng, capcode, ntok), capcode=capcode, charset=1, with_unk=unk)
            self.oracles[name] = Oracle(self.images[name])
        sizes = [self.oracles[name].n_ids() for name, *_ in VOCABS[:4]]
        assert all(b > 1.8 * a for a, b in zip(sizes, sizes[1:])), sizes
        self.lay = layouts(self.n, rng)
        self._expected = {}
        self.rt = Runtime()
        self.stream = self.rt.stream()
        self.ds = self.upload(self.data)
        self.passes = 0

    def upload(self, data, on=None):
        ds = C.c_void_p()
        if on is None:
            N.check(N.lib.tm_dataset_upload(N.ptr(data), data.size, C.byref(ds)))
        else:
            N.check(N.lib.tm_dataset_upload_on(N.ptr(data), data.size, on, C.byref(ds)))
        return ds

    def vocab(self, name):
        if name not in self.vocabs:
            self.vocabs[name] = tm.Vocab(self.images[name])
        return self.vocabs[name]

    def free_vocab(self, name):
        self.vocabs.pop(name).close()

    def expected(self, vname, lname, data=None, key=None):
        """the oracle's score of every strip by itself, summed -> (scores u64[n_ids], tokens_in_text, missing set u8[32]); computed once"""
        key = key or (vname, lname)
        if key not in self._expected:
            data = self.data if data is None else data
            orc = self.oracles[vname]
            strips = self.lay[lname] if isinstance(lname, str) else lname
            s = np.zeros(orc.n_ids(), dtype=np.uint64)
            t, m = 0, np.zeros(32, dtype=np.uint8)
            for a, l in ([(0, int(data.size))] if strips is None else strips):
                s_, t_, m_ = orc.score(data[a:a + l])
                s += s_
                t += t_
                m |= m_
            s.setflags(write=False)
            m.setflags(write=False)
            self._expected[key] = (s, t, m)
        return self._expected[key]

    def expected_range(self, vname, lo, hi, entry):
        key = (vname, "range", lo, hi, entry)
        if key not in self._expected:
            s, t, m, ex = self.oracles[vname].score_range(self.data, lo, hi, entry)
            self._expected[key] = (s.astype(np.uint64), t, m, ex)
        return self._expected[key]

    # ---- the entry points: each -> (scores, tokens_in_text, missing set) from outputs that held a sentinel ---------------------------------
    def outputs(self, v):
        return np.full(v.n_ids(), SENTINEL, dtype=np.uint32), C.c_uint64(0xDEADBEEFDEADBEEF), np.full(32, 0xA5, dtype=np.uint8)

    def args(self, strips):
        if strips is None:
            return None, None, 0, ()
        so, sl = strips_of(strips)
        return N.ptr(so), N.ptr(sl), len(strips), (so, sl)

    def read(self, v, ds):
        s, t, m = self.outputs(v)
        N.check(N.lib.tm_score_read(v.handle, ds, N.ptr(s), C.byref(t), N.ptr(m)))
        return s, int(t.value), m

    def score(self, v, ds, strips):
        s, t, m = self.outputs(v)
        po, pl, k, keep = self.args(strips)
        N.check(N.lib.tm_score(v.handle, ds, po, pl, k, N.ptr(s), C.byref(t), N.ptr(m)))
        return s, int(t.value), m

    def score_device(self, v, ds, strips):
        po, pl, k, keep = self.args(strips)
        hist, words = C.c_void_p(), C.c_uint64()
        N.check(N.lib.tm_score_device(v.handle, ds, po, pl, k, self.stream, C.byref(hist), C.byref(words)))
        self.rt.sync(self.stream)
        assert hist.value and words.value == v.n_ids() + TAIL
        got = self.read(v, ds)
        # the words in HBM, as a rank would hand them to an all-reduce
        assert np.array_equal(self.fetch(hist, words.value), self.words(got))
        return got

    def score_into(self, v, ds, strips, short=0):
        """tm_score_device_into a device buffer of exactly n_ids + 260 words (`short` words fewer: TM_E_NOSPACE) between guard words"""
        words = v.n_ids() + TAIL
        guard = 8
        dst = self.rt.malloc((words + 2 * guard) * 4)
        try:
            pin = PinnedBuffer((words + 2 * guard) * 4)
            pin.array.view(np.uint32)[:] = SENTINEL
            N.check(N.lib.tm_device_copy(dst, C.c_void_p(pin.array.ctypes.data), pin.array.size))
            po, pl, k, keep = self.args(strips)
            rc = N.lib.tm_score_device_into(v.handle, ds, po, pl, k, self.stream, C.c_void_p(dst.value + 4 * guard), words - short)
            self.rt.sync(self.stream)
            w = self.fetch(dst, words + 2 * guard)
            assert (w[:guard] == SENTINEL).all() and (w[guard + words:] == SENTINEL).all()
            if short:
                assert rc == N.TM_E_NOSPACE and (w == SENTINEL).all()
                return None
            N.check(rc)
            w = w[guard:guard + words]
        finally:
            self.rt.free(dst)
        n_ids = v.n_ids()
        # the layout the header states: scores | tokens_in_text as four 16-bit limbs | one counter per byte value, > 0 = that byte had no token
        assert (w[n_ids:n_ids + 4] < 65536).all()
        t = sum(int(w[n_ids + k]) << (16 * k) for k in range(4))
        m = np.packbits(w[n_ids + 4:] > 0, bitorder="little")
        got = self.read(v, ds)
        assert np.array_equal(w, self.words(got))
        return w[:n_ids].copy(), t, m

    def score_range(self, v, ds, lo, hi, continues, entry, into=False):
        """tm_score_begin + tm_score_finish from `entry` + tm_score_read -> (scores, tokens_in_text, missing set, the range's exit map)"""
        ex = np.full(80, 0xA5, dtype=np.uint8)
        N.check(N.lib.tm_score_begin(v.handle, ds, lo, hi - lo, continues, self.stream, N.ptr(ex)))
        self.rt.sync(self.stream)
        if not into:
            N.check(N.lib.tm_score_finish(v.handle, ds, entry, self.stream, None, 0))
            self.rt.sync(self.stream)
            return self.read(v, ds) + (ex,)
        words = v.n_ids() + TAIL                       # ... with the histogram copied into a device buffer of the caller's, as tm_score_device_into does
        dst = self.rt.malloc(words * 4)
        try:
            N.check(N.lib.tm_score_finish(v.handle, ds, entry, self.stream, dst, words))
            self.rt.sync(self.stream)
            w = self.fetch(dst, words)
        finally:
            self.rt.free(dst)
        got = self.read(v, ds)
        assert np.array_equal(w, self.words(got))
        return got + (ex,)

    def fetch(self, dev, words):
        pin = PinnedBuffer(int(words) * 4)
        N.check(N.lib.tm_device_copy(C.c_void_p(pin.array.ctypes.data), dev, pin.array.size))
        return pin.array.view(np.uint32).copy()

    @staticmethod
    def words(got):
        """(scores, tokens_in_text, missing set) -> the n_ids + 260 words of the device form"""
        s, t, m = got
        limbs = [(t >> (16 * k)) & 0xFFFF for k in range(4)]
        return np.concatenate([s, np.array(limbs, dtype=np.uint32), np.unpackbits(m, bitorder="little").astype(np.uint32)])

    # ---- one pass and its check ----------------------------------------------------------------------------------------------------------
    def check(self, got, exp, what):
        s, t, m = got
        assert s.dtype == np.uint32 and not (s == SENTINEL).any(), what          # scores is overwritten
        bad = np.nonzero(s != exp[0])[0]
        assert bad.size == 0, "%s: %d of %d scores differ, first at id %d: %d != %d" % (what, bad.size, s.size, bad[0], s[bad[0]], exp[0][bad[0]])
        assert t == exp[1], "%s: tokens_in_text %d != %d" % (what, t, exp[1])
        assert np.array_equal(m, exp[2]), "%s: missing set" % (what,)

    def step(self, vname, lname, how="score", ds=None):
        self.passes += 1
        v = self.vocab(vname)
        strips = self.lay[lname]
        got = {"score": self.score, "device": self.score_device, "into": self.score_into}[how](v, ds or self.ds, strips)
        self.check(got, self.expected(vname, lname), "pass %d: %s on %s through %s" % (self.passes, vname, lname, how))

    def close(self):
        for v in self.vocabs.values():
            v.close()
        N.lib.tm_dataset_free(self.ds)
        self.rt.destroy(self.stream)


@pytest.fixture(scope="module")
def h():
    x = Handle()
    yield x
    x.close()


def run(h, steps):
    for s in steps:
        h.step(*s)


# ---- 1. candidates on unchanged strips ------------------------------------------------------------------------------------------------------
def test_candidates_on_unchanged_strips(h):
    """small -> large (the histogram grows), large -> small (hist_words shrinks under one hist_cap: no stale tail), the same vocabulary twice
    (the cache hit), on the whole dataset and on trainvocab's 100 strips; the candidates differ in capcode and in having an unk token"""
    for lname in ("whole", "train100"):
        run(h, [("v60", lname), ("v150", lname), ("v400", lname), ("v900", lname), ("v900", lname), ("v400", lname), ("v60", lname), ("v60", lname),
                ("v900", lname, "device"), ("v150b", lname, "device"), ("v150", lname, "into"), ("v900", lname, "into"), ("v60", lname, "into")])


def test_a_vocabulary_freed_and_another_loaded_between_passes(h):
    run(h, [("v400", "three_a")])
    h.free_vocab("v400")
    run(h, [("v150", "three_a")])                  # (loaded into what v400 left behind)
    h.free_vocab("v150")
    h.free_vocab("v900")
    run(h, [("v900", "three_a"), ("v400", "three_a"), ("v150", "three_a")])


def test_tuning_between_two_passes_changes_no_id(h):
    """tm_vocab_tune lays the tables out by use on a sample: the ids, hence the histogram, stay what they were"""
    for sample in (h.data[:50_000], h.data[100_000:], h.data[:0]):
        run(h, [("v900", "train100b")])
        h.vocab("v900").tune(sample)
        run(h, [("v900", "train100b"), ("v400", "train100b")])


# ---- 2. layouts changing under one vocabulary, and under changing vocabularies ---------------------------------------------------------------
def test_bounds_change_while_the_number_of_strips_stays(h):
    """the cache of the strips' device state must tell two layouts of as many strips apart: whole <-> [7, n - 3), two three-strip layouts
    without a common bound, one length changed by 1, an empty strip moved, trainvocab's 100 strips from two starting points, a long strip
    moved by one byte"""
    seq = [("whole",), ("one",), ("whole",), ("one",), ("r1",), ("r2",), ("one",),
           ("three_a",), ("three_b",), ("three_b1",), ("three_b",), ("three_a",),
           ("zero_a",), ("zero_b",), ("zero_c",), ("zero_a",),
           ("train100",), ("train100b",), ("train100",),
           ("long_mid",), ("long_mid_b",), ("long_mid",)]
    for k, (lname,) in enumerate(seq):
        h.step("v400", lname, ("score", "device", "into")[k % 3])
    # ... and with another candidate at every step
    names = ["v900", "v60", "v150", "v400", "v150b"]
    for k, (lname,) in enumerate(seq):
        h.step(names[k % len(names)], lname, ("into", "score", "device")[k % 3])


def test_the_number_of_strips_grows_and_shrinks(h):
    """3 -> 100 -> about 1 000 strips (the workspace and the strip arrays are made again), back to 1, and up again; a strip of more than 512
    segments before and after short ones"""
    run(h, [("v150", "three_a"), ("v150", "train100"), ("v150", "thousand"), ("v900", "thousand", "device"), ("v150", "whole"), ("v60", "one", "into"),
            ("v60", "thousand", "into"), ("v400", "long_mid"), ("v400", "thousand"), ("v400", "long_mid", "device"), ("v400", "three_b"), ("v400", "train100b", "into"),
            ("v400", "long_mid"), ("v900", "whole", "device")])


def test_a_fresh_handle_begins_with_a_thousand_strips(h):
    """the strip arrays of a new handle are made for its first layout, the largest here; a smaller one follows"""
    ds = h.upload(h.data)
    try:
        run(h, [("v150", "thousand", "into", ds), ("v900", "train100", "score", ds), ("v150", "thousand", "device", ds), ("v60", "whole", "score", ds)])
    finally:
        N.lib.tm_dataset_free(ds)


# ---- 3. every entry point on the same handle, interleaved --------------------------------------------------------------------------------------
def test_a_destination_one_word_short_is_refused_and_the_next_pass_is_correct(h):
    for vname, lname in (("v400", "three_b"), ("v60", "thousand")):
        assert h.score_into(h.vocab(vname), h.ds, h.lay[lname], short=1) is None
        assert "destination holds" in N.lib.tm_last_error().decode()
        run(h, [(vname, lname, "into"), ("v900", lname, "score")])


@pytest.mark.parametrize("vname", ["v400", "v150"])
def test_byte_ranges_of_one_walk_between_strip_passes(h, vname):
    """tm_score_begin / tm_score_finish over [1 000, 90 000) with more text behind it (continues = 1) and over [90 000, n - 50) whose following
    text ends inside the halo (continues = 2), each between two passes over the SAME bytes as a strip: the range may look to the end of the
    dataset, the strip ends with itself, and the cached strips must tell the two apart.  The second range is entered in the state the
    first one leaves."""
    v, orc = h.vocab(vname), h.oracles[vname]
    lo1, hi1 = h.lay["r1"][0][0], sum(h.lay["r1"][0])
    lo2, hi2 = h.lay["r2"][0][0], sum(h.lay["r2"][0])
    assert hi1 == lo2 and h.n - hi1 >= 128 and 0 < h.n - hi2 < 128
    h.step(vname, "r1", "device")
    e1 = h.expected_range(vname, lo1, hi1, 0)
    s, t, m, ex1 = h.score_range(v, h.ds, lo1, hi1, 1, 0)
    h.check((s, t, m), e1, "%s: range [%d, %d) continues 1" % (vname, lo1, hi1))
    assert int(ex1[0]) == e1[3]
    if vname == "v400":      # (for this candidate the cut falls inside a token: the strip over the same bytes, which stops at its end, is another walk)
        assert not np.array_equal(e1[0], h.expected(vname, "r1")[0]) and e1[3] != 0
    h.step(vname, "r1", "score")
    h.step(vname, "r2", "into")
    entry = int(ex1[0])
    e2 = h.expected_range(vname, lo2, hi2, entry)
    s, t, m, ex2 = h.score_range(v, h.ds, lo2, hi2, 2, entry, into=True)
    h.check((s, t, m), e2, "%s: range [%d, %d) continues 2 from state %d" % (vname, lo2, hi2, entry))
    assert int(ex2[entry]) == e2[3]
    h.step(vname, "r2", "device")
    # the same range twice (the cache hit of a range), then as a strip, then the other candidate on the range
    for _ in range(2):
        s, t, m, _ = h.score_range(v, h.ds, lo1, hi1, 1, 0)
        h.check((s, t, m), e1, "%s: range again" % vname)
    h.step("v900", "r1", "into")
    s, t, m, _ = h.score_range(h.vocab("v900"), h.ds, lo1, hi1, 1, 0)
    h.check((s, t, m), h.expected_range("v900", lo1, hi1, 0), "v900: range after its strip")
    h.step("v900", "whole", "score")


# ---- 4. errors do not stick ---------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_the_handle_as_good_as_before(h):
    v = h.vocab("v400")
    s, t, m = h.outputs(v)

    def refused(strips):
        so, sl = strips_of(strips)
        assert N.lib.tm_score(v.handle, h.ds, N.ptr(so), N.ptr(sl), len(strips), N.ptr(s), C.byref(t), N.ptr(m)) == N.TM_E_INVALID
        hist, words = C.c_void_p(), C.c_uint64()
        assert N.lib.tm_score_device(v.handle, h.ds, N.ptr(so), N.ptr(sl), len(strips), h.stream, C.byref(hist), C.byref(words)) == N.TM_E_INVALID
        h.rt.sync(h.stream)

    run(h, [("v400", "three_b")])
    refused([(11, 20_002), (20_012, 60_000), (150_001, 4_095)])               # overlapping strips
    assert "overlap" in N.lib.tm_last_error().decode()
    run(h, [("v400", "three_b", "device"), ("v400", "three_a")])
    refused([(0, 30_000), (40_000, 513), (100_000, h.n - 100_000 + 1)])       # a strip that ends behind the dataset
    assert "outside" in N.lib.tm_last_error().decode()
    run(h, [("v400", "three_a", "into")])
    refused([(0, 30_000), (h.n + 1, 0), (100_000, 5)])                        # ... and one that begins there
    run(h, [("v60", "three_a"), ("v400", "three_b")])
    # tm_score_finish without tm_score_begin - also right behind a complete pass, and behind a refused begin
    assert N.lib.tm_score_finish(v.handle, h.ds, 0, h.stream, None, 0) == N.TM_E_INVALID
    ex = np.zeros(80, dtype=np.uint8)
    assert N.lib.tm_score_begin(v.handle, h.ds, 1_000, h.n - 1_000 - 50, 1, h.stream, N.ptr(ex)) == N.TM_E_INVALID      # continues = 1 without 128 bytes behind it
    assert N.lib.tm_score_finish(v.handle, h.ds, 0, h.stream, None, 0) == N.TM_E_INVALID
    h.rt.sync(h.stream)
    run(h, [("v400", "three_b", "device"), ("v900", "one")])


def test_a_pass_that_ends_in_an_input_error_on_the_device(h):
    """the UTF-16 vocabulary and text of test_utf16_cut_character_ends_the_walk_with_an_error (tests/test_gpu_parity.py) as a dataset of its
    own: the pass returns TM_E_INPUT - a returned code, the device has seen no fault - and a UTF-8 candidate on the same handle is scored
    as on a fresh one"""
    from test_gpu_parity import _utf16
    rng = np.random.default_rng(913)
    toks8 = fuzz_vocab_tokens(rng, 2, 100)
    img = synth.build_vocab(sorted(set(_utf16(t) for t in toks8 if len(t) <= 20) | {b"D", b" ", b"a"}), capcode=2, charset=2)
    docs = []
    for n in rng.integers(0, 1800, size=40):
        doc = _utf16(fuzz_text(rng, 2, int(n)))
        docs.append(doc[:-1] if n % 3 == 0 else doc)
    bad = [d for d in docs if len(d) == 2975]
    assert len(bad) == 1
    text = np.frombuffer(bad[0], dtype=np.uint8)
    v16 = tm.Vocab(img)
    ds = h.upload(text)
    try:
        lay = {"whole": None, "two": [(0, 1_000), (1_001, text.size - 1_001)]}
        for vname, lname in (("v150", "whole"), ("v400", "two")):
            s, t, m = h.outputs(v16)
            assert N.lib.tm_score(v16.handle, ds, None, None, 0, N.ptr(s), C.byref(t), N.ptr(m)) == N.TM_E_INPUT
            for how in (h.score, h.score_device, h.score_into):
                got = how(h.vocab(vname), ds, lay[lname])
                h.check(got, h.expected(vname, lay[lname], data=text, key=(vname, "utf16", lname)), "%s on the text of the input error, %s" % (vname, lname))
        # ... through the device form: the error is the read's
        hist, words = C.c_void_p(), C.c_uint64()
        N.check(N.lib.tm_score_device(v16.handle, ds, None, None, 0, h.stream, C.byref(hist), C.byref(words)))
        h.rt.sync(h.stream)
        s, t, m = h.outputs(v16)
        assert N.lib.tm_score_read(v16.handle, ds, N.ptr(s), C.byref(t), N.ptr(m)) == N.TM_E_INPUT
        h.check(h.score(h.vocab("v60"), ds, None), h.expected("v60", None, data=text, key=("v60", "utf16", "whole")), "v60 behind the input error")
    finally:
        N.lib.tm_dataset_free(ds)
        v16.close()


# ---- 5. two datasets, one vocabulary ---------------------------------------------------------------------------------------------------------------
def test_two_datasets_take_turns_under_one_vocabulary(h):
    """the second dataset - other bytes, uploaded with tm_dataset_upload_on(..., 0, ...) - keeps its own state: what one handle caches is never
    taken for the other's"""
    other = np.ascontiguousarray(h.data[::-1][: h.n - 20_000])
    ds = h.upload(other, on=0)
    try:
        assert N.lib.tm_dataset_device(ds) == 0 and N.lib.tm_dataset_device(h.ds) == 0
        for k, name in enumerate(("three_a", "three_b", "three_b", "whole", "one", "train100", "whole")):
            how = ("score", "device", "into")[k % 3]
            vname = ("v400", "v900")[k & 1]
            strips = h.lay[name]
            if strips is not None:
                strips = [(a, min(l, other.size - a)) for a, l in strips if a < other.size]       # (the other dataset is 20 000 bytes shorter)
            h.step(vname, name, how)
            got = {"score": h.score, "device": h.score_device, "into": h.score_into}[how](h.vocab(vname), ds, strips)
            h.check(got, h.expected(vname, strips, data=other, key=(vname, "other", name)), "%s on %s of the second dataset" % (vname, name))
    finally:
        N.lib.tm_dataset_free(ds)


# ---- 6. the in-library multi-device form ---------------------------------------------------------------------------------------------------------
def test_one_dataset_set_scored_with_three_vocabulary_sets(h):
    """tm_score_multi on 3 virtual members (tests/test_gpu_multi.py): one DatasetSet, candidates small, large, small - every member's dataset
    handle sees the histogram grow and shrink"""
    g = multi.Devices([0, 0, 0])
    try:
        ds = multi.DatasetSet(g, h.data)
        for vname in ("v60", "v900", "v60", "v400"):
            vs = multi.VocabSet(g, h.images[vname])
            for _ in range(2):
                s, t, m = ds.score(vs)
                h.check((s, t, m), h.expected(vname, "whole"), "%s on three members" % vname)
            vs.close()
        ds.close()
    finally:
        g.close()

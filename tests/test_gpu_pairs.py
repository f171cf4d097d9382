"""-m gpu: text pairs as fixed-shape rows - tm_batch_pair / tm_batch_pair_spans_in / tm_batch_pair_window_rows / tm_batch_pair_windows /
tm_batch_pair_windows_spans_in (tokenmonster_amd/csrc/tm_pairs.hip) at the C ABI, outputs in tm_host_alloc memory behind sentinels, against a
numpy statement of the rule of include/tokenmonster_hip.h.  The ids and the ragged pairs come from tm_batch_download and tm_batch_spans_in of the
same run: this file tests layout, not tokenization.  tests/test_pairs_emulated.py runs this file on the emulated device (tools/emu), without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth
from fixed_shape import Collate, Out, DT, FILL, KEEP_TAIL, NONE, PAD_LEFT

ROW_LENS = [1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 257]
SPAN_LENS = [1, 4, 9, 65]
WINDOW_LENS = [2, 3, 5, 8, 9, 64, 65]
LONGEST, ONLY_FIRST, ONLY_SECOND = 0, 1, 2
TRUNCS = (LONGEST, ONLY_FIRST, ONLY_SECOND)
# (text, unit) of the span forms: normalized bytes, raw bytes, raw code points, normalized UTF-16 units
FORMS = [((0, 0), 4), ((1, 0), 8), ((1, 1), 4), ((0, 2), 8)]
EMPTY_RUN = 16          # (sixteen rows in a row hold a whole 16-byte vector of two-byte ids wherever the run begins)
pytestmark = pytest.mark.gpu


class Pair(C.Structure):
    """tm_pair"""
    _fields_ = [(n, C.c_uint32) for n in ("first_a", "first_b", "npairs", "row_len", "id_bytes", "pad_id", "bos_id", "sep_id", "eos_id", "sep_count", "truncation", "flags")]


def specials(L):
    """every (bos?, separators, eos?) that leaves R >= 0 at row length L -> list of (has_bos, nsep, has_eos, R)"""
    return [(hb, ns, he, L - hb - ns - he) for hb in (0, 1) for ns in (0, 1, 2) for he in (0, 1) if L - hb - ns - he >= 0]


def side_lengths(R):
    h = R // 2
    return sorted({n for n in (0, 1, h - 1, h, h + 1, R - h, R - 1, R, R + 1, 2 * R + 1) if n >= 0})


# ---- the rule, in numpy --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kept_counts(a, b, R, trunc):
    if a + b <= R:
        return a, b
    if trunc == LONGEST:                 # one id at a time from the side that is longer, from A on a tie
        while a + b > R:
            if a >= b:
                a -= 1
            else:
                b -= 1
        return a, b
    if trunc == ONLY_SECOND:
        ka = min(a, R)
        return ka, min(b, R - ka)
    kb = min(b, R)
    return min(a, R - kb), kb


class Rows:
    """the outputs of a pair call, built row by row: [bos] A [sep]* B [eos], then padding"""

    def __init__(self, rows, L, pad, bos, sep, nsep, eos, pad_left, with_spans):
        self.ids = np.full((rows, L), pad, dtype=np.uint64)
        self.mask = np.zeros((rows, L), dtype=np.uint8)
        self.types = np.zeros((rows, L), dtype=np.uint8)
        self.kept = np.zeros((rows, 2), dtype=np.uint32)
        self.spans = np.zeros((rows, L, 2), dtype=np.int64) if with_spans else None
        self.content = np.zeros((rows, L), dtype=bool)
        self.head = [bos] if bos is not None else []
        self.seps = [sep] * nsep
        self.tail = [eos] if eos is not None else []
        self.L, self.pad_left = L, pad_left

    def put(self, r, A, B, sa=None, sb=None):
        row = self.head + list(A) + self.seps + list(B) + self.tail
        assert len(row) <= self.L
        lo = self.L - len(row) if self.pad_left else 0
        a0 = lo + len(self.head)
        b0 = a0 + len(A) + len(self.seps)
        self.ids[r, lo:lo + len(row)] = row
        self.mask[r, lo:lo + len(row)] = 1
        self.types[r, b0:lo + len(row)] = 1
        self.kept[r] = (len(A), len(B))
        self.content[r, a0:a0 + len(A)] = True
        self.content[r, b0:b0 + len(B)] = True
        if self.spans is not None:
            self.spans[r, a0:a0 + len(A)] = sa
            self.spans[r, b0:b0 + len(B)] = sb

    def freeze(self):
        for x in vars(self).values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        return self


def np_pairs(A, B, L, pad, bos, sep, nsep, eos, trunc, pad_left, SA=None, SB=None):
    """A, B: lists of id arrays (SA, SB: [n, 2] arrays beside them) -> Rows"""
    R = L - (bos is not None) - nsep - (eos is not None)
    out = Rows(len(A), L, pad, bos, sep, nsep, eos, pad_left, SA is not None)
    for p, (x, y) in enumerate(zip(A, B)):
        ka, kb = kept_counts(len(x), len(y), R, trunc)
        out.put(p, x[:ka], y[:kb], SA[p][:ka] if SA is not None else None, SB[p][:kb] if SB is not None else None)
    return out.freeze()


def n_windows(n, room, step):
    return 1 if n <= room else 1 + -(-(n - room) // step)


def np_pair_windows(A, B, L, pad, bos, sep, nsep, eos, overlap, max_first, pad_left, SA=None, SB=None):
    """-> Rows with row_pair and row_start: row k of pair p is [bos] A[:a'] [sep]* B[k * step_p : k * step_p + room_p] [eos]"""
    R = L - (bos is not None) - nsep - (eos is not None)
    assert max_first <= R and R - max_first > overlap
    plan = []
    for p, (x, y) in enumerate(zip(A, B)):
        room = R - min(len(x), max_first)
        plan += [(p, k * (room - overlap), room) for k in range(n_windows(len(y), room, room - overlap))]
    out = Rows(len(plan), L, pad, bos, sep, nsep, eos, pad_left, SA is not None)
    for r, (p, s, room) in enumerate(plan):
        ka = min(len(A[p]), max_first)
        out.put(r, A[p][:ka], B[p][s:s + room], SA[p][:ka] if SA is not None else None, SB[p][s:s + room] if SB is not None else None)
    out.row_pair = np.array([p for p, _, _ in plan], dtype=np.uint32)
    out.row_start = np.array([s for _, s, _ in plan], dtype=np.uint32)
    return out.freeze()


# ---- one vocabulary, one run for the whole file -----------------------------------------------------------------------------------------
LETTERS = b"abcdefghijklmnopqrst"


def vocab_tokens():
    """every letter a..t, the capcode markers and some punctuation are tokens of one byte, and no longer token is made of those letters alone: a
    document of n of those letters is n ids, each the id of its letter.  'x' and 'y' have no token (one unk id each); the longer tokens
    are for the raw documents"""
    toks = {bytes([c]) for c in LETTERS + b" .,'\nDCW"}
    toks |= {" zz".encode(), b"zzu", b"uz", b" zu", b"D zz", b"zu z", "é".encode(), "́".encode(), "ź".encode()}
    return sorted(toks)


class Env:
    def __init__(self):
        rng = np.random.default_rng(88002)
        self.v = tm.Vocab(synth.build_vocab(vocab_tokens(), capcode=2, charset=1, norm_flag=1, with_unk=True))
        n_ids = self.v.n_ids()
        self.pad, self.bos, self.sep, self.eos = n_ids + 5, n_ids + 6, n_ids + 7, n_ids + 8          # (no document holds them)
        assert self.eos < 65536

        def letters(n):
            """n letters, no two neighbours alike"""
            a = rng.integers(0, len(LETTERS), size=n)
            for i in range(1, n):
                if a[i] == a[i - 1]:
                    a[i] = (a[i] + 1 + i % 7) % len(LETTERS)
            return bytes(LETTERS[int(x)] for x in a)

        docs = []
        self.groups = {}          # name -> (first_a, first_b, npairs)
        self.lengths = {}         # R -> the (a, b) of the group's pairs

        def group(name, la, lb):
            self.groups[name] = (len(docs), len(docs) + len(la), len(la))
            docs.extend([letters(n) for n in la] + [letters(n) for n in lb])

        # for every R any shape has: the side lengths crossed, A's in one block of documents and B's in the block behind it
        for R in sorted({R for L in ROW_LENS for _, _, _, R in specials(L)}):
            S = side_lengths(R)
            self.lengths[R] = [(a, b) for a in S for b in S]
            group(("cross", R), [a for a, _ in self.lengths[R]], [b for _, b in self.lengths[R]])
        # what the normalizer changes (capitals, a two-byte letter, a four-byte character: UTF-16 differs from code points), short random
        # documents, and a run of pairs of empty documents in the middle and at the end
        special_docs = ["Hello WORLD zzé Éa zu zzu".encode(), "aBé cD".encode() * 6, b"x", b"xay" * 5, "É".encode() + letters(30) + b" ZZU", "ab😀cd é😀".encode(),
                        "Zu 😀 zzu Éé".encode() * 3]
        half = []
        for side in range(2):
            blk = list(special_docs) if side == 0 else list(reversed(special_docs))
            blk += [letters(int(n)) for n in rng.integers(0, 40, size=20)] + [b""] * EMPTY_RUN
            blk += [letters(int(n)) for n in rng.integers(0, 40, size=24)] + ["é😀".encode() + letters(5)] + [b""] * EMPTY_RUN
            half.append(blk)
        self.groups["mixed"] = (len(docs), len(docs) + len(half[0]), len(half[0]))
        self.mixed_empty = (len(special_docs) + 20, len(half[0]) - EMPTY_RUN)          # where the two runs of empty pairs begin
        docs += half[0] + half[1]
        # windows: a short and a long A against every length of B around every room and room + step of the shapes tested
        small_a, small_b = [0, 1, 2, 12], list(range(0, 31))
        group("win_small", [a for a in small_a for _ in small_b], [b for _ in small_a for b in small_b])
        big_a, big_b = [0, 1, 70], list(range(0, 6)) + list(range(54, 136))
        group("win_big", [a for a in big_a for _ in big_b], [b for _ in big_a for b in big_b])
        self.raw = docs
        assert sum(len(d) for d in docs) < (1 << 20) and max(len(d) for d in docs) <= 1500
        self.b = self.new_batch(1 << 20, len(docs) + 8)
        self.run_raw(self.b, docs)
        self.total, self.toff, self.ids, self.missing = self.download(self.b, len(docs))
        self.docs = [self.ids[int(self.toff[d]):int(self.toff[d + 1])] for d in range(len(docs))]
        self.spans = {}
        for form, _ in FORMS:
            sp = self.ragged(self.b, *form)
            self.spans[form] = [sp[int(self.toff[d]):int(self.toff[d + 1])] for d in range(len(docs))]
        # the inputs hold what they were built for
        for R, ab in self.lengths.items():
            fa, fb, n = self.groups[("cross", R)]
            assert [(len(self.docs[fa + p]), len(self.docs[fb + p])) for p in range(n)] == ab, "the fixture's documents do not have the id counts it was built for"
        for name in [("cross", 257), "win_big"]:
            fa, fb, n = self.groups[name]
            for d in [d for d in self.docs[fa:fb + n] if len(d) >= 64]:
                assert (d[1:] != d[:-1]).all()                       # ids differ by position: a shifted side shows
                for shift in range(2, min(len(d), 8)):
                    assert (d[shift:] != d[:-shift]).any()
        fa, fb, n = self.groups["mixed"]
        for e0 in self.mixed_empty:
            assert all(len(self.docs[f + e0 + i]) == 0 for f in (fa, fb) for i in range(EMPTY_RUN)) and len(self.docs[fa + e0 - 1]) > 0
        assert self.mixed_empty[1] + EMPTY_RUN == n
        cat = {form: np.concatenate(self.spans[form]) for form, _ in FORMS}
        assert len({cat[f].tobytes() for f in cat}) == 4, "two span forms are the same on this fixture: the normalizer or the units changed nothing"

    def new_batch(self, max_bytes, max_docs):
        b = C.c_void_p()
        N.check(N.lib.tm_batch_create(self.v.handle, max_bytes, max_docs, C.byref(b)))
        return b

    def run_raw(self, b, docs):
        raw, offs = tm.pack_documents(docs)
        N.check(N.lib.tm_batch_upload_raw(b, N.ptr(raw), N.ptr(offs), len(docs)))
        N.check(N.lib.tm_batch_normalize(b, None))
        N.check(N.lib.tm_batch_run(b, None))

    def download(self, b, nd):
        n, m = C.c_uint64(), C.c_uint64()
        N.check(N.lib.tm_batch_totals(b, C.byref(n), C.byref(m)))
        ids = np.zeros(max(n.value, 1), dtype=np.uint32)
        toff = np.zeros(nd + 1, dtype=np.uint64)
        miss = np.zeros(max(nd, 1), dtype=np.uint32)
        N.check(N.lib.tm_batch_download(b, N.ptr(ids), n.value, N.ptr(toff), N.ptr(miss)))
        assert toff[nd] == n.value
        return int(n.value), toff, ids[:n.value], np.append(miss[:nd], m.value)

    def ragged(self, b, text, unit):
        out = Out(2 * self.total, 4)
        N.check(N.lib.tm_batch_spans_in(b, None, text, unit, out.ptr, self.total, None, None))
        self.sync(b)
        assert out.sentinels_intact()
        return out.view(np.uint32).reshape(self.total, 2).astype(np.int64)

    def sync(self, b=None):
        N.check(N.lib.tm_batch_totals(b or self.b, None, None))           # (everything here runs on the NULL stream, which this waits for)

    def how(self, fa, fb, n, L, id_bytes, has_bos, nsep, has_eos, trunc, pad_left, **kw):
        f = dict(first_a=fa, first_b=fb, npairs=n, row_len=L, id_bytes=id_bytes, pad_id=self.pad, bos_id=self.bos if has_bos else NONE,
                 sep_id=self.sep if nsep else NONE, eos_id=self.eos if has_eos else NONE, sep_count=nsep, truncation=trunc, flags=PAD_LEFT if pad_left else 0)
        f.update(kw)
        return Pair(*[f[k] for k, _ in Pair._fields_])

    def pair(self, how, shift=0, outputs=(True, True, True)):
        """-> ids, mask, types, kept as Out (an output left out is passed as NULL)"""
        n, L = how.npairs, how.row_len
        o = [Out(n * L, how.id_bytes, shift), Out(n * L, 1, shift), Out(n * L, 1, shift), Out(2 * n, 4, shift)]
        p = [o[0].ptr] + [x.ptr if use else None for x, use in zip(o[1:], outputs)]
        N.check(N.lib.tm_batch_pair(self.b, C.byref(how), None, *p))
        self.sync()
        return o

    def window_rows(self, how, overlap, max_first, b=None):
        need = C.c_uint64(12345)
        N.check(N.lib.tm_batch_pair_window_rows(b or self.b, C.byref(how), overlap, max_first, C.byref(need)))
        return int(need.value)

    def windows(self, how, overlap, max_first, rows, shift=0, outputs=(True, True, True, True, True)):
        """-> ids, mask, types, kept, row_pair, row_start as Out"""
        L = how.row_len
        o = [Out(rows * L, how.id_bytes, shift), Out(rows * L, 1, shift), Out(rows * L, 1, shift), Out(2 * rows, 4, shift), Out(rows, 4, shift), Out(rows, 4, shift)]
        p = [o[0].ptr] + [x.ptr if use else None for x, use in zip(o[1:], outputs)]
        N.check(N.lib.tm_batch_pair_windows(self.b, C.byref(how), overlap, max_first, None, rows, *p))
        self.sync()
        return o


_env = None
_expected = {}


@pytest.fixture(scope="module")
def env():
    global _env
    if _env is None:
        _env = Env()
    return _env


def sides(env, fa, fb, n, form=None):
    src = env.docs if form is None else env.spans[form]
    return src[fa:fa + n], src[fb:fb + n]


def expected(env, fa, fb, n, L, has_bos, nsep, has_eos, trunc, pad_left, form=None):
    """np_pairs of the pairs, computed once and never changed"""
    key = ("pair", fa, fb, n, L, has_bos, nsep, has_eos, trunc, pad_left, form)
    if key not in _expected:
        A, B = sides(env, fa, fb, n)
        SA, SB = sides(env, fa, fb, n, form) if form is not None else (None, None)
        _expected[key] = np_pairs(A, B, L, env.pad, env.bos if has_bos else None, env.sep, nsep, env.eos if has_eos else None, trunc, pad_left, SA, SB)
    return _expected[key]


def expected_windows(env, fa, fb, n, L, has_bos, nsep, has_eos, overlap, max_first, pad_left, form=None):
    key = ("win", fa, fb, n, L, has_bos, nsep, has_eos, overlap, max_first, pad_left, form)
    if key not in _expected:
        A, B = sides(env, fa, fb, n)
        SA, SB = sides(env, fa, fb, n, form) if form is not None else (None, None)
        _expected[key] = np_pair_windows(A, B, L, env.pad, env.bos if has_bos else None, env.sep, nsep, env.eos if has_eos else None, overlap, max_first, pad_left, SA, SB)
    return _expected[key]


def check_rows(o, e, id_bytes, what, outputs=None):
    """ids and every optional output against the Rows e (outputs: which of the optional ones were passed)"""
    rows, L = e.ids.shape
    want = [e.mask.reshape(-1), e.types.reshape(-1), e.kept.reshape(-1)] + ([e.row_pair, e.row_start] if len(o) == 6 else [])
    outputs = outputs or (True,) * len(want)
    assert (o[0].view(DT[id_bytes]).reshape(rows, L) == e.ids).all() and o[0].sentinels_intact(), what
    for x, exp, use, dt in zip(o[1:], want, outputs, (np.uint8, np.uint8, np.uint32, np.uint32, np.uint32)):
        if use:
            assert (x.view(dt) == exp).all() and x.sentinels_intact(), what
        else:
            assert x.untouched(), what


# ---- ids, mask, types and kept counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ROW_LENS)
def test_pairs_every_shape(env, L):
    """every combination of bos, 0 / 1 / 2 separators and eos that leaves R >= 0 (R == 0: a row of specials only), the three truncations, ids of
    2, 4 and 8 bytes, right and left padding, outputs on a 16-byte boundary and off it; side lengths 0, 1, h - 1, h, h + 1, R - h, R - 1, R,
    R + 1 and 2R + 1 crossed for A and B"""
    k = 0
    seen = set()
    for has_bos, nsep, has_eos, R in specials(L):
        fa, fb, n = env.groups[("cross", R)]
        for trunc in TRUNCS:
            for id_bytes in ((2, 4, 8) if L <= 7 else ((2, 4, 8)[k % 3],)):
                pad_left, shift = bool(k & 1), (k >> 1) & 1
                k += 1
                e = expected(env, fa, fb, n, L, has_bos, nsep, has_eos, trunc, pad_left)
                how = env.how(fa, fb, n, L, id_bytes, has_bos, nsep, has_eos, trunc, pad_left)
                what = (L, has_bos, nsep, has_eos, trunc, id_bytes, pad_left, shift)
                check_rows(env.pair(how, shift), e, id_bytes, what)
                seen.add((id_bytes, pad_left, shift))
                # the kept counts fill the row whenever something was cut, and the row's entries are the specials and the kept ids
                cut = np.array([a + b > R for a, b in env.lengths[R]])
                assert (e.kept.sum(axis=1)[cut] == R).all() and (e.mask.sum(axis=1) == e.kept.sum(axis=1) + (L - R)).all(), what
        if R >= 3:
            # the three truncations differ on this fixture
            assert len({expected(env, fa, fb, n, L, has_bos, nsep, has_eos, t, False).kept.tobytes() for t in TRUNCS}) == 3
    assert {i for i, _, _ in seen} == {2, 4, 8} and {(p, s) for _, p, s in seen} == {(p, s) for p in (False, True) for s in (0, 1)}


def test_ranges_disjoint_overlapping_identical_and_each_output_null_in_turn(env):
    fa, fb, n = env.groups["mixed"]
    e0, e1 = env.mixed_empty
    for (a0, b0, cnt), (L, id_bytes, has_bos, nsep, has_eos, trunc, pad_left, shift) in zip(
            ((fa, fb, n), (fa, fa + 3, n), (fa + 5, fa + 5, n - 5), (fb, fa, n)),
            ((9, 2, True, 1, True, LONGEST, False, 1), (7, 8, True, 2, False, ONLY_FIRST, True, 1), (65, 4, False, 1, True, LONGEST, False, 0), (1, 2, False, 0, False, ONLY_SECOND, True, 0))):
        e = expected(env, a0, b0, cnt, L, has_bos, nsep, has_eos, trunc, pad_left)
        how = env.how(a0, b0, cnt, L, id_bytes, has_bos, nsep, has_eos, trunc, pad_left)
        for outputs in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            check_rows(env.pair(how, shift, outputs), e, id_bytes, (a0, b0, L, id_bytes, outputs), outputs)
        if a0 == b0:
            assert (e.kept[:, 0] <= e.kept[:, 1]).all() and (e.kept[:, 0] < e.kept[:, 1]).any()      # the same document twice: A gives way on a tie
    # the runs of pairs of empty documents: rows of specials only between rows that hold ids, and at the end
    e = expected(env, fa, fb, n, 9, True, 1, True, LONGEST, False)
    for s in (e0, e1):
        assert not e.kept[s:s + EMPTY_RUN].any() and e.kept[s - 1].any() and (e.mask[s:s + EMPTY_RUN].sum(axis=1) == 3).all()
    # no pairs: nothing written
    how = env.how(fa, fb, 0, 7, 4, True, 1, True, LONGEST, False)
    o = Out(64, 4)
    N.check(N.lib.tm_batch_pair(env.b, C.byref(how), None, o.ptr, o.ptr, o.ptr, o.ptr))
    N.check(N.lib.tm_batch_pair_spans_in(env.b, C.byref(how), None, 0, 0, o.ptr, 4))
    env.sync()
    assert o.untouched()


# ---- spans -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SPAN_LENS)
def test_pair_spans(env, L):
    """the pairs of tm_batch_spans_in in the columns of their ids, each side counting from its own document's start, (0, 0) on specials and
    padding; elements of 4 and 8 bytes; normalized bytes, raw bytes, raw code points and normalized UTF-16 units"""
    fa, fb, n = env.groups["mixed"]
    k = 0
    seen = set()
    for j, (has_bos, nsep, has_eos, R) in enumerate(specials(L)):
        for form, span_bytes in (FORMS if L == 1 else [FORMS[j % 4]]):
            pad_left, shift, trunc = bool(k & 1), (k >> 1) % 3, TRUNCS[k % 3]
            a0, b0, cnt = ((fa, fb, n), (fa + 2, fa + 9, n), (fb, fb, n))[k % 3]
            k += 1
            e = expected(env, a0, b0, cnt, L, has_bos, nsep, has_eos, trunc, pad_left, form)
            how = env.how(a0, b0, cnt, L, 4, has_bos, nsep, has_eos, trunc, pad_left)
            out = Out(cnt * L * 2, span_bytes, shift)
            N.check(N.lib.tm_batch_pair_spans_in(env.b, C.byref(how), None, form[0], form[1], out.ptr, span_bytes))
            env.sync()
            what = (L, has_bos, nsep, has_eos, form, span_bytes, trunc, pad_left, shift, a0, b0)
            got = out.view(np.uint32 if span_bytes == 4 else np.uint64).reshape(cnt, L, 2)
            assert out.sentinels_intact() and (got == e.spans).all(), what
            assert not got[~e.content].any() and (R == 0 or got[e.content][:, 1].any()), what
            seen.add((form, span_bytes))
    assert seen == set(FORMS)


# ---- pair windows ----------------------------------------------------------------------------------------------------------------------------
def window_shapes(L):
    """-> list of (has_bos, nsep, has_eos, R, overlap, max_first): overlap 0, 1 and room_min - 1, max_first 0, 1 and R - overlap - 1"""
    out = []
    for has_bos, nsep, has_eos, R in specials(L):
        if L >= 64 and (has_bos, nsep, has_eos) not in ((1, 1, 1), (0, 0, 0), (1, 2, 1)):
            continue
        combos = set()
        for o in (0, 1):
            for mf in (0, 1, R - o - 1):
                if 0 <= mf <= R and R - mf > o:
                    combos.add((o, mf))
        for mf in (0, 1):
            if R - mf >= 1:
                combos.add((R - mf - 1, mf))              # overlap = room_min - 1: a step of one id
        out += [(has_bos, nsep, has_eos, R, o, mf) for o, mf in sorted(combos)]
    return out


@pytest.mark.parametrize("L", WINDOW_LENS)
def test_pair_windows(env, L):
    """A of 0, 1, 2 ids and one that max_first cuts, against B of every length around room_p and room_p + step_p: the number of rows, the
    pair and the start of every row, the kept counts, ids, mask and types"""
    fa, fb, n = env.groups["win_small" if L < 64 else "win_big"]
    k = 0
    seen = set()
    shapes = window_shapes(L)
    assert {o for *_, o, _ in shapes} >= {0, 1} and {mf for *_, mf in shapes} >= {0, 1}
    for has_bos, nsep, has_eos, R, overlap, max_first in shapes:
        id_bytes, pad_left, shift = (2, 4, 8)[k % 3], bool((k // 3) & 1), (k >> 1) & 1
        k += 1
        if L >= 64 and R - max_first - overlap == 1 and k % 4:          # (a step of one id makes a hundred rows a pair: a quarter of those shapes)
            continue
        e = expected_windows(env, fa, fb, n, L, has_bos, nsep, has_eos, overlap, max_first, pad_left)
        rows = e.ids.shape[0]
        how = env.how(fa, fb, n, L, id_bytes, has_bos, nsep, has_eos, ONLY_SECOND, pad_left)
        what = (L, has_bos, nsep, has_eos, overlap, max_first, id_bytes, pad_left, shift)
        assert env.window_rows(how, overlap, max_first) == rows, what
        check_rows(env.windows(how, overlap, max_first, rows, shift), e, id_bytes, what)
        seen.add((id_bytes, pad_left))
        # every pair has a row, a short A leaves more room than a cut one, and some pair takes several rows
        assert set(e.row_pair.tolist()) == set(range(n)) and rows > n, what
        if max_first >= 2:
            assert len(set(e.kept[:, 0].tolist())) >= 3, what
    assert seen == {(i, p) for i in (2, 4, 8) for p in (False, True)}


def test_pair_windows_part_of_the_run_null_outputs_and_rows_cap(env):
    fa, fb, n = env.groups["win_small"]
    L, overlap, max_first = 9, 1, 3
    for a0, b0, cnt, id_bytes, shift in ((fa + 3, fb + 3, n - 7, 2, 1), (fb, fb, n, 8, 0)):
        e = expected_windows(env, a0, b0, cnt, L, True, 1, True, overlap, max_first, False)
        rows = e.ids.shape[0]
        how = env.how(a0, b0, cnt, L, id_bytes, True, 1, True, ONLY_SECOND, False)
        assert env.window_rows(how, overlap, max_first) == rows
        for outputs in ((True,) * 5, (False, True, True, True, True), (True, False, True, True, True), (True, True, False, True, True), (True, True, True, False, True),
                        (True, True, True, True, False), (False,) * 5):
            check_rows(env.windows(how, overlap, max_first, rows, shift, outputs), e, id_bytes, (a0, id_bytes, outputs), outputs)
        # more room than needed: the rows behind the last stay as they were
        o = Out((rows + 3) * L, id_bytes, shift)
        N.check(N.lib.tm_batch_pair_windows(env.b, C.byref(how), overlap, max_first, None, rows + 3, o.ptr, None, None, None, None, None))
        env.sync()
        assert (o.view(DT[id_bytes])[:rows * L].reshape(rows, L) == e.ids).all() and (o.buf.array[o.off + rows * L * id_bytes:] == FILL).all()
        # rows_cap one too small: nothing written, the number is in the message
        o = [Out(rows * L, id_bytes), Out(rows * L, 1), Out(rows * L, 1), Out(2 * rows, 4), Out(rows, 4), Out(rows, 4)]
        so = Out(rows * L * 2, 8)
        assert N.lib.tm_batch_pair_windows(env.b, C.byref(how), overlap, max_first, None, rows - 1, *[x.ptr for x in o]) == N.TM_E_NOSPACE
        assert str(rows).encode() in N.lib.tm_last_error()
        assert N.lib.tm_batch_pair_windows_spans_in(env.b, C.byref(how), overlap, max_first, None, rows - 1, 0, 0, so.ptr, 8) == N.TM_E_NOSPACE
        assert str(rows).encode() in N.lib.tm_last_error()
        env.sync()
        assert all(x.untouched() for x in o + [so])
    # no pairs: no rows, nothing written
    how = env.how(fa, fb, 0, L, 4, True, 1, True, ONLY_SECOND, False)
    assert env.window_rows(how, overlap, max_first) == 0
    o = Out(64, 4)
    N.check(N.lib.tm_batch_pair_windows(env.b, C.byref(how), overlap, max_first, None, 8, o.ptr, o.ptr, o.ptr, o.ptr, o.ptr, o.ptr))
    env.sync()
    assert o.untouched()


@pytest.mark.parametrize("L", [4, 9, 65])
def test_pair_window_spans(env, L):
    """B's offsets count from B's document start in every row, A's from A's"""
    fa, fb, n = env.groups["mixed"]
    k = 0
    seen = set()
    for has_bos, nsep, has_eos, R, overlap, max_first in window_shapes(L)[::3]:          # (every third shape: test_pair_windows has them all)
        form, span_bytes = FORMS[k % 4]
        pad_left, shift = bool((k >> 2) & 1), k % 3
        a0, b0, cnt = ((fa, fb, n), (fa + 2, fa + 9, n - 3))[k & 1]
        k += 1
        e = expected_windows(env, a0, b0, cnt, L, has_bos, nsep, has_eos, overlap, max_first, pad_left, form)
        rows = e.ids.shape[0]
        how = env.how(a0, b0, cnt, L, 4, has_bos, nsep, has_eos, ONLY_SECOND, pad_left)
        out = Out(rows * L * 2, span_bytes, shift)
        N.check(N.lib.tm_batch_pair_windows_spans_in(env.b, C.byref(how), overlap, max_first, None, rows, form[0], form[1], out.ptr, span_bytes))
        env.sync()
        what = (L, has_bos, nsep, has_eos, overlap, max_first, form, span_bytes, pad_left, shift, a0)
        got = out.view(np.uint32 if span_bytes == 4 else np.uint64).reshape(rows, L, 2)
        assert out.sentinels_intact() and (got == e.spans).all(), what
        assert not got[~e.content].any() and got[e.content][:, 1].any(), what
        seen.add((form, span_bytes))
    assert seen == set(FORMS)


# ---- the new layout against the old ones -----------------------------------------------------------------------------------------------------
def same(x, y):
    """two outputs hold the same bytes, and nothing was written around either"""
    return x.sentinels_intact() and y.sentinels_intact() and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_an_empty_second_side_is_collate(env):
    """B empty for every pair, no separator, eos behind: byte for byte the ids, mask and spans of tm_batch_collate / tm_batch_collate_spans_in"""
    fa, fb, n = env.groups["mixed"]
    empty = fb + env.mixed_empty[1]                       # sixteen empty documents
    for first, cnt, L, id_bytes, has_bos, has_eos, trunc, pad_left, shift in ((fa, EMPTY_RUN, 9, 2, True, True, LONGEST, False, 1), (fa + 3, EMPTY_RUN, 4, 8, False, True, ONLY_SECOND, True, 0),
                                                                              (fa + 7, EMPTY_RUN, 65, 4, True, False, ONLY_FIRST, False, 1)):
        how = env.how(first, empty, cnt, L, id_bytes, has_bos, 0, has_eos, trunc, pad_left)
        old = Collate(first, cnt, L, id_bytes, env.pad, env.bos if has_bos else NONE, env.eos if has_eos else NONE, PAD_LEFT if pad_left else 0)
        o = env.pair(how, shift)
        c = [Out(cnt * L, id_bytes, shift), Out(cnt * L, 1, shift), Out(cnt, 4, shift)]
        N.check(N.lib.tm_batch_collate(env.b, C.byref(old), None, *[x.ptr for x in c]))
        env.sync()
        assert same(o[0], c[0]) and same(o[1], c[1])
        kept = o[3].view(np.uint32).reshape(cnt, 2)
        assert not o[2].view(np.uint8)[o[0].view(DT[id_bytes]) != env.eos].any() and not kept[:, 1].any()
        assert (kept[:, 0] + has_bos + has_eos == c[2].view(np.uint32)).all() and kept[:, 0].any()
        for form, span_bytes in FORMS:
            s, t = Out(cnt * L * 2, span_bytes, shift), Out(cnt * L * 2, span_bytes, shift)
            N.check(N.lib.tm_batch_pair_spans_in(env.b, C.byref(how), None, form[0], form[1], s.ptr, span_bytes))
            N.check(N.lib.tm_batch_collate_spans_in(env.b, C.byref(old), None, form[0], form[1], t.ptr, span_bytes))
            env.sync()
            assert same(s, t) and s.view(np.uint32).any()


def test_an_empty_first_side_is_windows(env):
    """A empty and max_first 0: tm_batch_pair_windows is tm_batch_windows on the B range"""
    fa, fb, n = env.groups["mixed"]
    empty = fa + env.mixed_empty[0]
    first = fb + env.mixed_empty[0] - 6                   # six documents with ids, ten empty ones
    for L, id_bytes, has_bos, has_eos, overlap, pad_left, shift in ((5, 2, True, True, 1, False, 1), (8, 8, False, False, 0, True, 0), (3, 4, True, False, 1, False, 1)):
        cnt = EMPTY_RUN
        how = env.how(empty, first, cnt, L, id_bytes, has_bos, 0, has_eos, ONLY_SECOND, pad_left)
        old = Collate(first, cnt, L, id_bytes, env.pad, env.bos if has_bos else NONE, env.eos if has_eos else NONE, PAD_LEFT if pad_left else 0)
        rows = env.window_rows(how, overlap, 0)
        need = C.c_uint64()
        N.check(N.lib.tm_batch_window_rows(env.b, C.byref(old), overlap, C.byref(need)))
        assert rows == need.value > cnt
        o = env.windows(how, overlap, 0, rows, shift)
        w = [Out(rows * L, id_bytes, shift), Out(rows * L, 1, shift), Out(rows, 4, shift), Out(rows, 4, shift), Out(rows, 4, shift)]
        N.check(N.lib.tm_batch_windows(env.b, C.byref(old), overlap, None, rows, *[x.ptr for x in w]))
        env.sync()
        for x, y in ((o[0], w[0]), (o[1], w[1]), (o[4], w[3]), (o[5], w[4])):
            assert same(x, y)
        kept = o[3].view(np.uint32).reshape(rows, 2)
        assert not kept[:, 0].any() and (kept[:, 1] + has_bos + has_eos == w[2].view(np.uint32)).all()
        for form, span_bytes in FORMS[:2]:
            s, t = Out(rows * L * 2, span_bytes, shift), Out(rows * L * 2, span_bytes, shift)
            N.check(N.lib.tm_batch_pair_windows_spans_in(env.b, C.byref(how), overlap, 0, None, rows, form[0], form[1], s.ptr, span_bytes))
            N.check(N.lib.tm_batch_windows_spans_in(env.b, C.byref(old), overlap, None, rows, form[0], form[1], t.ptr, span_bytes))
            env.sync()
            assert same(s, t) and s.view(np.uint32).any()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(env):
    fa, fb, n = env.groups["mixed"]
    nd = len(env.docs)
    L = 8
    o = [Out(n * L, 8), Out(n * L, 1), Out(n * L, 1), Out(2 * n, 4), Out(n, 4), Out(n, 4)]
    so = Out(n * L * 2, 8)
    need = C.c_uint64()
    INV = N.TM_E_INVALID

    def every_call(how, overlap=1, max_first=2, rows_cap=1 << 20, b=None, text=0, unit=0, span_bytes=8, calls=(0, 1, 2, 3, 4)):
        """the return codes of the five calls (calls: which of them to make - 0, 1 the pair forms, 2, 3, 4 the window forms; 1 and 4 the span forms)"""
        b = b or env.b
        fns = [lambda: N.lib.tm_batch_pair(b, C.byref(how), None, *[x.ptr for x in o[:4]]),
               lambda: N.lib.tm_batch_pair_spans_in(b, C.byref(how), None, text, unit, so.ptr, span_bytes),
               lambda: N.lib.tm_batch_pair_window_rows(b, C.byref(how), overlap, max_first, C.byref(need)),
               lambda: N.lib.tm_batch_pair_windows(b, C.byref(how), overlap, max_first, None, rows_cap, *[x.ptr for x in o]),
               lambda: N.lib.tm_batch_pair_windows_spans_in(b, C.byref(how), overlap, max_first, None, rows_cap, text, unit, so.ptr, span_bytes)]
        rc = [fns[i]() for i in calls]
        env.sync(b)
        assert all(x.untouched() for x in o + [so])
        return rc

    def how(**kw):
        f = dict(fa=fa, fb=fb, n=n, L=L, id_bytes=4, has_bos=True, nsep=1, has_eos=True, trunc=ONLY_SECOND, pad_left=False)
        f.update({k: kw.pop(k) for k in list(kw) if k in f})
        return env.how(*[f[k] for k in ("fa", "fb", "n", "L", "id_bytes", "has_bos", "nsep", "has_eos", "trunc", "pad_left")], **kw)

    assert every_call(how(fa=nd - n + 1)) == [INV] * 5 and b"of a run of" in N.lib.tm_last_error()           # A's range beyond the run
    assert every_call(how(fb=nd - n + 1)) == [INV] * 5                                                        # B's
    assert every_call(how(fa=0xFFFFFFF0)) == [INV] * 5
    assert every_call(how(L=2)) == [INV] * 5 and b"row_len" in N.lib.tm_last_error()                          # row_len < ns
    assert every_call(how(L=0)) == [INV] * 5
    assert every_call(how(flags=KEEP_TAIL)) == [INV] * 5 and b"KEEP_TAIL" in N.lib.tm_last_error()
    assert every_call(how(flags=PAD_LEFT | KEEP_TAIL)) == [INV] * 5
    assert every_call(how(flags=4)) == [INV] * 5                                                              # unknown flag
    assert every_call(how(truncation=3)) == [INV] * 5 and b"truncation" in N.lib.tm_last_error()
    assert every_call(how(sep_count=0)) == [INV] * 5 and b"sep_count" in N.lib.tm_last_error()                # a sep_id wants 1 or 2
    assert every_call(how(sep_count=3)) == [INV] * 5
    assert every_call(how(sep_id=NONE)) == [INV] * 5                                                          # no sep_id wants 0
    assert every_call(how(id_bytes=3)) == [INV] * 5
    assert every_call(how(id_bytes=2, sep_id=65536)) == [INV] * 5 and b"two bytes" in N.lib.tm_last_error()   # sep_id counts among the specials
    assert every_call(how(id_bytes=2, pad_id=70000)) == [INV] * 5
    assert every_call(how(pad_id=NONE)) == [INV] * 5
    # the truncations the window form does not take
    for t in (LONGEST, ONLY_FIRST):
        assert every_call(how(trunc=t), calls=(2, 3, 4)) == [INV] * 3 and b"ONLY_SECOND" in N.lib.tm_last_error()
    # R = 5: max_first > R, and R - max_first <= overlap
    assert every_call(how(), 0, 6, calls=(2, 3, 4)) == [INV] * 3 and b"max_first" in N.lib.tm_last_error()
    assert every_call(how(), 3, 2, calls=(2, 3, 4)) == [INV] * 3
    assert every_call(how(), 5, 0, calls=(2, 3, 4)) == [INV] * 3
    assert every_call(how(), 0xFFFFFFFF, 0xFFFFFFFF, calls=(2, 3, 4)) == [INV] * 3
    assert every_call(how(L=3), 0, 0, calls=(2, 3, 4)) == [INV] * 3                                                        # R == 0 holds no window
    # the span arguments
    assert every_call(how(), span_bytes=2, calls=(1, 4)) == [INV] * 2 and b"span_bytes" in N.lib.tm_last_error()
    assert every_call(how(), text=2, calls=(1, 4)) == [INV] * 2
    assert every_call(how(), unit=3, calls=(1, 4)) == [INV] * 2
    # more than 2^36 elements in one output
    LIM = N.TM_E_LIMIT
    assert every_call(how(L=1 << 30), calls=(0, 1)) == [LIM] * 2
    assert every_call(how(L=1 << 31, has_bos=False, nsep=0, has_eos=False), 0, 0, calls=(2, 3, 4)) == [LIM] * 3 and need.value >= n
    # null arguments
    h = how()
    assert N.lib.tm_batch_pair(env.b, C.byref(h), None, None, None, None, None) == INV
    assert N.lib.tm_batch_pair(env.b, None, None, o[0].ptr, None, None, None) == INV
    assert N.lib.tm_batch_pair(None, C.byref(h), None, o[0].ptr, None, None, None) == INV
    assert N.lib.tm_batch_pair_spans_in(env.b, C.byref(h), None, 0, 0, None, 8) == INV
    assert N.lib.tm_batch_pair_window_rows(env.b, C.byref(h), 1, 2, None) == INV
    assert N.lib.tm_batch_pair_windows(env.b, C.byref(h), 1, 2, None, 1 << 20, None, None, None, None, None, None) == INV
    assert N.lib.tm_batch_pair_windows_spans_in(env.b, C.byref(h), 1, 2, None, 1 << 20, 0, 0, None, 8) == INV
    env.sync()
    assert all(x.untouched() for x in o + [so])
    b = env.new_batch(1 << 16, 64)
    try:
        docs = [env.raw[fa], b"", b"abc" * 30, b"cab" * 7]
        h4 = env.how(0, 2, 2, L, 8, True, 1, True, ONLY_SECOND, False)
        assert every_call(h4, b=b) == [INV] * 5 and b"no ids" in N.lib.tm_last_error()                        # no run yet
        # a batch uploaded NORMALIZED has no raw text to point into: TM_TEXT_RAW is refused, the rest works
        text, offs = tm.pack_documents([env.v.normalize(d) for d in docs])
        N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(offs), 4))
        N.check(N.lib.tm_batch_run(b, None))
        assert every_call(h4, b=b, text=1, calls=(1, 4)) == [INV] * 2
        rows = env.window_rows(h4, 1, 2, b)
        assert rows > 2
        ok = Out(rows * L * 2, 8)
        N.check(N.lib.tm_batch_pair_windows_spans_in(b, C.byref(h4), 1, 2, None, rows, 0, 1, ok.ptr, 8))
        env.sync(b)
        assert ok.sentinels_intact() and ok.view(np.uint64).any()
        # ids that came from no walk have no spans: tm_batch_load_ids behind a raw run
        env.run_raw(b, docs)
        src = Out(4 * 8, 4)
        src.view(np.uint32)[:] = np.arange(32) % 5
        N.check(N.lib.tm_batch_load_ids(b, src.ptr, 4, 8, 4, None, NONE, NONE, NONE, None))
        assert N.lib.tm_batch_pair_spans_in(b, C.byref(h4), None, 0, 0, so.ptr, 8) == INV
        assert N.lib.tm_batch_pair_windows_spans_in(b, C.byref(h4), 1, 2, None, 1 << 20, 0, 0, so.ptr, 8) == INV
        env.sync(b)
        assert so.untouched()
        # ... but they pair: rows 0, 1 against rows 2, 3, eight ids each, R = 5
        ids4 = [np.arange(8 * r, 8 * r + 8) % 5 for r in range(4)]
        e = np_pairs(ids4[:2], ids4[2:], L, env.pad, env.bos, env.sep, 1, env.eos, LONGEST, False)
        got = Out(2 * L, 8)
        h4.truncation = LONGEST
        N.check(N.lib.tm_batch_pair(b, C.byref(h4), None, got.ptr, None, None, None))
        env.sync(b)
        assert (got.view(np.uint64).reshape(2, L) == e.ids).all() and (e.kept == (2, 3)).all()
    finally:
        N.lib.tm_batch_free(b)
    # the batch of the fixture is as good as before
    e = expected(env, fa, fb, n, L, True, 1, True, LONGEST, False)
    check_rows(env.pair(how(trunc=LONGEST, id_bytes=8)), e, 8, "after the errors")

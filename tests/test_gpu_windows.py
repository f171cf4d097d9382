"""-m gpu: sliding windows - tm_batch_window_rows / tm_batch_windows / tm_batch_windows_spans / tm_batch_windows_raw_spans
(tokenmonster_amd/csrc/tm_windows.hip) at the C ABI, outputs in tm_host_alloc memory behind sentinels, against a numpy statement of the rule of
include/tokenmonster_hip.h.  The ids and the pairs come from tm_batch_download, tm_batch_spans and tm_batch_raw_spans of the same run: this
file tests layout, not tokenization.  tests/test_windows_emulated.py runs this file on the emulated device (tools/emu), without a GPU."""
import ctypes as C

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth
from fixed_shape import Collate, Out, spec, DT, FILL, KEEP_TAIL, NONE, PAD_LEFT

ROW_LENS = [1, 2, 3, 7, 64, 65, 257]
SPAN_LENS = [1, 3, 7, 65]
FORMS = [("norm", 4), ("raw", 8), ("norm", 8), ("raw", 4)]
SPECIALS = [(False, False), (True, False), (False, True), (True, True)]
EMPTY_RUN = 16          # (sixteen rows in a row hold a whole 16-byte vector of two-byte ids wherever the run begins)
pytestmark = pytest.mark.gpu


def shapes(L):
    """every (bos?, eos?, overlap) to test at row length L -> list of (has_bos, has_eos, room, overlap)"""
    out = []
    for has_bos, has_eos in SPECIALS:
        room = L - has_bos - has_eos
        if room < 1:
            continue
        for overlap in sorted({o for o in (0, 1, room - 1) if 0 <= o < room}):
            out.append((has_bos, has_eos, room, overlap))
    return out


def counts_of(room, step):
    return {0, 1, room - 1, room, room + 1, room + step, room + step + 1, 3 * room + 1}


# ---- the rule, in numpy --------------------------------------------------------------------------------------------------------------------
def n_windows(n, room, step):
    return 1 if n <= room else 1 + -(-(n - room) // step)


def np_windows(docs, L, pad, bos, eos, overlap, pad_left, spans=None):
    """docs: list of id arrays (spans: list of [n, 2] arrays beside them) -> ids u64 [rows, L], mask, lengths, row_doc, row_start
    (and the pairs i64 [rows, L, 2]): window k of a document is [bos] ids[k * step : min(k * step + room, n)] [eos], then padding"""
    room = L - (bos is not None) - (eos is not None)
    step = room - overlap
    assert room >= 1 and step >= 1
    plan = [(d, k * step) for d, doc in enumerate(docs) for k in range(n_windows(len(doc), room, step))]
    rows = len(plan)
    ids = np.full((rows, L), pad, dtype=np.uint64)
    mask = np.zeros((rows, L), dtype=np.uint8)
    lens = np.zeros(rows, dtype=np.uint32)
    sp = np.zeros((rows, L, 2), dtype=np.int64) if spans is not None else None
    head = [bos] if bos is not None else []
    tail = [eos] if eos is not None else []
    for r, (d, s) in enumerate(plan):
        body = docs[d][s:s + room]
        row = head + list(body) + tail
        lo = L - len(row) if pad_left else 0
        ids[r, lo:lo + len(row)] = row
        mask[r, lo:lo + len(row)] = 1
        lens[r] = len(row)
        if sp is not None:
            sp[r, lo + len(head):lo + len(head) + len(body)] = spans[d][s:s + room]
    row_doc = np.array([d for d, _ in plan], dtype=np.uint32)
    row_start = np.array([s for _, s in plan], dtype=np.uint32)
    return ids, mask, lens, row_doc, row_start, sp


# ---- one vocabulary, one run for the whole file -----------------------------------------------------------------------------------------
LETTERS = b"abcdefghijklmnopqrst"


def vocab_tokens():
    """every letter a..t, the capcode markers and some punctuation are tokens of one byte, and no longer token is made of those letters alone: a
    document of n of those letters is n ids, each the id of its letter.  'x' and 'y' have no token (one unk id each); the longer tokens
    are for the raw documents"""
    toks = {bytes([c]) for c in LETTERS + b" .,'\nDCW"}
    toks |= {" zz".encode(), b"zzu", b"uz", b" zu", b"D zz", b"zu z", "é".encode(), "́".encode(), "ź".encode()}
    return sorted(toks)


class Env:
    def __init__(self):
        rng = np.random.default_rng(88001)
        self.v = tm.Vocab(synth.build_vocab(vocab_tokens(), capcode=2, charset=1, norm_flag=1, with_unk=True))
        n_ids = self.v.n_ids()
        self.pad, self.bos, self.eos = n_ids + 5, n_ids + 6, n_ids + 7          # (no document holds them)
        assert self.eos < 65536

        def letters(n):
            """n letters, no two neighbours alike and no period a window step could hide behind"""
            a = rng.integers(0, len(LETTERS), size=n)
            for i in range(1, n):
                if a[i] == a[i - 1]:
                    a[i] = (a[i] + 1 + i % 7) % len(LETTERS)
            return bytes(LETTERS[int(x)] for x in a)

        want = set()
        for L in ROW_LENS:
            for _, _, room, overlap in shapes(L):
                want |= counts_of(room, room - overlap)
        self.exact = sorted(want)
        docs = [letters(n) for n in self.exact]
        self.groups = {"exact": (0, len(docs))}
        # two long documents with a run of empty ones between them, what the normalizer changes, short random documents, and a run of empty
        # documents at the end
        first = len(docs)
        docs += [letters(1500)] + [b""] * EMPTY_RUN + [letters(1203)]
        docs += ["Hello WORLD zzé Éa zu zzu".encode(), "aBé cD".encode() * 40, b"x", b"xay" * 5, "É".encode() + letters(300) + b" ZZU"]
        docs += [letters(int(n)) for n in rng.integers(0, 40, size=150)]
        docs += [b""] * EMPTY_RUN
        self.groups["mixed"] = (first, len(docs) - first)
        self.raw = docs
        assert sum(len(d) for d in docs) < (1 << 20)
        self.b = self.new_batch(1 << 19, len(docs) + 8)
        self.run_raw(self.b, docs)
        self.total, self.toff, self.ids, self.missing = self.download(self.b, len(docs))
        self.docs = [self.ids[int(self.toff[d]):int(self.toff[d + 1])] for d in range(len(docs))]
        sp = self.ragged(self.b, raw=False)
        rsp = self.ragged(self.b, raw=True)
        self.spans = [sp[int(self.toff[d]):int(self.toff[d + 1])] for d in range(len(docs))]
        self.raw_spans = [rsp[int(self.toff[d]):int(self.toff[d + 1])] for d in range(len(docs))]
        # the inputs hold what they were built for
        assert [len(d) for d in self.docs[:len(self.exact)]] == self.exact, "the fixture's documents do not have the id counts it was built for"
        for d in self.docs[:len(self.exact)] + [self.docs[first], self.docs[first + EMPTY_RUN + 1]]:
            assert (d[1:] != d[:-1]).all()                       # ids differ by position: a shifted window shows
            for shift in range(2, min(len(d), 8)):
                assert (d[shift:] != d[:-shift]).any()
        assert all(len(d) == 0 for d in self.docs[first + 1:first + 1 + EMPTY_RUN]) and len(self.docs[first]) == 1500 and len(self.docs[first + EMPTY_RUN + 1]) == 1203
        assert all(len(d) == 0 for d in self.docs[-EMPTY_RUN:])
        assert not np.array_equal(sp, rsp), "the normalizer changed nothing: raw and normalized spans are the same"
        k = first + EMPTY_RUN + 2                                # "Hello WORLD ...": capitals and a two-byte letter
        assert int(self.raw_spans[k][-1, 1]) == len(docs[k]) != int(self.spans[k][-1, 1])

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

    def ragged(self, b, raw):
        out = Out(2 * self.total, 4)
        if raw:
            hd = C.c_uint32(77)
            N.check(N.lib.tm_batch_raw_spans(b, None, out.ptr, self.total, C.byref(hd)))
            assert hd.value == 0
        else:
            N.check(N.lib.tm_batch_spans(b, None, out.ptr, self.total))
        self.sync(b)
        assert out.sentinels_intact()
        return out.view(np.uint32).reshape(self.total, 2).astype(np.int64)

    def sync(self, b=None):
        N.check(N.lib.tm_batch_totals(b or self.b, None, None))           # (everything here runs on the NULL stream, which this waits for)

    def how(self, first, nd, L, id_bytes, bos, eos, pad_left, **kw):
        f = dict(first_doc=first, ndocs=nd, row_len=L, id_bytes=id_bytes, pad_id=self.pad, bos_id=spec(bos), eos_id=spec(eos), flags=PAD_LEFT if pad_left else 0)
        f.update(kw)
        return Collate(*[f[n] for n, _ in Collate._fields_])

    def rows(self, how, overlap, b=None):
        need = C.c_uint64(12345)
        N.check(N.lib.tm_batch_window_rows(b or self.b, C.byref(how), overlap, C.byref(need)))
        return int(need.value)

    def windows(self, how, overlap, rows, shift=0, outputs=(True, True, True, True)):
        """-> ids, mask, lengths, row_doc, row_start as Out (an output left out is passed as NULL)"""
        L = how.row_len
        o = [Out(rows * L, how.id_bytes, shift), Out(rows * L, 1, shift), Out(rows, 4, shift), Out(rows, 4, shift), Out(rows, 4, shift)]
        p = [o[0].ptr] + [x.ptr if use else None for x, use in zip(o[1:], outputs)]
        N.check(N.lib.tm_batch_windows(self.b, C.byref(how), overlap, None, rows, *p))
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


def expected(env, first, nd, L, has_bos, has_eos, overlap, pad_left, spans=None):
    """np_windows of the documents first .. first + nd, computed once and never changed"""
    key = (first, nd, L, has_bos, has_eos, overlap, pad_left, spans)
    if key not in _expected:
        sp = {None: None, "norm": env.spans, "raw": env.raw_spans}[spans]
        _expected[key] = np_windows(env.docs[first:first + nd], L, env.pad, env.bos if has_bos else None, env.eos if has_eos else None, overlap, pad_left,
                                    sp[first:first + nd] if sp is not None else None)
        for a in _expected[key]:
            if a is not None:
                a.setflags(write=False)
    return _expected[key]


def check_rows(env, o, e, id_bytes, what, outputs=(True, True, True, True)):
    rows, L = e[0].shape
    assert (o[0].view(DT[id_bytes]).reshape(rows, L) == e[0]).all() and o[0].sentinels_intact(), what
    for x, exp, use, dt in zip(o[1:], (e[1].reshape(-1), e[2], e[3], e[4]), outputs, (np.uint8, np.uint32, np.uint32, np.uint32)):
        if use:
            assert (x.view(dt) == exp).all() and x.sentinels_intact(), what
        else:
            assert x.untouched(), what


# ---- ids, mask and the per-row outputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ROW_LENS)
def test_windows_every_shape(env, L):
    """every specials combination, overlap 0, 1 and room - 1, ids of 2, 4 and 8 bytes, right and left padding, outputs on a 16-byte boundary
    and off it; documents of 0, 1, room - 1, room, room + 1, room + step, room + step + 1 and 3 * room + 1 ids for every (room, step), two
    long documents around a run of empty ones and a run of empty ones at the end"""
    nd = len(env.docs)
    have = {len(d) for d in env.docs}
    k = 0
    seen = set()
    for has_bos, has_eos, room, overlap in shapes(L):
        assert counts_of(room, room - overlap) <= have
        for id_bytes in (2, 4, 8):
            for pad_left in ((False, True) if L <= 7 else (bool(k & 1),)):
                shift = (k >> 1) & 1 if L > 1 else k & 1
                k += 1
                e = expected(env, 0, nd, L, has_bos, has_eos, overlap, pad_left)
                rows = e[0].shape[0]
                how = env.how(0, nd, L, id_bytes, env.bos if has_bos else None, env.eos if has_eos else None, pad_left)
                what = (L, has_bos, has_eos, overlap, id_bytes, pad_left, shift)
                assert env.rows(how, overlap) == rows, what
                check_rows(env, env.windows(how, overlap, rows, shift), e, id_bytes, what)
                seen.add((id_bytes, pad_left, shift))
                # every row of a document but its last is full, and rows of one document follow each other `step` ids apart
                full = e[2] == L
                last = np.append(e[3][1:] != e[3][:-1], True)
                assert (full | last).all() and (e[4][~np.append(True, last[:-1])] >= room - overlap).all()
    assert {(i, p) for i, p, _ in seen} == {(i, p) for i in (2, 4, 8) for p in (False, True)} and {s for _, _, s in seen} == {0, 1}
    if L == 1:
        # two-byte ids, rows of one id: a 16-byte vector holds eight rows - of eight documents inside a run of empty ones, and of a long
        # document's windows and the first empty documents behind it
        rd = expected(env, 0, nd, 1, False, False, 0, False)[3]
        eight = [rd[r:r + 8] for r in range(0, rd.size - 7, 8)]
        assert any(len(set(x.tolist())) == 8 and all(len(env.docs[d]) == 0 for d in x) for x in eight)
        assert any(len(set(x.tolist())) in range(2, 9) and len(env.docs[x[-1]]) == 0 and len(env.docs[x[0]]) > 8 for x in eight)


def test_a_part_of_the_run_and_each_output_null_in_turn(env):
    first, n = env.groups["mixed"]
    first, nd = first - 3, EMPTY_RUN + 12                              # from inside the exact counts over both long documents and the empty run between
    assert first > 0 and first + nd < len(env.docs)
    for L, id_bytes, has_bos, has_eos, overlap, pad_left, shift in ((7, 2, True, False, 1, False, 1), (65, 8, True, True, 62, True, 1), (3, 4, False, False, 0, False, 0)):
        e = expected(env, first, nd, L, has_bos, has_eos, overlap, pad_left)
        rows = e[0].shape[0]
        assert rows > nd and e[3].max() == nd - 1 and e[3].min() == 0
        how = env.how(first, nd, L, id_bytes, env.bos if has_bos else None, env.eos if has_eos else None, pad_left)
        assert env.rows(how, overlap) == rows
        for outputs in ((True, True, True, True), (False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False),
                        (False, False, False, False)):
            check_rows(env, env.windows(how, overlap, rows, shift, outputs), e, id_bytes, (L, id_bytes, outputs), outputs)
        # more room than needed: the rows behind the last stay as they were
        o = Out((rows + 3) * L, id_bytes, shift)
        N.check(N.lib.tm_batch_windows(env.b, C.byref(how), overlap, None, rows + 3, o.ptr, None, None, None, None))
        env.sync()
        assert (o.view(DT[id_bytes])[:rows * L].reshape(rows, L) == e[0]).all() and (o.buf.array[o.off + rows * L * id_bytes:] == FILL).all()
    # no documents: no rows, nothing written
    how = env.how(first, 0, 7, 4, None, None, False)
    assert env.rows(how, 0) == 0
    o = Out(64, 4)
    N.check(N.lib.tm_batch_windows(env.b, C.byref(how), 0, None, 8, o.ptr, None, None, None, None))
    env.sync()
    assert o.untouched()


# ---- spans -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SPAN_LENS)
def test_window_spans(env, L):
    """the pairs of tm_batch_spans / tm_batch_raw_spans in the columns of their ids, (0, 0) on specials and padding; elements of 4 and 8 bytes"""
    fm, nm = env.groups["mixed"]
    k = 0
    seen = set()
    for j, (has_bos, has_eos, room, overlap) in enumerate(shapes(L)):
        for which, span_bytes in (FORMS if L <= 3 else [FORMS[j % 4]]):
            pad_left, shift = bool(k & 1), (k >> 1) % 3
            first, nd = (0, len(env.docs)) if k % 3 else (fm - 2, nm - 7)
            k += 1
            e = expected(env, first, nd, L, has_bos, has_eos, overlap, pad_left, which)
            rows = e[0].shape[0]
            how = env.how(first, nd, L, 4, env.bos if has_bos else None, env.eos if has_eos else None, pad_left)
            fn = N.lib.tm_batch_windows_raw_spans if which == "raw" else N.lib.tm_batch_windows_spans
            out = Out(rows * L * 2, span_bytes, shift)
            N.check(fn(env.b, C.byref(how), overlap, None, rows, out.ptr, span_bytes))
            env.sync()
            what = (L, has_bos, has_eos, overlap, which, span_bytes, pad_left, shift, first)
            got = out.view(np.uint32 if span_bytes == 4 else np.uint64).reshape(rows, L, 2)
            assert out.sentinels_intact() and (got == e[5]).all(), what
            # (0, 0) wherever the row holds no content id, and a content column has the pair of ITS id
            content = e[1].astype(bool)
            if has_bos:
                content[np.arange(rows), np.argmax(e[1], axis=1)] = False
            if has_eos:
                content[np.arange(rows), L - 1 - np.argmax(e[1][:, ::-1], axis=1)] = False
            assert not got[~content].any() and got[content][:, 1].any(), what
            seen.add((which, span_bytes))
    assert seen == {(w, s) for w in ("norm", "raw") for s in (4, 8)}


# ---- nothing disturbed -----------------------------------------------------------------------------------------------------------------------
def test_the_calls_leave_the_batch_as_it_was(env):
    nd = len(env.docs)
    how = env.how(0, nd, 7, 2, env.bos, env.eos, False)
    rows = env.rows(how, 2)                                            # (the grow-only buffers exist from here on)
    out = Out(rows * 7 * 2, 8)
    N.check(N.lib.tm_batch_windows_raw_spans(env.b, C.byref(how), 2, None, rows, out.ptr, 8))

    def state():
        total, toff, ids, miss = env.download(env.b, nd)
        return [np.array([total, int(N.lib.tm_batch_device_bytes(env.b))]), toff, ids, miss, env.ragged(env.b, False), env.ragged(env.b, True)]

    before = state()
    env.windows(how, 2, rows)
    N.check(N.lib.tm_batch_windows_spans(env.b, C.byref(how), 2, None, rows, out.ptr, 8))
    between = state()
    N.check(N.lib.tm_batch_windows_raw_spans(env.b, C.byref(how), 2, None, rows, out.ptr, 8))
    assert env.rows(how, 2) == rows
    after = state()
    for other in (between, after):
        for x, y in zip(before, other):
            assert np.array_equal(x, y)
    assert np.array_equal(before[2], env.ids) and np.array_equal(before[1], env.toff)
    assert np.array_equal(before[4], np.concatenate(env.spans)) and np.array_equal(before[5], np.concatenate(env.raw_spans))


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(env):
    nd = len(env.docs)
    L = 8
    rows = expected(env, 0, nd, L, True, True, 2, False)[0].shape[0]
    o = [Out(rows * L, 8), Out(rows * L, 1), Out(rows, 4), Out(rows, 4), Out(rows, 4)]
    so = Out(rows * L * 2, 8)
    need = C.c_uint64()

    def all_three(how, overlap, rows_cap=rows, b=None):
        """the return codes of the rows call, the ids call and the two span calls"""
        b = b or env.b
        rc = [N.lib.tm_batch_window_rows(b, C.byref(how), overlap, C.byref(need)),
              N.lib.tm_batch_windows(b, C.byref(how), overlap, None, rows_cap, *[x.ptr for x in o]),
              N.lib.tm_batch_windows_spans(b, C.byref(how), overlap, None, rows_cap, so.ptr, 8),
              N.lib.tm_batch_windows_raw_spans(b, C.byref(how), overlap, None, rows_cap, so.ptr, 8)]
        env.sync(b)
        assert all(x.untouched() for x in o + [so])
        return rc

    INV = N.TM_E_INVALID
    both = dict(bos=env.bos, eos=env.eos)
    assert all_three(env.how(0, nd, L, 4, pad_left=False, **both), 6) == [INV] * 4 and b"overlap" in N.lib.tm_last_error()      # overlap == room
    assert all_three(env.how(0, nd, L, 4, pad_left=False, **both), 0xFFFFFFFF) == [INV] * 4
    assert all_three(env.how(0, nd, 2, 4, pad_left=False, **both), 0) == [INV] * 4 and b"row_len" in N.lib.tm_last_error()        # room == 0
    assert all_three(env.how(0, nd, 1, 4, pad_left=False, **both), 0) == [INV] * 4                                                # room < 0
    assert all_three(env.how(0, nd, 1, 4, env.bos, None, False), 0) == [INV] * 4
    assert all_three(env.how(0, nd, L, 4, pad_left=False, flags=KEEP_TAIL, **both), 2) == [INV] * 4 and b"KEEP_TAIL" in N.lib.tm_last_error()
    assert all_three(env.how(0, nd, L, 4, pad_left=False, flags=4, **both), 2) == [INV] * 4                                       # unknown flag
    assert all_three(env.how(0, nd, L, 3, pad_left=False, **both), 2) == [INV] * 4
    assert all_three(env.how(0, nd, L, 2, pad_left=False, bos=65536, eos=None), 2) == [INV] * 4 and b"two bytes" in N.lib.tm_last_error()
    assert all_three(env.how(0, nd, L, 2, pad_left=False, pad_id=70000, **both), 2) == [INV] * 4
    assert all_three(env.how(0, nd, L, 4, pad_left=False, pad_id=NONE, **both), 2) == [INV] * 4
    assert all_three(env.how(nd - 1, 2, L, 4, pad_left=False, **both), 2) == [INV] * 4                                            # beyond the run
    # rows_cap one too small: the number is in the message
    how = env.how(0, nd, L, 8, pad_left=False, **both)
    for rc in all_three(how, 2, rows - 1)[1:]:
        assert rc == N.TM_E_NOSPACE and str(rows).encode() in N.lib.tm_last_error()
    assert all_three(how, 2, rows - 1)[0] == N.TM_OK and need.value == rows
    assert N.lib.tm_batch_windows_spans(env.b, C.byref(how), 2, None, rows, so.ptr, 2) == INV                                     # span_bytes
    assert N.lib.tm_batch_windows(env.b, C.byref(how), 2, None, rows, None, None, None, None, None) == INV
    assert N.lib.tm_batch_window_rows(env.b, C.byref(how), 2, None) == INV
    env.sync()
    assert so.untouched()
    b = env.new_batch(1 << 16, 64)
    try:
        docs = [env.raw[env.groups["mixed"][0] + EMPTY_RUN + 2], b"", b"abc" * 30]
        how3 = env.how(0, 3, L, 8, pad_left=False, **both)
        assert all_three(how3, 2, b=b) == [INV] * 4 and b"no ids" in N.lib.tm_last_error()                                        # no run yet
        # a batch uploaded NORMALIZED has no raw text to point into: the raw form is refused, the others work
        text, offs = tm.pack_documents([env.v.normalize(d) for d in docs])
        N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(offs), 3))
        N.check(N.lib.tm_batch_run(b, None))
        n3 = env.rows(how3, 2, b)
        assert n3 > 3 and N.lib.tm_batch_windows_raw_spans(b, C.byref(how3), 2, None, rows, so.ptr, 8) == INV
        env.sync(b)
        assert so.untouched()
        ok = Out(n3 * L * 2, 8)
        N.check(N.lib.tm_batch_windows_spans(b, C.byref(how3), 2, None, n3, ok.ptr, 8))
        env.sync(b)
        assert ok.sentinels_intact() and ok.view(np.uint64).any()
        # ids that came from no walk have no spans: tm_batch_load_ids behind a raw run
        env.run_raw(b, docs)
        src = Out(4 * 8, 4)
        src.view(np.uint32)[:] = np.arange(32) % 5
        N.check(N.lib.tm_batch_load_ids(b, src.ptr, 4, 8, 4, None, NONE, NONE, NONE, None))
        how4 = env.how(0, 4, 6, 8, pad_left=False, **both)
        assert N.lib.tm_batch_windows_spans(b, C.byref(how4), 1, None, rows, so.ptr, 8) == INV
        assert N.lib.tm_batch_windows_raw_spans(b, C.byref(how4), 1, None, rows, so.ptr, 8) == INV
        env.sync(b)
        assert so.untouched()
        # ... but they have windows: four rows of eight ids, room 4, step 3 -> 1 + ceil(4 / 3) = 3 rows each
        e = np_windows([np.arange(8 * r, 8 * r + 8) % 5 for r in range(4)], 6, env.pad, env.bos, env.eos, 1, False)
        assert env.rows(how4, 1, b) == 12 == e[0].shape[0]
        got = Out(12 * 6, 8)
        N.check(N.lib.tm_batch_windows(b, C.byref(how4), 1, None, 12, got.ptr, None, None, None, None))
        env.sync(b)
        assert (got.view(np.uint64).reshape(12, 6) == e[0]).all()
    finally:
        N.lib.tm_batch_free(b)
    # the batch of the fixture is as good as before
    e = expected(env, 0, nd, L, True, True, 2, False)
    check_rows(env, env.windows(env.how(0, nd, L, 8, pad_left=False, **both), 2, rows), e, 8, "after the errors")

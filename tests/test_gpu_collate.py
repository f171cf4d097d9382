"""-m gpu: tm_batch_collate / tm_batch_pack / tm_batch_load_ids (tokenmonster_amd/csrc/tm_collate.hip) at the C ABI, outputs in tm_host_alloc
memory, against a numpy statement of their rules.  The ids come from tm_batch_download of the same run: this file tests layout, not
tokenization.  tests/test_collate_emulated.py runs this file on the emulated device (tools/emu), without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import tokenmonster_amd as tm
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth
from conftest import fuzz_text, fuzz_vocab_tokens
from fixed_shape import Collate, Out, spec, DT, FILL, KEEP_TAIL, NONE, PAD_LEFT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_LENS = [1, 2, 3, 7, 63, 64, 65, 257]          # (2: the number of specials when both are given; 1 covers it for one special)
PACK_LENS = [1, 7, 64, 257]


# ---- the rules, in numpy ---------------------------------------------------------------------------------------------------------------
def truncated(doc, L, bos, eos, flags):
    room = L - (bos is not None) - (eos is not None)
    m = min(len(doc), room)
    return doc[len(doc) - m:] if flags & KEEP_TAIL else doc[:m]


def np_collate(docs, L, pad, bos, eos, flags, dtype):
    ids = np.full((len(docs), L), pad, dtype=dtype)
    mask = np.zeros((len(docs), L), dtype=np.uint8)
    lens = np.zeros(len(docs), dtype=np.uint32)
    for r, doc in enumerate(docs):
        row = ([bos] if bos is not None else []) + list(truncated(doc, L, bos, eos, flags)) + ([eos] if eos is not None else [])
        lo = L - len(row) if flags & PAD_LEFT else 0
        ids[r, lo:lo + len(row)] = row
        mask[r, lo:lo + len(row)] = 1
        lens[r] = len(row)
    return ids, mask, lens


def np_pack(docs, L, pad, eos, dtype):
    s, di, po = [], [], []
    for d, doc in enumerate(docs):
        n = len(doc) + (eos is not None)
        s += list(doc) + ([eos] if eos is not None else [])
        di += [d] * n
        po += list(range(n))
    rows = (len(s) + L - 1) // L
    fill = rows * L - len(s)
    return (np.array(s + [pad] * fill, dtype=dtype).reshape(rows, L), np.array(di + [0xFFFFFFFF] * fill, dtype=np.uint32).reshape(rows, L),
            np.array(po + [0] * fill, dtype=np.uint32).reshape(rows, L), len(s))


def np_load(rows, lengths, pad, bos, eos):
    out = []
    for r, row in enumerate(rows):
        row = [int(x) for x in row]
        start = 0
        if pad is not None:
            while start < len(row) and row[start] == pad:
                start += 1
        end = len(row) if lengths is None else min(start + int(lengths[r]), len(row))
        if bos is not None and start < end and row[start] == bos:
            start += 1
        if eos is not None and eos in row[start:end]:
            end = start + row[start:end].index(eos)
        out.append(np.array(row[start:end], dtype=np.uint32))
    return out


# ---- one vocabulary, one run for the whole file -----------------------------------------------------------------------------------------
class Env:
    def __init__(self):
        rng = np.random.default_rng(77001)
        self.img = synth.build_vocab(fuzz_vocab_tokens(rng, 2, 200), capcode=2, charset=1, with_unk=True)
        self.v = tm.Vocab(self.img)
        self.n_ids = self.v.n_ids()
        self.pad, self.bos, self.eos = self.n_ids + 5, self.n_ids + 6, self.n_ids + 7          # (no document holds them)
        self.max_docs = 4096
        self.b = self.new_batch(1 << 20)
        self.b2 = self.new_batch(1 << 16)                # what tm_batch_load_ids fills
        # documents with EXACT id counts: a byte no token has ('x') is one unk id wherever it stands, so text + 'x' * k has k more ids than
        # text + 'x' has less one.  First run: the counts of the texts; second run: the documents.  (Checked below.)
        want = {}                                        # group -> list of id counts
        row = set()
        for L in ROW_LENS:
            for ns in (0, 1, 2):
                row |= {0, 1, 3 * L} | {c for c in (L - ns - 1, L - ns, L - ns + 1) if c >= 0}
        want["row"] = sorted(row) + [5000]
        for L in PACK_LENS:
            # ends on row ends with EOS (L-1 and 2L-1 ids), over five rows, 600 empty documents in a row, and two documents that fill the
            # last row exactly: the one before last with EOS, the last without (t in 1 .. L)
            g = [L - 1, 2 * L - 1, 5 * L + 2] + [0] * 600 + [3]
            g.append(L - (sum(g) + len(g) + 1) % L)                      # with EOS: full after this document
            g.append(L - sum(g) % L)                                     # without EOS: full after this one
            want["pack%d" % L] = g
        texts, self.groups = [], {}
        for name, counts in want.items():
            self.groups[name] = (len(texts), len(counts))
            texts += [fuzz_text(rng, 2, int(c * 1.2)) if c >= 8 else b"" for c in counts]
        self.groups["random"] = (len(texts), 1000)
        texts += [fuzz_text(rng, 2, int(n)) for n in rng.integers(0, 61, size=1000)]           # 0 .. about 25 ids: 0 .. 3L at L = 7
        counts = [c for cs in want.values() for c in cs]
        first, _ = self.run([t + b"x" for t in texts[:len(counts)]])
        docs = []
        for t, c, have in zip(texts, counts, first):
            while len(have) - 1 > c:                     # too many already: a shorter text (rare)
                t = t[:len(t) // 2]
                have = self.run([t + b"x"])[0][0]
            docs.append(t + b"x" * (c - (len(have) - 1)))
        docs += texts[len(counts):]
        self.docs, _ = self.run(docs)
        assert [len(d) for d in self.docs[:len(counts)]] == counts, "the fixture's documents do not have the id counts it was built for"
        assert len(self.docs) <= self.max_docs

    def new_batch(self, max_bytes, v=None, max_docs=None):
        b = C.c_void_p()
        N.check(N.lib.tm_batch_create((v or self.v).handle, max_bytes, max_docs or self.max_docs, C.byref(b)))
        return b

    def run(self, docs, b=None):
        """tokenize on the batch -> (list of u32 id arrays as tm_batch_download returns them, missing)"""
        b = b or self.b
        text, offs = tm.pack_documents(docs)
        N.check(N.lib.tm_batch_upload(b, N.ptr(text), N.ptr(offs), len(docs)))
        N.check(N.lib.tm_batch_run(b, None))
        return self.download(b, len(docs))

    def download(self, b, nd):
        n = C.c_uint64()
        N.check(N.lib.tm_batch_totals(b, C.byref(n), None))
        ids = np.zeros(max(n.value, 1), dtype=np.uint32)
        toff = np.zeros(nd + 1, dtype=np.uint64)
        miss = np.zeros(max(nd, 1), dtype=np.uint32)
        N.check(N.lib.tm_batch_download(b, N.ptr(ids), n.value, N.ptr(toff), N.ptr(miss)))
        assert toff[nd] == n.value
        return [ids[int(toff[d]):int(toff[d + 1])] for d in range(nd)], miss[:nd]

    def sync(self, b=None):
        N.check(N.lib.tm_batch_totals(b or self.b, None, None))           # (everything here runs on the NULL stream, which this waits for)

    def group(self, name):
        f, n = self.groups[name]
        return f, n, self.docs[f:f + n]

    def collate(self, first, nd, L, id_bytes, bos, eos, flags, shift=0, with_mask=True, with_lengths=True, b=None):
        how = Collate(first, nd, L, id_bytes, self.pad, spec(bos), spec(eos), flags)
        ids, mask, lens = Out(nd * L, id_bytes, shift), Out(nd * L, 1, shift), Out(nd, 4, 0)
        N.check(N.lib.tm_batch_collate(b or self.b, C.byref(how), None, ids.ptr, mask.ptr if with_mask else None, lens.ptr if with_lengths else None))
        self.sync(b)
        return ids, mask, lens

    def load(self, rows_ptr, nrows, L, id_bytes, lengths_ptr, pad, bos, eos):
        N.check(N.lib.tm_batch_load_ids(self.b2, rows_ptr, nrows, L, id_bytes, lengths_ptr, spec(pad), spec(bos), spec(eos), None))
        return self.download(self.b2, nrows)


_env = None


@pytest.fixture(scope="module")
def env():
    global _env
    if _env is None:
        _env = Env()
    return _env


def same(got, exp):
    return len(got) == len(exp) and all(a.size == b.size and (a == b).all() for a, b in zip(got, exp))


SPECIALS = [(False, False), (True, False), (False, True), (True, True)]
pytestmark = pytest.mark.gpu


# ---- row mode ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ROW_LENS)
def test_rows_every_special_flag_and_width(env, L):
    """documents of 0, 1, L-ns-1, L-ns, L-ns+1, 3L and 5000 ids (and the same for the other row lengths); each specials combination, each
    flags value, ids of 2, 4 and 8 bytes; mask and lengths agree with the ids; nothing around the outputs is touched; then the way back:
    tm_batch_load_ids of the rows + tm_batch_download returns the truncated ids"""
    first, nd, docs = env.group("row")
    assert {0, 1, 3 * L, 5000} <= {len(d) for d in docs}
    for has_bos, has_eos in SPECIALS:
        ns = has_bos + has_eos
        if L < ns:
            continue
        assert {c for c in (L - ns - 1, L - ns, L - ns + 1) if c >= 0} <= {len(d) for d in docs}
        bos, eos = env.bos if has_bos else None, env.eos if has_eos else None
        for flags in (0, PAD_LEFT, KEEP_TAIL, PAD_LEFT | KEEP_TAIL):
            for id_bytes in (2, 4, 8):
                shift = (flags + id_bytes // 2) & 1            # (aligned and one element off a 16-byte boundary, both for every width)
                ids, mask, lens = env.collate(first, nd, L, id_bytes, bos, eos, flags, shift=shift)
                e_ids, e_mask, e_lens = np_collate(docs, L, env.pad, bos, eos, flags, DT[id_bytes])
                what = (L, has_bos, has_eos, flags, id_bytes)
                assert (ids.view(DT[id_bytes]).reshape(nd, L) == e_ids).all(), what
                assert (mask.view(np.uint8).reshape(nd, L) == e_mask).all(), what
                assert (lens.view(np.uint32) == e_lens).all(), what
                assert ids.sentinels_intact() and mask.sentinels_intact() and lens.sentinels_intact(), what
                # the way back, with the lengths and without
                trunc = [np.asarray(truncated(d, L, bos, eos, flags), dtype=np.uint32) for d in docs]
                got, miss = env.load(ids.ptr, nd, L, id_bytes, lens.ptr, env.pad, bos, eos)
                assert same(got, trunc) and not miss.any(), what
                got, _ = env.load(ids.ptr, nd, L, id_bytes, None, env.pad, bos, eos)
                assert same(got, np_load(e_ids, None, env.pad, bos, eos)), what
                if has_eos or (flags & PAD_LEFT):               # (without lengths and EOS, right padding counts as ids)
                    assert same(got, trunc), what


def test_rows_of_a_part_of_the_run_and_optional_outputs(env):
    first, nd, docs = env.group("row")
    L = 65
    for id_bytes, shift in ((2, 1), (8, 1), (4, 0)):
        e_ids, e_mask, e_lens = np_collate(docs[3:nd - 2], L, env.pad, env.bos, None, KEEP_TAIL, DT[id_bytes])
        for with_mask, with_lengths in ((True, False), (False, True), (False, False)):
            ids, mask, lens = env.collate(first + 3, nd - 5, L, id_bytes, env.bos, None, KEEP_TAIL, shift, with_mask, with_lengths)
            assert (ids.view(DT[id_bytes]).reshape(nd - 5, L) == e_ids).all() and ids.sentinels_intact()
            assert (mask.view(np.uint8).reshape(nd - 5, L) == e_mask).all() if with_mask else mask.untouched()
            assert (lens.view(np.uint32) == e_lens).all() if with_lengths else lens.untouched()
    ids, _, _ = env.collate(first, 0, L, 4, None, None, 0)            # no rows: nothing is written
    assert ids.untouched()


@pytest.mark.parametrize("L,id_bytes", [(7, 2), (7, 8), (20, 4)])
def test_a_thousand_rows_of_random_lengths(env, L, id_bytes):
    first, nd, docs = env.group("random")
    lens_seen = {len(d) for d in docs}
    assert nd == 1000 and 0 in lens_seen and max(lens_seen) > 2 * 7
    for flags in (0, PAD_LEFT | KEEP_TAIL):
        ids, mask, lens = env.collate(first, nd, L, id_bytes, env.bos, env.eos, flags, shift=1)
        e_ids, e_mask, e_lens = np_collate(docs, L, env.pad, env.bos, env.eos, flags, DT[id_bytes])
        assert (ids.view(DT[id_bytes]).reshape(nd, L) == e_ids).all() and (mask.view(np.uint8).reshape(nd, L) == e_mask).all()
        assert (lens.view(np.uint32) == e_lens).all() and ids.sentinels_intact() and mask.sentinels_intact()


# ---- pack mode -----------------------------------------------------------------------------------------------------------------------------
def pack(env, first, nd, L, id_bytes, eos, rows_cap=None, shift=0, extras=True):
    how = Collate(first, nd, L, id_bytes, env.pad, NONE, spec(eos), 0)
    need = C.c_uint64()
    N.check(N.lib.tm_batch_pack_rows(env.b, C.byref(how), C.byref(need)))
    cap = need.value if rows_cap is None else rows_cap
    ids, di, po = Out(cap * L, id_bytes, shift), Out(cap * L, 4, shift), Out(cap * L, 4, 0)
    rc = N.lib.tm_batch_pack(env.b, C.byref(how), None, cap, ids.ptr, di.ptr if extras else None, po.ptr if extras else None)
    env.sync()
    return rc, need.value, ids, di, po


@pytest.mark.parametrize("L", PACK_LENS)
def test_pack_stream(env, L):
    """document ends on row ends, a document over five rows, 600 empty documents in a row (gone from the stream without EOS), a last row that
    is partial and one that is exactly full, doc_index and position, ids of 2 and 8 bytes, an output one element off a 16-byte boundary"""
    first, nd, docs = env.group("pack%d" % L)
    assert len(docs[2]) > 5 * L and sum(1 for d in docs if len(d) == 0) >= 600
    full = set()
    for eos in (env.eos, None):
        for use in (nd, nd - 1):
            for id_bytes, shift in ((2, 1), (8, 0)):
                e_ids, e_di, e_po, stream_len = np_pack(docs[:use], L, env.pad, eos, DT[id_bytes])
                rc, need, ids, di, po = pack(env, first, use, L, id_bytes, eos, shift=shift)
                what = (L, eos, use, id_bytes)
                assert rc == N.TM_OK and need == e_ids.shape[0] == (stream_len + L - 1) // L, what
                assert (ids.view(DT[id_bytes]).reshape(need, L) == e_ids).all(), what
                assert (di.view(np.uint32).reshape(need, L) == e_di).all() and (po.view(np.uint32).reshape(need, L) == e_po).all(), what
                assert ids.sentinels_intact() and di.sentinels_intact() and po.sentinels_intact(), what
                full.add((eos is not None, stream_len % L == 0))
            if eos is not None and use == nd:
                ends = np.cumsum([len(d) + 1 for d in docs[:2]])
                assert (ends % L == 0).all()                        # the first two documents end on row ends
    assert (True, True) in full and (False, True) in full           # exactly full, with and without EOS
    if L > 1:
        assert (True, False) in full or (False, False) in full      # and a partial last row
    # without the optional outputs; and rows_cap one too small
    rc, need, ids, di, po = pack(env, first, nd, L, 2, env.eos, extras=False)
    assert rc == N.TM_OK and di.untouched() and po.untouched()
    assert (ids.view(np.uint16).reshape(need, L) == np_pack(docs, L, env.pad, env.eos, np.uint16)[0]).all()
    rc, need2, ids, di, po = pack(env, first, nd, L, 2, env.eos, rows_cap=need - 1)
    assert rc == N.TM_E_NOSPACE and need2 == need and str(need).encode() in N.lib.tm_last_error()
    assert ids.untouched() and di.untouched() and po.untouched()


def test_pack_a_part_of_the_run(env):
    first, nd, docs = env.group("random")
    e_ids, e_di, e_po, _ = np_pack(docs[100:900], 64, env.pad, env.eos, np.uint32)
    rc, need, ids, di, po = pack(env, first + 100, 800, 64, 4, env.eos, shift=1)
    assert rc == N.TM_OK and (ids.view(np.uint32).reshape(need, 64) == e_ids).all()
    assert (di.view(np.uint32).reshape(need, 64) == e_di).all() and (po.view(np.uint32).reshape(need, 64) == e_po).all()


# ---- load ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id_bytes", [2, 4, 8])
def test_load_rows_by_hand(env, id_bytes):
    """lengths given and not given; a row without EOS, a row that is all pad, a row that is only BOS EOS, left and right padding in one tensor"""
    P, B, E = env.pad, env.bos, env.eos
    L = 70                                                           # (more than a wavefront of columns)
    body = list(range(1, 60))
    rows = [[B] + body[:40] + [E] + [P] * 28,                        # right padded
            [P] * 28 + [B] + body[:40] + [E],                        # left padded
            body + body[:11],                                        # no EOS, no BOS, full
            [P] * L,                                                 # all pad
            [B, E] + [P] * 68,                                       # empty document
            [P] * 65 + [B, 7, 8, 9, 10],                             # left padded, no EOS
            [B] + body[:10] + [E] + body[:5] + [E] + [P] * 52]       # two EOS: the first one ends the row
    lengths = np.array([42, 42, 70, 0, 2, 5, 12], dtype=np.uint32)
    src = Out(len(rows) * L, id_bytes, 1)
    src.view(DT[id_bytes])[:] = np.array(rows, dtype=DT[id_bytes]).reshape(-1)
    lens = Out(len(rows), 4)
    lens.view(np.uint32)[:] = lengths
    for pad, bos, eos, lp in ((P, B, E, None), (P, B, E, lens), (P, None, None, lens), (None, None, None, None), (P, B, None, lens), (None, None, E, None)):
        got, miss = env.load(src.ptr, len(rows), L, id_bytes, lp.ptr if lp else None, pad, bos, eos)
        exp = np_load(rows, lengths if lp else None, pad, bos, eos)
        assert same(got, exp) and not miss.any(), (pad, bos, eos, lp is not None, [g.tolist() for g in got])
    assert same(env.load(src.ptr, len(rows), L, id_bytes, None, P, B, E)[0][:2], [np.array(body[:40], dtype=np.uint32)] * 2)
    assert src.sentinels_intact()


@pytest.mark.parametrize("raw", [0, 1])
def test_loaded_ids_decode_like_the_ragged_ids(env, raw):
    first, nd, docs = env.group("random")
    L = 24
    ids, _, lens = env.collate(first, nd, L, 4, env.bos, env.eos, 0)
    trunc = [np.asarray(truncated(d, L, env.bos, env.eos, 0), dtype=np.uint32) for d in docs]
    got, _ = env.load(ids.ptr, nd, L, 4, lens.ptr, env.pad, env.bos, env.eos)
    assert same(got, trunc)
    nbytes, host_docs = C.c_uint64(), C.c_uint32()
    N.check(N.lib.tm_batch_decode(env.b2, raw, None, C.byref(nbytes), C.byref(host_docs)))
    ooff = np.zeros(nd + 1, dtype=np.uint64)
    out = np.zeros(sum(t.size for t in trunc) * 48 + 64, dtype=np.uint8)
    N.check(N.lib.tm_batch_decoded_download(env.b2, N.ptr(out), out.size, N.ptr(ooff)))
    toff = np.zeros(nd + 1, dtype=np.uint64)
    np.cumsum([t.size for t in trunc], out=toff[1:])
    e_out, e_off = env.v.decode_packed(np.concatenate(trunc), toff, raw=bool(raw))
    assert (ooff == e_off).all() and (out[:int(ooff[nd])] == e_out).all() and int(ooff[nd]) > 1000


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_batch_usable(env):
    first, nd, docs = env.group("row")
    out = Out(nd * 300, 8)

    def collate_rc(b, **kw):
        f = dict(first_doc=first, ndocs=nd, row_len=64, id_bytes=4, pad_id=env.pad, bos_id=env.bos, eos_id=env.eos, flags=0)
        f.update(kw)
        how = Collate(*[f[n] for n, _ in Collate._fields_])
        return N.lib.tm_batch_collate(b, C.byref(how), None, out.ptr, None, None)

    assert collate_rc(env.b, row_len=1) == N.TM_E_INVALID and b"row_len" in N.lib.tm_last_error()        # L < nspecial
    assert collate_rc(env.b, row_len=0, bos_id=NONE, eos_id=NONE) == N.TM_E_INVALID
    assert collate_rc(env.b, id_bytes=3) == N.TM_E_INVALID and b"id_bytes" in N.lib.tm_last_error()
    assert collate_rc(env.b, pad_id=NONE) == N.TM_E_INVALID
    assert collate_rc(env.b, id_bytes=2, pad_id=65536) == N.TM_E_INVALID
    assert collate_rc(env.b, flags=4) == N.TM_E_INVALID
    assert collate_rc(env.b, first_doc=len(env.docs) - 1, ndocs=2) == N.TM_E_INVALID                     # beyond the run
    assert collate_rc(env.b, first_doc=0xFFFFFFFF, ndocs=2) == N.TM_E_INVALID
    how = Collate(first, nd, 64, 4, env.pad, NONE, env.eos, 0)
    need = C.c_uint64()
    how.id_bytes = 3
    assert N.lib.tm_batch_pack_rows(env.b, C.byref(how), C.byref(need)) == N.TM_E_INVALID
    assert N.lib.tm_batch_pack(env.b, C.byref(how), None, 1 << 20, out.ptr, None, None) == N.TM_E_INVALID
    assert N.lib.tm_batch_load_ids(env.b2, out.ptr, 4, 8, 3, None, NONE, NONE, NONE, None) == N.TM_E_INVALID
    assert N.lib.tm_batch_load_ids(env.b2, out.ptr, env.max_docs + 1, 1, 4, None, NONE, NONE, NONE, None) == N.TM_E_LIMIT      # nrows > max_docs
    assert out.untouched()
    # before any run, and between an upload and its run
    fresh = env.new_batch(1 << 16)
    try:
        assert collate_rc(fresh, first_doc=0, ndocs=0) == N.TM_E_INVALID and b"no ids" in N.lib.tm_last_error()
        how = Collate(0, 0, 64, 4, env.pad, NONE, env.eos, 0)
        assert N.lib.tm_batch_pack_rows(fresh, C.byref(how), C.byref(need)) == N.TM_E_INVALID
        text, offs = tm.pack_documents([b" abc abc", b" de"])
        N.check(N.lib.tm_batch_upload(fresh, N.ptr(text), N.ptr(offs), 2))
        assert collate_rc(fresh, first_doc=0, ndocs=2) == N.TM_E_INVALID
        got, _ = env.run([b" abc abc", b" de"], fresh)                                                   # it still runs
        exp, _ = env.v.tokenize_normalized([b" abc abc", b" de"])
        assert same(got, exp)
        ids, _, lens = env.collate(0, 2, 8, 4, None, None, 0, b=fresh)
        assert (lens.view(np.uint32) == [min(len(e), 8) for e in exp]).all()
    finally:
        N.lib.tm_batch_free(fresh)
    # the batch of the fixture is as good as before
    ids, _, _ = env.collate(first, nd, 64, 4, env.bos, env.eos, 0)
    assert (ids.view(np.uint32).reshape(nd, 64) == np_collate(docs, 64, env.pad, env.bos, env.eos, 0, np.uint32)[0]).all()
    assert same(env.download(env.b, len(env.docs))[0], env.docs)


def test_two_byte_ids_need_a_vocabulary_that_fits(env):
    rng = np.random.default_rng(77002)
    toks = fuzz_vocab_tokens(rng, 2, 100) + [bytes([0x7F, 0x30 + k % 40, 0x30 + (k // 40) % 40, 0x30 + k // 1600]) for k in range(66_000)]
    v = tm.Vocab(synth.build_vocab(list(dict.fromkeys(toks)), capcode=2, charset=1, with_unk=True))
    assert v.n_ids() > 65536
    b = env.new_batch(1 << 16, v, 16)
    try:
        docs = [fuzz_text(rng, 2, 300), b"", fuzz_text(rng, 2, 40)]
        got, _ = env.run(docs, b)
        out, need = Out(3 * 16, 8), C.c_uint64()
        for id_bytes, rc in ((2, N.TM_E_INVALID), (4, N.TM_OK)):
            how = Collate(0, 3, 16, id_bytes, 70000 if id_bytes == 4 else 1, NONE, NONE, 0)
            assert N.lib.tm_batch_collate(b, C.byref(how), None, out.ptr, None, None) == rc
            assert N.lib.tm_batch_pack_rows(b, C.byref(how), C.byref(need)) == rc
            assert N.lib.tm_batch_load_ids(b, out.ptr, 3, 16, id_bytes, None, NONE, NONE, NONE, None) == rc
        assert same(env.run(docs, b)[0], got)
    finally:
        N.lib.tm_batch_free(b)
        v.close()

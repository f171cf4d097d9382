"""-m gpu: what the host-buffer calls of tokenmonster_amd/csrc/tm_host.hip promise at their edges - tm_tokenize_batch, tm_tokenize_batch_spans,
tm_tokenize_batch_raw_spans, tm_tokenize_batch_serialized, and tm_decode_batch beside tm_batch_decode + tm_batch_decoded_download.  An empty
batch, a capacity that is exactly enough, one that is one id (one byte) short, outputs the header allows to be NULL and outputs it does not -
and after every refusal a second, correct call on the same vocabulary, which shows that the lane went back to the pool with nothing in
flight.  The ids and spans themselves are measured against the batch path (tm_batch_run + tm_batch_download + tm_batch_spans /
tm_batch_raw_spans) on the same input; that path is the one tests/test_gpu_spans.py and tests/test_gpu_raw_spans.py hold against the oracle.
tests/test_one_shot_contract_emulated.py runs this file on the emulated device."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_spans as S
from test_gpu_spans import Out, download, new_batch

pytestmark = pytest.mark.gpu

CALLS = ("ids", "spans", "raw_spans", "serialized")
VOCABS = ("id_per_byte", "wide")          # at most 65 536 ids (two-byte serialized form) / more (three bytes): tests/test_gpu_spans.py builds both
MARK64, MARK32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5


def _mods():
    return S._mods()


def documents():
    """empty | one byte | three 256-byte segments | a character without a token"""
    rng = np.random.default_rng(77)
    long_doc = bytes(rng.choice(np.frombuffer(b"qrstuvwx   ", dtype=np.uint8), size=600))
    docs = [b"", b"q", b"Qr " + long_doc[3:], b"qr st %uv wx"]
    assert (len(docs[2]) + 255) // 256 == 3
    return docs


class Ref:
    """the batch path on the four documents, once per vocabulary and kind of text: ids, offsets, missing counts, spans (never changed)"""

    def __init__(self, name):
        tm, N, _ = _mods()
        self.v = S.case(name).v
        self.enc = 2 if self.v.n_ids() <= 65536 else 3
        self.docs = documents()
        self.text, self.offs = tm.pack_documents(self.docs)
        self.nd = len(self.docs)
        b = new_batch(self.v, 8192, 16)
        try:
            self.by_raw = {}
            for raw in (False, True):
                if raw:
                    N.check(N.lib.tm_batch_upload_raw(b, N.ptr(self.text), N.ptr(self.offs), self.nd))
                    N.check(N.lib.tm_batch_normalize(b, None))
                else:
                    N.check(N.lib.tm_batch_upload(b, N.ptr(self.text), N.ptr(self.offs), self.nd))
                N.check(N.lib.tm_batch_run(b, None))
                ids, toff, miss, total, _ = download(b, self.nd)
                out = Out(2 * total, 4)
                if raw:
                    N.check(N.lib.tm_batch_raw_spans(b, None, out.ptr, total, None))
                else:
                    N.check(N.lib.tm_batch_spans(b, None, out.ptr, total))
                N.check(N.lib.tm_batch_totals(b, None, None))
                assert out.sentinels_intact()
                assert total > 600 // 8 and int(miss[3]) >= 1 and int(toff[1]) == 0
                self.by_raw[raw] = (ids.copy(), toff.copy(), miss.copy(), out.view(np.uint32).copy())
        finally:
            N.lib.tm_batch_free(b)


_refs = {}


def ref(name):
    if name not in _refs:
        _refs[name] = Ref(name)
    return _refs[name]


class Result:
    pass


def one_shot(r, call, cap, ndocs=None, toff_null=False, miss_null=False, tok_null=False, sp_null=False, enc_null=False):
    """one call with `cap` ids (bytes for the serialized form) of room; every output starts as a sentinel"""
    _, N, _ = _mods()
    nd = r.nd if ndocs is None else ndocs
    x = Result()
    x.toff = np.full(r.nd + 1, MARK64, dtype=np.uint64)
    x.miss = np.full(r.nd, MARK32, dtype=np.uint32)
    x.tok = Out(max(cap, 1), 1 if call == "serialized" else 4)
    x.sp = Out(2 * max(cap, 1), 4)
    x.enc_used = C.c_uint32(MARK32)
    toff, miss = None if toff_null else N.ptr(x.toff), None if miss_null else N.ptr(x.miss)
    tok, sp = None if tok_null else x.tok.ptr, None if sp_null else x.sp.ptr
    text, offs = (N.ptr(r.text), N.ptr(r.offs)) if nd else (None, None)
    if call == "ids":
        x.rc = N.lib.tm_tokenize_batch(r.v.handle, text, offs, nd, tok, cap, toff, miss)
    elif call == "spans":
        x.rc = N.lib.tm_tokenize_batch_spans(r.v.handle, text, offs, nd, tok, cap, toff, sp, miss)
    elif call == "raw_spans":
        x.rc = N.lib.tm_tokenize_batch_raw_spans(r.v.handle, text, offs, nd, tok, cap, toff, sp, miss)
    else:
        x.rc = N.lib.tm_tokenize_batch_serialized(r.v.handle, text, offs, nd, 0, tok, cap, toff, miss, None if enc_null else C.byref(x.enc_used))
    return x


def expected(r, call):
    """-> (capacity exactly sufficient, the id output as bytes, offsets, missing, spans or None)"""
    ids, toff, miss, spans = r.by_raw[call == "raw_spans"]
    if call == "serialized":
        packed = np.ascontiguousarray(ids.astype("<u4").view(np.uint8).reshape(-1, 4)[:, :r.enc]).reshape(-1)
        return ids.size * r.enc, packed, toff * np.uint64(r.enc), miss, None
    return ids.size, ids.view(np.uint8), toff, miss, spans if call != "ids" else None


def check_filled(r, call, x, toff=True, miss=True, ids=True):
    cap, e_bytes, e_toff, e_miss, e_sp = expected(r, call)
    if toff:
        assert np.array_equal(x.toff, e_toff)
    if miss:
        assert np.array_equal(x.miss, e_miss)
    if ids:
        assert x.tok.sentinels_intact() and np.array_equal(x.tok.view(np.uint8)[:e_bytes.size], e_bytes)
        if e_sp is not None:
            assert x.sp.sentinels_intact() and np.array_equal(x.sp.view(np.uint32)[:e_sp.size], e_sp)
        else:
            assert x.sp.untouched()
    else:
        assert x.tok.untouched() and x.sp.untouched()


def check_lane_is_clean(r, call):
    """a correct call behind a refused one gives the right ids, offsets and counts"""
    _, N, _ = _mods()
    x = one_shot(r, call, expected(r, call)[0])
    assert x.rc == N.TM_OK
    check_filled(r, call, x)


@pytest.mark.parametrize("name", VOCABS)
@pytest.mark.parametrize("call", CALLS)
def test_empty_batch(call, name):
    _, N, _ = _mods()
    r = ref(name)
    x = one_shot(r, call, 16, ndocs=0)
    assert x.rc == N.TM_OK
    assert int(x.toff[0]) == 0 and (x.toff[1:] == MARK64).all()          # tok_offsets[0] / byte_offsets[0], and nothing behind it
    assert (x.miss == MARK32).all() and x.tok.untouched() and x.sp.untouched()
    if call == "serialized":
        assert x.enc_used.value == r.enc
    # ... and without the offsets
    x = one_shot(r, call, 16, ndocs=0, toff_null=True, miss_null=True)
    assert x.rc == N.TM_OK and x.tok.untouched() and x.sp.untouched()
    check_lane_is_clean(r, call)


@pytest.mark.parametrize("name", VOCABS)
@pytest.mark.parametrize("call", CALLS)
def test_capacity_exactly_sufficient(call, name):
    _, N, _ = _mods()
    r = ref(name)
    x = one_shot(r, call, expected(r, call)[0])
    assert x.rc == N.TM_OK
    check_filled(r, call, x)
    if call == "serialized":
        assert x.enc_used.value == r.enc
    if call == "spans":               # already-normalized text: the one-shot ids are tm_tokenize_batch's
        assert np.array_equal(x.tok.view(np.uint8), one_shot(r, "ids", expected(r, "ids")[0]).tok.view(np.uint8))


@pytest.mark.parametrize("name", VOCABS)
@pytest.mark.parametrize("call", CALLS)
def test_capacity_one_short(call, name):
    """TM_E_NOSPACE: the three id calls fill tok_offsets and missing and leave ids and spans alone; the serialized call fills byte_offsets and
    missing (and encoding_length_used) and leaves bytes_out alone"""
    _, N, _ = _mods()
    r = ref(name)
    x = one_shot(r, call, expected(r, call)[0] - 1)
    assert x.rc == N.TM_E_NOSPACE
    check_filled(r, call, x, ids=False)
    if call == "serialized":
        assert x.enc_used.value == r.enc
    check_lane_is_clean(r, call)
    # the same without the offsets and the counts: still refused, still nothing written
    x = one_shot(r, call, expected(r, call)[0] - 1, toff_null=True, miss_null=True)
    assert x.rc == N.TM_E_NOSPACE and x.tok.untouched() and x.sp.untouched()
    assert (x.toff == MARK64).all() and (x.miss == MARK32).all()
    check_lane_is_clean(r, call)


@pytest.mark.parametrize("name", VOCABS)
@pytest.mark.parametrize("call", CALLS)
def test_optional_outputs_may_be_null(call, name):
    _, N, _ = _mods()
    r = ref(name)
    cap = expected(r, call)[0]
    for toff_null, miss_null in ((True, False), (False, True), (True, True)):
        x = one_shot(r, call, cap, toff_null=toff_null, miss_null=miss_null, enc_null=True)
        assert x.rc == N.TM_OK
        check_filled(r, call, x, toff=not toff_null, miss=not miss_null)
        assert toff_null == bool((x.toff == MARK64).all()) and miss_null == bool((x.miss == MARK32).all())
        assert x.enc_used.value == MARK32


@pytest.mark.parametrize("name", VOCABS)
@pytest.mark.parametrize("call", ("spans", "raw_spans"))
def test_required_outputs_may_not_be_null(call, name):
    """tokens_out or spans_out NULL with ids to deliver: TM_E_INVALID - behind the offsets and the counts, which are filled as for TM_E_NOSPACE"""
    _, N, _ = _mods()
    r = ref(name)
    cap = expected(r, call)[0]
    for tok_null, sp_null in ((True, False), (False, True), (True, True)):
        x = one_shot(r, call, cap, tok_null=tok_null, sp_null=sp_null)
        assert x.rc == N.TM_E_INVALID
        check_filled(r, call, x, ids=False)
        check_lane_is_clean(r, call)
    # too small a capacity is answered first
    x = one_shot(r, call, cap - 1, tok_null=True, sp_null=True)
    assert x.rc == N.TM_E_NOSPACE
    check_lane_is_clean(r, call)
    # an empty batch has no ids to deliver
    x = one_shot(r, call, 0, ndocs=0, tok_null=True, sp_null=True)
    assert x.rc == N.TM_OK and int(x.toff[0]) == 0


# ---- decode: the host-buffer call and the resident one share the host's part --------------------------------------------------------------
class DecodeRef:
    def __init__(self):
        tm, N, synth = _mods()
        wide_a = "ａ".encode()          # FULLWIDTH LATIN SMALL LETTER A: a three-byte letter with case, which the device leaves to the host decoder
        toks = [bytes([c]) for c in b"abcdehlorw DCW.,"] + [wide_a, b" w", b"he", b"D h"]
        self.v = tm.Vocab(synth.build_vocab(toks, capcode=2, charset=1, with_unk=True))
        self.plain = ["Hello WORLD, C".encode(), b"a " + wide_a + b" Be", b"lo. "]
        docs = [synth.normalize(d, 2, 0) for d in self.plain]          # (capcode-2 text as the normalizer writes it)
        text, offs = tm.pack_documents(docs)
        self.nd = len(docs)
        self.b = new_batch(self.v, 4096, 8)
        N.check(N.lib.tm_batch_upload(self.b, N.ptr(text), N.ptr(offs), self.nd))
        N.check(N.lib.tm_batch_run(self.b, None))
        self.ids, self.toff, miss, total, _ = download(self.b, self.nd)
        self.ids, self.toff = self.ids.copy(), self.toff.copy()
        assert int(miss.sum()) == 0 and total >= 20


_dec = []


def dec_ref():
    if not _dec:
        _dec.append(DecodeRef())
    return _dec[0]


def decode_host_buffers(r, raw, cap):
    _, N, _ = _mods()
    out, ooff = Out(max(cap, 1), 1), np.full(r.nd + 1, MARK64, dtype=np.uint64)
    rc = N.lib.tm_decode_batch(r.v.handle, N.ptr(r.ids), N.ptr(r.toff), r.nd, raw, out.ptr, cap, N.ptr(ooff))
    return rc, out, ooff, int(N.lib.tm_decode_host_docs())


def decode_resident(r, raw, cap):
    _, N, _ = _mods()
    nbytes, hd = C.c_uint64(MARK64), C.c_uint32(MARK32)
    N.check(N.lib.tm_batch_decode(r.b, raw, None, C.byref(nbytes), C.byref(hd)))
    out, ooff = Out(max(cap, 1), 1), np.full(r.nd + 1, MARK64, dtype=np.uint64)
    rc = N.lib.tm_batch_decoded_download(r.b, out.ptr, cap, N.ptr(ooff))
    return rc, out, ooff, int(hd.value)


@pytest.mark.parametrize("raw", (0, 1))
def test_decode_both_ways(raw):
    _, N, _ = _mods()
    r = dec_ref()
    big = 4096
    rc, out, ooff, hd = decode_host_buffers(r, raw, big)
    assert rc == N.TM_OK and out.sentinels_intact()
    n = int(ooff[r.nd])
    assert int(ooff[0]) == 0 and (np.diff(ooff.astype(np.int64)) > 0).all()
    text = out.view(np.uint8)[:n].tobytes()
    if raw:
        assert n >= len(b"".join(r.plain)) and hd == 0          # (the tokens' bytes as the vocabulary holds them)
    else:
        assert text == b"".join(r.plain) and hd == 1
    for way in (decode_host_buffers, decode_resident):
        # room to spare, and exactly enough
        for cap in (big, n):
            rc2, out2, ooff2, hd2 = way(r, raw, cap)
            assert rc2 == N.TM_OK and out2.sentinels_intact()
            assert np.array_equal(ooff2, ooff) and out2.view(np.uint8)[:n].tobytes() == text and hd2 == hd
        # one byte short: the offsets say what is needed, nothing is written
        rc2, out2, ooff2, hd2 = way(r, raw, n - 1)
        assert rc2 == N.TM_E_NOSPACE and np.array_equal(ooff2, ooff) and out2.untouched() and hd2 == hd
        # ... and the next call is served as if nothing had happened
        rc2, out2, ooff2, _ = way(r, raw, n)
        assert rc2 == N.TM_OK and np.array_equal(ooff2, ooff) and out2.view(np.uint8)[:n].tobytes() == text

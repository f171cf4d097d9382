"""-m gpu: tm_batch_collate_denoise (tm_denoise.hip) at the C ABI, outputs in tm_host_alloc memory behind sentinels, against the rule of include/tokenmonster_hip.h as a plain
loop over one row's window: masked_range (test_gpu_masked.py) selects over the whole document, one loop emits the input and the target entries.  Every comparison is exact.
Ids from tm_batch_load_ids.  The torch case runs in a child process that imports torch first (this file as a script).  Twin: tests/test_denoise_emulated.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ != "__main__":          # (as a script this file is the torch child, and torch comes before the package there)
    from tokenmonster_amd import _native as N
    from fixed_shape import Collate, Out, spec, DT, KEEP_TAIL, NONE, PAD_LEFT
    from test_gpu_select import batch, load, sync          # noqa: F401  (the batch fixture; documents of chosen id counts)
    from test_gpu_masked import masked_range, philox       # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
ONE = 1 << 32
PAD, BOS, EOS, SENT = 60001, 60002, 60003, 62000          # (no document holds them: load() keeps ids below 60000; SENT +- 100 fits two bytes)
SPANS = [(1, 1), (3, 3), (1, 32)]
WAVE = {id_bytes: 64 * 16 // id_bytes for id_bytes in (2, 4, 8)}          # the ids of one wavefront's share of a trip; a trip is four of them
denoise = lambda seed, thr, span, step, n, T, id_bytes: N.Denoise(seed, thr, span[0], span[1], SENT, step, n, T, 65535 if id_bytes == 2 else -100)          # noqa: E731


def selected(docs, dn):
    """rules 1 - 3 over every document of the run -> one bool array per document"""
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    m = N.Masking(dn.seed, dn.start_thr, dn.span_min, dn.span_max, 0, 0, 0, 0, 1, 0)
    return [masked_range(d, int(off[i]), m)[1] for i, d in enumerate(docs)]


def rule(doc, sel, src, n, dn):
    """the window doc[src : src + n] -> (the input entries, the target entries, the span number of every id or -1), specials apart"""
    inp, tgt, num, k, prev = [], [], [], -1, False
    for i in range(src, src + n):
        s = bool(sel[i])
        k += s and not prev
        if s and k < dn.sentinel_n:
            if not prev:
                inp.append(SENT + k * dn.sentinel_step)
                tgt.append(SENT + k * dn.sentinel_step)
            tgt.append(int(doc[i]))
        else:
            inp.append(int(doc[i]))
        num.append(k if s else -1)
        prev = s
    return inp, tgt, num


def expect(docs, dn, L, id_bytes, bos, eos, flags, rows_of):
    """-> [ids [rows, L], targets [rows, T], mask, lengths, target lengths, bad], and the span numbers of every row's window"""
    dt, T, ign, sels = DT[id_bytes], dn.target_len, dn.label_ignore % (1 << (8 * id_bytes)), selected(docs, dn)
    hb, he, rows = [] if bos is None else [bos], [] if eos is None else [eos], len(rows_of)
    ids, tg, nums = np.full((rows, L), PAD, dtype=dt), np.full((rows, T), ign, dtype=dt), []
    mask, lens, tlens = np.zeros((rows, L), dtype=np.uint8), np.zeros(rows, dtype=np.uint32), np.zeros(rows, dtype=np.uint32)
    for r, d in enumerate(rows_of):
        if d >= len(docs):          # an index that is no document: padding only
            nums.append([])
            continue
        n = min(len(docs[d]), L - len(hb) - len(he))
        inp, tgt, num = rule(docs[d], sels[d], len(docs[d]) - n if flags & KEEP_TAIL else 0, n, dn)
        inp, tlens[r], tgt = hb + inp + he, len(tgt) + len(he), tgt[:T - len(he)] + he
        ids[r, :len(inp)], mask[r, :len(inp)], lens[r], tg[r, :len(tgt)] = inp, 1, len(inp), tgt
        nums.append(num)
    return [ids, tg, mask, lens, tlens, np.array([sum(d >= len(docs) for d in rows_of)])], nums


def run(b, docs, dn, L, id_bytes, bos, eos, flags, sel=None, shift=0, given=(True,) * 5):
    """one call against the rule -> what the rule expects.  sel: the list of document numbers (None: every document); given: which of the five optional outputs are passed"""
    rows_of, dt = list(range(len(docs))) if sel is None else list(sel), DT[id_bytes]
    rows = len(rows_of)
    exp = expect(docs, dn, L, id_bytes, bos, eos, flags, rows_of)[0]
    o, idx = [Out(rows * L, id_bytes, shift), Out(rows * dn.target_len, id_bytes, shift), Out(rows * L, 1, shift), Out(rows, 4), Out(rows, 4), Out(1, 4)], Out(rows, 4)
    idx.view(np.uint32)[:] = rows_of
    how = Collate(0, rows, L, id_bytes, PAD, spec(bos), spec(eos), flags)
    N.check(N.lib.tm_batch_collate_denoise(b, C.byref(how), C.byref(dn), None if sel is None else idx.ptr, None, o[0].ptr, *[x.ptr if use else None for x, use in zip(o[1:], given)]))
    sync(b)
    what = (L, id_bytes, bos, eos, flags, sel is not None, shift, given, (dn.start_thr, dn.span_min, dn.span_max, dn.sentinel_step, dn.sentinel_n, dn.target_len))
    for x, e, d, use in zip(o, exp, (dt, dt, np.uint8, np.uint32, np.uint32, np.uint32), (True,) + tuple(given)):
        assert (x.sentinels_intact() and (x.view(d) == np.asarray(e).reshape(-1)).all()) if use else x.untouched(), what
    return exp


@pytest.mark.parametrize("id_bytes,L", [(id_bytes, L) for id_bytes, t in WAVE.items() for L in (1, 2, t - 1, t, t + 1, 4 * t - 1, 4 * t, 4 * t + 1, 8 * t + 1)])
def test_denoise_every_rule(batch, id_bytes, L):
    """documents of 0, 1 and room - 1, room, room + 40 ids for every number of specials; the specials and flags against start_thr 0 / middle / 2^32, the spans, both sentinel
    steps and caps, the target lengths, with a list (reversed, a document twice, one bad index) and without, either alignment, every optional output left out in turn"""
    counts = sorted({0, 1} | {c for ns in (0, 1, 2) for c in (L - ns - 1, L - ns, L - ns + 40) if c >= 0}) + [0, 3]
    docs, nd = load(batch, counts, id_bytes), len(counts)
    sel, combos = list(range(nd))[::-1] + [2, nd + 3, 1], itertools.product(itertools.product((False, True), repeat=2), (0, KEEP_TAIL), (0, ONE // 6, ONE), SPANS)
    for k, ((has_bos, has_eos), flags, thr, span) in enumerate(combos):
        if L >= has_bos + has_eos:
            dn = denoise(1000 + k, thr, span, (1, -1)[k & 1], (2, 100)[(k // 2 + k // 9) & 1], (1, 7, L + 2)[(k + k // 3) % 3], id_bytes)
            run(batch, docs, dn, L, id_bytes, BOS if has_bos else None, EOS if has_eos else None, flags, sel if (k // 3 + k // 18) & 1 else None, (k // 6 + k) & 1,
                tuple((k + k // 6) % 6 != i for i in range(5)))


def test_seams_caps_cuts_and_seeds(batch):
    """int64 rows of two trips under KEEP_TAIL: on the REFERENCE a row has three spans and more, spans cross a wavefront's and a trip's seam, a row begins inside a span that opened in
    front of it, a row has more spans than sentinel_n, a target is cut and one is not; one seed selects the same places of a document through two layouts; a second seed differs"""
    counts, L, t = [5, 1100, 0, 700, 40], 600, WAVE[8]
    docs, dn = load(batch, counts, 8), denoise(4, ONE // 12, (1, 8), -1, 3, 10, 8)          # (the seed: chosen so that the asserts on the reference below hold)
    sels, (exp, nums) = selected(docs, dn), expect(docs, dn, L, 8, None, None, KEEP_TAIL, range(len(docs)))
    same = lambda num, i: num[i] >= 0 and num[i] == num[i + 1]          # noqa: E731  (ids i and i + 1 of the window stand in one span)
    assert any(same(num, s - 1) for num in nums for s in (t, 2 * t, 3 * t) if len(num) > s) and any(same(num, 4 * t - 1) for num in nums if len(num) > 4 * t)
    assert sels[1][1100 - L - 1] and sels[1][1100 - L] and nums[1][0] == 0          # the row begins inside a span
    assert max(nums[1]) >= 3 == dn.sentinel_n and exp[4][1] > dn.target_len >= exp[4][0] and (exp[1][0] == dn.label_ignore % (1 << 64)).any()
    run(batch, docs, dn, L, 8, None, None, KEEP_TAIL)
    # whole documents, no specials / behind BOS in reversed order: the same targets; another seed: other input rows
    free = denoise(4, ONE // 12, (1, 8), -1, 1000, 1200, 8)
    wide = run(batch, docs, free, 1200, 8, None, None, 0)
    back = run(batch, docs, free, 1210, 8, BOS, None, KEEP_TAIL, sel=list(range(len(docs)))[::-1])
    assert (wide[1] == back[1][::-1]).all() and (wide[4] == back[4][::-1]).all() and wide[4].max() > 100
    assert (wide[0] != run(batch, docs, denoise(5, ONE // 12, (1, 8), -1, 1000, 1200, 8), 1200, 8, None, None, 0)[0]).any()


def test_argument_errors_write_nothing(batch):
    load(batch, [3, 1, 2], 4)
    good = dict(seed=1, start_thr=ONE // 2, span_min=1, span_max=3, sentinel_first=SENT, sentinel_step=-1, sentinel_n=100, target_len=8, label_ignore=5)
    bad = [(4, dict(span_min=0)), (4, dict(span_min=4)), (4, dict(span_max=33)), (4, dict(start_thr=ONE + 1)), (4, dict(sentinel_step=0)), (4, dict(sentinel_n=0)),
           (4, dict(target_len=0)), (4, dict(sentinel_first=50)), (8, dict(sentinel_first=0xFFFFFFFF, sentinel_step=1, sentinel_n=2)), (2, dict(sentinel_first=65536)),
           (2, dict(sentinel_first=65500, sentinel_step=1)), (2, dict(label_ignore=-100)), (2, dict(label_ignore=65536))]
    o = [Out(3 * 8, 8) for _ in range(2)] + [Out(3 * 8, 1), Out(3, 4), Out(3, 4), Out(1, 4)]
    ptrs, idx = [x.ptr for x in o], Out(17, 4)
    for (id_bytes, change), ix in itertools.product(bad, (None, idx.ptr)):
        how = Collate(0, 3, 8, id_bytes, PAD, NONE, NONE, 0)
        assert N.lib.tm_batch_collate_denoise(batch, C.byref(how), C.byref(N.Denoise(**dict(good, **change))), ix, None, *ptrs) == N.TM_E_INVALID, change
    how, dn = Collate(0, 3, 8, 4, PAD, NONE, NONE, 0), N.Denoise(**good)
    assert N.lib.tm_batch_collate_denoise(batch, C.byref(how), None, None, None, *ptrs) == N.TM_E_INVALID and b"denoising" in N.lib.tm_last_error()
    assert N.lib.tm_batch_collate_denoise(batch, C.byref(how), C.byref(dn), None, None, None, *ptrs[1:]) == N.TM_E_INVALID          # no ids_out
    # left padding, with and without a list; first_doc 1 with a list (must be 0) and without (documents 1 .. 3 of a run of 3); a flag bit that is no flag
    for first, flags, ix in ((0, PAD_LEFT, None), (0, PAD_LEFT | KEEP_TAIL, idx.ptr), (1, 0, idx.ptr), (1, 0, None), (0, 4, None)):
        how.first_doc, how.flags = first, flags
        assert N.lib.tm_batch_collate_denoise(batch, C.byref(how), C.byref(dn), ix, None, *ptrs) == N.TM_E_INVALID, (first, flags)
    how = Collate(0, 17, 8, 4, PAD, NONE, NONE, 0)          # 17 rows of 2^32 - 1 target ids: beyond 2^36 elements
    assert N.lib.tm_batch_collate_denoise(batch, C.byref(how), C.byref(N.Denoise(**dict(good, target_len=ONE - 1))), idx.ptr, None, *ptrs) == N.TM_E_INVALID
    assert all(x.untouched() for x in o + [idx])


def child_main():
    import torch                                     # first: its HIP runtime is the one the library then shares
    if not torch.cuda.is_available():
        return print("SKIP torch has no device")
    sys.path[:0] = [HERE, os.path.dirname(HERE)]
    import tokenmonster_amd as tm
    from tokenmonster_amd import _native as N, synth, torch_api
    v = tm.Vocab(synth.build_vocab(sorted(bytes([c]) for c in b"abcdefgh"), capcode=0, charset=1, norm_flag=0, with_unk=True))
    docs = [b"abc", b"", b"defgh" * 9, b"abcdefgha", b"h", b"gfedcbagfedcbagfe" * 4]
    kw = dict(pad_id=60001, bos_id=60002, eos_id=60003, dtype=torch.int32)
    sc = torch_api.SpanCorruption(62000, noise_density=0.3, span=(1, 4))
    res = torch_api.tokenize_resident(v, docs)
    idx = torch.tensor([5, 2, 9, 0, 2], dtype=torch.int32, device="cuda")
    got, plain = res.collate(idx, 24, **kw, denoise=sc, target_length=48, seed=11), res.collate(idx, 24, **kw)
    exp = [torch.empty((5, 24), dtype=torch.int32, device="cuda"), torch.empty((5, 48), dtype=torch.int32, device="cuda"), torch.empty((5,), dtype=torch.int32, device="cuda")]
    how, dn = torch_api._Collate(0, 5, 24, 4, 60001, 60002, 60003, 0), N.Denoise(11, round(ONE * 0.3 / 2.5), 1, 4, 62000, -1, 100, 48, -100)
    N.check(N.lib.tm_batch_collate_denoise(res.handle, C.byref(how), C.byref(dn), idx.data_ptr(), None, exp[0].data_ptr(), exp[1].data_ptr(), None, None, exp[2].data_ptr(), None))
    torch.cuda.synchronize()
    assert all(torch.equal(got[k], e) for k, e in zip(("input_ids", "labels", "target_lengths"), exp)) and int(got["bad_indices"]) == 1
    assert got["labels"].shape == (5, 48) and not torch.equal(got["lengths"], plain["lengths"])
    # undone: the target's spans back behind their sentinels in the input give the plain row
    for row, tg, n, tn, want, wn in zip(*(x.tolist() for x in (got["input_ids"], got["labels"], got["lengths"], got["target_lengths"], plain["input_ids"], plain["lengths"]))):
        spans = {}
        for x in tg[:max(tn - 1, 0)]:                # (without the EOS)
            key = x if 62000 - 100 < x <= 62000 else key
            spans.setdefault(key, []).extend([] if x == key else [x])
        assert [y for x in row[:n] for y in spans.get(x, [x])] == want[:wn]
    enc = torch_api.encode_batch(v, docs, 24, **kw, denoise=sc, target_length=48, seed=11)          # the same documents tokenized again: the same places in the run
    again = res.collate(list(range(len(docs))), 24, **kw, denoise=sc, target_length=48, seed=11)
    assert all(torch.equal(enc[k], again[k]) for k in ("input_ids", "labels", "attention_mask", "lengths", "target_lengths")) and "bad_indices" not in enc
    res.close()
    print("OK")


def test_torch_denoise():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    if "SKIP" in out:
        pytest.skip(out.strip())
    assert r.returncode == 0 and out.strip().endswith("OK"), out[-4000:]


if __name__ == "__main__":
    child_main()

"""-m gpu: tm_batch_collate_masked (tm_masked.hip) at the C ABI, outputs in tm_host_alloc memory behind sentinels, against a numpy statement of
the rule in include/tokenmonster_hip.h: Philox4x32-10 in uint64 arithmetic (checked against the Random123 known answers), the span recurrence
as the plain loop over a document, the rows by np_collate.  Every comparison is exact.  Ids from tm_batch_load_ids.  The torch case runs in a
child process that imports torch first (this file as a script).  Twin: tests/test_masked_emulated.py."""
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
    from test_gpu_collate import np_collate
    from test_gpu_select import batch, load, sync          # noqa: F401  (the batch fixture; documents of chosen id counts)

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
U = np.uint64
M32, ONE = U(0xFFFFFFFF), 1 << 32
PAD, BOS, EOS, MASK, RLO, RN = 60001, 60002, 60003, 60004, 61000, 500          # (no document holds them: load() keeps ids below 60000)
SPANS = [(1, 1), (3, 3), (1, 32), (32, 32)]
SHARES = [(ONE, 0), (0, ONE), (ONE // 2, ONE // 4), (0, 0)]                    # (mask_thr, random_thr): all mask, all random, split, all kept
TILES = {id_bytes: 64 * 16 // id_bytes for id_bytes in (2, 4, 8)}              # the columns of one wavefront's tile
masking = lambda seed, thr, span, share, id_bytes: N.Masking(seed, thr, span[0], span[1], share[0], share[1], MASK, RLO, RN, 65535 if id_bytes == 2 else -100)          # noqa: E731


def philox(g, seed, c23=0):
    """Philox4x32-10 of the counters (g & 0xFFFFFFFF, g >> 32, c23, c23) under the 64-bit seed -> four uint64 arrays of 32-bit words"""
    g = np.asarray(g, dtype=U)
    c, k0, k1 = [g & M32, g >> U(32), g * U(0) + U(c23), g * U(0) + U(c23)], U(seed & 0xFFFFFFFF), U(seed >> 32)
    for i in range(10):
        if i:
            k0, k1 = (k0 + U(0x9E3779B9)) & M32, (k1 + U(0xBB67AE85)) & M32
        p0, p1 = U(0xD2511F53) * c[0], U(0xCD9E8D57) * c[2]
        c = [(p1 >> U(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> U(32)) ^ c[3] ^ k1, p0 & M32]
    return c


def masked_range(ids, g0, m):
    """rules 1-4 over the ids at places g0 .. g0 + len(ids) - 1 taken as ONE document -> (the ids afterwards, which are selected)"""
    w = philox(np.arange(g0, g0 + len(ids), dtype=U), m.seed)
    reach = np.where(w[0] < U(m.start_thr), U(m.span_min) + ((w[1] * U(m.span_max - m.span_min + 1)) >> U(32)), U(0)).astype(np.int64)
    sel, rem = np.zeros(len(ids), dtype=bool), 0
    for i in range(len(ids)):
        rem = max(int(reach[i]), rem - 1)
        sel[i] = rem >= 1
    ids = np.asarray(ids, dtype=U)
    new = np.where(w[2] < U(m.mask_thr), U(m.mask_id), np.where(w[2] < U(m.mask_thr + m.random_thr), U(m.random_lo) + ((w[3] * U(m.random_n)) >> U(32)), ids))
    return np.where(sel, new, ids).astype(np.uint32), sel


def test_philox_known_answers():
    assert [int(x[0]) for x in philox([0], 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(x[0]) for x in philox([2 ** 64 - 1], 2 ** 64 - 1, 0xFFFFFFFF)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def run(b, docs, m, L, id_bytes, bos, eos, flags, sel=None, shift=0, given=(True, True, True, True)):
    """one call against the rule -> (ids, labels) as [rows, L] arrays.  sel: the list of document numbers (None: no list, every document);
    given: which of labels_out, mask_out, lengths_out, bad_out are passed"""
    dt, ign = DT[id_bytes], m.label_ignore % (1 << (8 * id_bytes))
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    done = [masked_range(d, int(off[i]), m) for i, d in enumerate(docs)]
    labdocs = [[int(t) if s else ign for t, s in zip(d, done[i][1])] for i, d in enumerate(docs)]
    rows_of = list(range(len(docs))) if sel is None else list(sel)
    isbad = np.array([i >= len(docs) for i in rows_of], dtype=bool)
    e = list(np_collate([done[i][0] if i < len(docs) else [] for i in rows_of], L, PAD, bos, eos, flags, dt))
    lab = np_collate([labdocs[i] if i < len(docs) else [] for i in rows_of], L, ign, None if bos is None else ign, None if eos is None else ign, flags, dt)[0]
    e[0][isbad], e[1][isbad], e[2][isbad], lab[isbad] = PAD, 0, 0, ign          # an index that is no document: padding only
    rows = len(rows_of)
    o, idx = [Out(rows * L, id_bytes, shift), Out(rows * L, id_bytes, shift), Out(rows * L, 1, shift), Out(rows, 4), Out(1, 4)], Out(rows, 4)
    idx.view(np.uint32)[:] = rows_of
    how = Collate(0, rows, L, id_bytes, PAD, spec(bos), spec(eos), flags)
    N.check(N.lib.tm_batch_collate_masked(b, C.byref(how), C.byref(m), None if sel is None else idx.ptr, None, o[0].ptr, *[x.ptr if use else None for x, use in zip(o[1:], given)]))
    sync(b)
    what = (L, id_bytes, bos, eos, flags, sel is not None, shift, given, (m.start_thr, m.span_min, m.span_max, m.mask_thr, m.random_thr))
    for x, exp, d, use in zip(o, [e[0], lab, e[1], e[2], np.array([isbad.sum()])], (dt, dt, np.uint8, np.uint32, np.uint32), (True,) + tuple(given)):
        assert (x.sentinels_intact() and (x.view(d) == np.asarray(exp).reshape(-1)).all()) if use else x.untouched(), what
    return o[0].view(dt).reshape(rows, L).copy(), o[1].view(dt).reshape(rows, L).copy()


@pytest.mark.parametrize("id_bytes,L", [(id_bytes, L) for id_bytes, t in TILES.items() for L in (1, 2, t - 1, t, t + 1, 4 * t - 1, 4 * t, 4 * t + 1)])
def test_masked_every_rule(batch, id_bytes, L):
    """documents of 0, 1 and room - 1, room, room + 40 ids for every number of specials; every specials combination and flag set against
    start_thr 0 / middle / 2^32, the spans, the shares, with a list (reversed, documents twice, one bad index) and without, either
    alignment, every optional output left out in turn"""
    counts = sorted({0, 1} | {c for ns in (0, 1, 2) for c in (L - ns - 1, L - ns, L - ns + 40) if c >= 0}) + [0, 3]
    docs, nd = load(batch, counts, id_bytes), len(counts)
    sel = list(range(nd))[::-1] + [2, nd + 3, 1]
    combos = itertools.product(itertools.product((False, True), repeat=2), (0, PAD_LEFT, KEEP_TAIL, PAD_LEFT | KEEP_TAIL), (0, ONE // 6, ONE))
    for k, ((has_bos, has_eos), flags, thr) in enumerate(combos):
        if L >= has_bos + has_eos:
            m = masking(1000 + k, thr, SPANS[k % 4], SHARES[(k // 3 + k // 12) % 4], id_bytes)
            run(batch, docs, m, L, id_bytes, BOS if has_bos else None, EOS if has_eos else None, flags, sel if (k // 2) & 1 else None, k & 1, tuple(k % 5 != i for i in range(4)))


def test_spans_documents_cuts_and_seeds(batch):
    """spans of 1 .. 32 at a middle start_thr over short and long documents: on the REFERENCE some but not all ids are selected, a span is cut
    by a document's start and a span enters a row from ids the row cut off; two seeds differ; one seed selects the same ids of a document
    through two layouts"""
    counts, L, ign = [5, 300, 0, 7, 7, 150, 2, 90], 64, 2 ** 32 - 100
    docs, off = load(batch, counts, 4), np.concatenate([[0], np.cumsum(counts)])
    m = masking(7, ONE // 20, (1, 32), SHARES[0], 4)
    per_doc = np.concatenate([masked_range(d, int(off[i]), m)[1] for i, d in enumerate(docs)])
    one_run = masked_range(np.concatenate(docs), 0, m)[1]                          # ... as if no document began anywhere
    assert per_doc.any() and not per_doc.all()
    assert any(one_run[off[i]] and not per_doc[off[i]] for i in range(1, len(docs)) if counts[i])
    tails = [masked_range(d[-L:], int(off[i + 1]) - min(L, len(d)), m)[1] for i, d in enumerate(docs)]      # ... as if a document began where its row does
    assert any((t != per_doc[off[i + 1] - len(t):off[i + 1]]).any() for i, t in enumerate(tails))
    ids = run(batch, docs, m, L, 4, None, None, KEEP_TAIL)[0]
    assert (ids != run(batch, docs, masking(8, ONE // 20, (1, 32), SHARES[0], 4), L, 4, None, None, KEEP_TAIL)[0]).any()
    # whole documents, right-padded without specials / left-padded behind BOS in reversed order: the same places of every document are selected
    wide = run(batch, docs, m, 320, 4, None, None, 0)[1]
    back = run(batch, docs, m, 333, 4, BOS, None, PAD_LEFT, sel=list(range(len(docs)))[::-1])[1][::-1]
    for i, n in enumerate(counts):
        assert ((wide[i, :n] != ign) == (back[i, 333 - n:] != ign)).all() and ((wide[i, :n] != ign) == per_doc[off[i]:off[i + 1]]).all()


def test_argument_errors_write_nothing(batch):
    load(batch, [3, 1, 2], 4)
    good = dict(seed=1, start_thr=ONE // 2, span_min=1, span_max=3, mask_thr=ONE // 2, random_thr=ONE // 2, mask_id=MASK, random_lo=RLO, random_n=RN, label_ignore=5)
    bad = [(4, dict(span_min=0)), (4, dict(span_min=4)), (4, dict(span_max=33)), (4, dict(start_thr=ONE + 1)), (4, dict(mask_thr=ONE + 1)), (4, dict(random_thr=ONE // 2 + 1)),
           (4, dict(random_n=0)), (8, dict(random_lo=0xFFFFFFFF, random_n=2)), (2, dict(mask_id=65536)), (2, dict(random_lo=65536 - RN + 1)), (2, dict(label_ignore=-100)),
           (2, dict(label_ignore=65536))]
    o = [Out(3 * 8, 8) for _ in range(2)] + [Out(3 * 8, 1), Out(3, 4), Out(1, 4)]
    ptrs = [x.ptr for x in o]
    for (id_bytes, change), idx in itertools.product(bad, (None, o[3].ptr)):
        how = Collate(0, 3, 8, id_bytes, PAD, NONE, NONE, 0)
        assert N.lib.tm_batch_collate_masked(batch, C.byref(how), C.byref(N.Masking(**dict(good, **change))), idx, None, *ptrs) == N.TM_E_INVALID, change
    how, m = Collate(0, 3, 8, 4, PAD, NONE, NONE, 0), N.Masking(**good)
    assert N.lib.tm_batch_collate_masked(batch, C.byref(how), None, None, None, *ptrs) == N.TM_E_INVALID and b"masking" in N.lib.tm_last_error()
    assert N.lib.tm_batch_collate_masked(batch, C.byref(how), C.byref(m), None, None, None, *ptrs[1:]) == N.TM_E_INVALID          # no ids_out
    # first_doc 1 with a list (must be 0) and without (documents 1 .. 3 of a run of 3); a flag bit that is no flag
    for first, flags, idx in ((1, 0, o[3].ptr), (1, 0, None), (0, 4, None)):
        how.first_doc, how.flags = first, flags
        assert N.lib.tm_batch_collate_masked(batch, C.byref(how), C.byref(m), idx, None, *ptrs) == N.TM_E_INVALID, (first, flags)
    assert all(x.untouched() for x in o)


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
    mk = torch_api.Masking(mask_id=60004, probability=0.3, span=(1, 4), random_ids=(61000, 9))
    res = torch_api.tokenize_resident(v, docs)
    idx = torch.tensor([5, 2, 9, 0, 2], dtype=torch.int32, device="cuda")
    got, plain = res.collate(idx, 24, **kw, masking=mk, seed=11), res.collate(idx, 24, **kw)
    exp = [torch.empty((5, 24), dtype=torch.int32, device="cuda") for _ in range(2)]
    how, m = torch_api._Collate(0, 5, 24, 4, 60001, 60002, 60003, 0), N.Masking(11, round(ONE * 0.3 / 2.5), 1, 4, round(ONE * 0.8), round(ONE * 0.1), 60004, 61000, 9, -100)
    N.check(N.lib.tm_batch_collate_masked(res.handle, C.byref(how), C.byref(m), idx.data_ptr(), None, exp[0].data_ptr(), exp[1].data_ptr(), None, None, None))
    torch.cuda.synchronize()
    assert torch.equal(got["input_ids"], exp[0]) and torch.equal(got["labels"], exp[1]) and int(got["bad_indices"]) == 1
    sel = got["labels"] != -100
    assert sel.any() and not sel.all() and torch.equal(torch.where(sel, got["labels"], got["input_ids"]), plain["input_ids"]) and "labels" not in plain
    enc = torch_api.encode_batch(v, docs, 24, **kw, masking=mk, seed=11)          # the same documents tokenized again: the same places in the run
    again = res.collate(list(range(len(docs))), 24, **kw, masking=mk, seed=11)
    assert all(torch.equal(enc[k], again[k]) for k in ("input_ids", "labels", "attention_mask", "lengths"))
    res.close()
    print("OK")


def test_torch_masking():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    if "SKIP" in out:
        pytest.skip(out.strip())
    assert r.returncode == 0 and out.strip().endswith("OK"), out[-4000:]


if __name__ == "__main__":
    child_main()

"""-m gpu: region labels - tm_batch_region_labels, tm_batch_collate_region_labels (tokenmonster_amd/csrc/tm_regions.hip), Vocab.tokenize_region_labels_packed,
torch_api.encode_batch(regions=...).  Expected: the header's rule as brute force in numpy (reference) over the pairs tm_batch_spans_in returns for the same
batch, text and unit; for normalized bytes those pairs are first held against the oracle's walk.  One batch: three documents of 256 ids with 127 / 128 /
129 one-unit regions (a tile each: both sides of the LDS window), one of 256 (its own tile: LDS path) and one of 255 ids (its tile ends in the next document:
global path) with regions on and beside token edges, documents of 256 (no region), 257 (one), 513 (one per token) and 600 ids (one over all of it), empty and
tiny ones in shared tiles.  On the emulated device (TM_EMU=1) run it with -k "not torch": the torch case needs a real device and fails without one."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest
from fixed_shape import Collate, Out, spec, KEEP_TAIL, PAD_LEFT

pytestmark = pytest.mark.gpu
FORMS = {"normalized_bytes": (0, 0), "raw_chars": (1, 1), "raw_utf16": (1, 2)}      # (TM_TEXT_*, TM_UNIT_*)
SIZES = [256, 256, 256, 256, 255, 256, 257, 513, 600]


def mods():
    import tokenmonster_amd as tm
    from tokenmonster_amd import _native as N, synth
    return tm, N, synth


def fuzz_str(rng, n):
    """text over the micro vocabulary's alphabet with capitals (capcode markers, forward deletes) and two-, three- and four-byte characters"""
    t = list(conftest.fuzz_text(rng, 0, n).replace(b"\xff", b"Q").replace(b"\x00", b"'").decode())
    for i in range(3, len(t), 7):
        t[i] = str(rng.choice(["é", "한", "😀", "H", "IT", t[i].upper()]))
    return "".join(t)


def trimmed(count, s, target):
    """a piece of s that count() gives exactly `target` ids: the shortest prefix with that many or more, of s without its first k characters"""
    for k in range(64):
        lo, hi = 0, len(s) - k
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (mid + 1, hi) if count(s[k:k + mid]) < target else (lo, mid)
        if count(s[k:k + lo]) == target:
            return s[k:k + lo]
    raise AssertionError("no piece of %d ids" % target)


def edge_regions(sp, length):
    """sorted, disjoint regions: ending / beginning at a forward-delete id's place, on and one unit beside token edges, splitting a token, empty, beyond the end"""
    out = []
    def add(x, y):
        if (out[-1][1] if out else 0) <= x <= y:
            out.append((x, y))
    for i, (b, e) in enumerate(sp.tolist()):
        m = (b + e) // 2
        if e == b:
            add(max(out[-1][1] if out else 0, b - 2), b)
            add(b, b + 2)
        elif i % 4 == 0:
            for x, y in [[(b, e)], [(b + 1, e)], [(b - 1, b)], [(b, e - 1)], [(e, e + 1)], [(b, m), (m, e)], [(b, b)]][(i // 4) % 7]:
                add(x, y)
    add(max(out[-1][1], length - 1), length + 50)
    return out


def reference(sp, toff, regs, roff, lens, ignore):
    """the header's rule, a loop over every region of every document"""
    labels, rtok = np.full(sp.shape[0], ignore, np.int64), np.zeros((regs.shape[0], 2), np.int64)
    for d in range(len(lens)):
        t0, t1 = int(toff[d]), int(toff[d + 1])
        b, e, free = sp[t0:t1, 0], sp[t0:t1, 1], np.ones(t1 - t0, bool)
        for r in range(int(roff[d]), int(roff[d + 1])):
            rb, re = min(int(regs[r, 0]), lens[d]), min(int(regs[r, 1]), lens[d])
            hit = (b < re) & np.where(e > b, rb < e, rb <= b) & (rb < re)
            if hit.any():
                idx = np.nonzero(hit)[0]
                rtok[r] = (idx[0], idx[-1] + 1)
                labels[t0:t1][hit & free] = regs[r, 2]
                free &= ~hit
    return labels, rtok


class Scene:
    def __init__(self):
        from oracle_bind import Oracle
        tm, N, synth = mods()
        rng = np.random.default_rng(20261)
        toks = set(conftest.fuzz_vocab_tokens(rng, 2, 220)) | {bytes([c]) for c in b"abcdefghilnorstw .,1290'\nQ"}
        toks |= {b"D", b"C", b"W", b" h", b" a", b"D a", b"DW", b"W h", b"i", "é".encode(), "́".encode(), "한".encode()}
        self.v = tm.Vocab(synth.build_vocab(sorted(toks), capcode=2, charset=1, norm_flag=1, with_unk=True))
        self.orc = Oracle(self.v.image())
        self.norm = lambda s: synth.normalize(s.encode(), 2, 1)
        self.strs = [trimmed(lambda s: self.orc.tokenize(self.norm(s))[0].size, fuzz_str(rng, 6 * n), n) for n in SIZES] + ["", "a", ".", "", "", " ab.", "Hi", "é"] * 8
        self.docs = [s.encode() for s in self.strs]
        raw, offs = tm.pack_documents(self.docs)
        self.b = C.c_void_p()
        N.check(N.lib.tm_batch_create(self.v.handle, 4 * raw.size + 8192, len(self.docs), C.byref(self.b)))
        N.check(N.lib.tm_batch_upload_raw(self.b, N.ptr(raw), N.ptr(offs), len(self.docs)))
        N.check(N.lib.tm_batch_normalize(self.b, None))
        N.check(N.lib.tm_batch_run(self.b, None))
        self.memo, self.hd = {}, {}                  # (hd: documents the span call mapped on the host, per kind of text)

    def state(self, text=1, unit=1):
        """-> (ids, tok_offsets, pairs int64 [total, 2]) of the batch"""
        _, N, _ = mods()
        n = C.c_uint64()
        N.check(N.lib.tm_batch_totals(self.b, C.byref(n), None))
        ids, toff = np.zeros(n.value, np.uint32), np.zeros(len(self.docs) + 1, np.uint64)
        N.check(N.lib.tm_batch_download(self.b, N.ptr(ids), n.value, N.ptr(toff), None))
        sp = Out(2 * n.value, 4)
        hd = C.c_uint32(7)
        N.check(N.lib.tm_batch_spans_in(self.b, None, text, unit, sp.ptr, n.value, C.byref(hd), None))
        N.check(N.lib.tm_batch_totals(self.b, None, None))
        self.hd[text] = hd.value
        return ids, toff.astype(np.int64), sp.view(np.uint32).reshape(-1, 2).astype(np.int64)

    def form(self, name):
        """-> (tok_offsets, pairs, regions int64 [nreg, 3], reg_offsets, documents' lengths) in this text and unit"""
        if name not in self.memo:
            text, unit = FORMS[name]
            ids, toff, sp = self.state(text, unit)
            assert [int(x) for x in np.diff(toff)[:len(SIZES)]] == SIZES and (sp[:, 0] == sp[:, 1]).sum() > 5
            lens = [len(self.norm(s)) if text == 0 else len(s) if unit == 1 else len(s.encode("utf-16-le")) // 2 for s in self.strs]
            per = []
            for d in range(len(self.docs)):
                dsp = sp[toff[d]:toff[d + 1]]
                ones = [(int(x), int(x) + 1) for x in np.unique(dsp[dsp[:, 1] > dsp[:, 0], 0])]
                edge = edge_regions(dsp, lens[d]) if d in (3, 4) else []
                per.append({0: ones[:127], 1: ones[:128], 2: ones[:129], 3: edge, 4: edge, 5: [], 6: [(lens[d] // 2, lens[d] // 2 + 9)], 7: ones,
                            8: [(0, lens[d])]}.get(d, [(0, 5)] if d % 3 else []))
            assert [len(p) for p in per[:3]] == [127, 128, 129] and 40 < len(per[3]) <= 128 and len(per[7]) > 270      # (7: more than 128 in each of its tiles)
            roff = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.uint64)
            regs = np.array([r + ((k * 7) % 23 - 9,) for p in per for k, r in enumerate(p)], np.int64)
            for a in (toff, sp, regs, roff):
                a.setflags(write=False)
            self.memo[name] = (toff, sp, regs, roff, lens)
        return self.memo[name]

    def labels(self, name, regs, roff, ignore, nbytes, shift=0, how=None):
        """tm_batch_region_labels, or with `how` tm_batch_collate_region_labels, into page-locked memory behind sentinels -> (labels, token ranges, bad)"""
        _, N, _ = mods()
        pin = [Out(roff.size, 8), Out(max(regs.size, 1), 4)]
        pin[0].view(np.uint64)[:] = roff
        pin[1].view(np.uint32)[:regs.size] = regs.astype(np.uint32).reshape(-1)
        rg = N.Regions(pin[0].ptr, pin[1].ptr, FORMS[name][0], FORMS[name][1], ignore)
        total, hd = int(self.form(name)[0][-1]), C.c_uint32(9)
        out, rt, bad = Out(how.ndocs * how.row_len if how else total, nbytes, shift), Out(2 * regs.shape[0], 4), Out(1, 4)
        if how:
            N.check(N.lib.tm_batch_collate_region_labels(self.b, C.byref(how), None, C.byref(rg), out.ptr, nbytes, bad.ptr))
        else:
            N.check(N.lib.tm_batch_region_labels(self.b, None, C.byref(rg), out.ptr, nbytes, total, rt.ptr, bad.ptr, C.byref(hd)))
        N.check(N.lib.tm_batch_totals(self.b, None, None))                  # (waits for the NULL stream)
        assert (how or hd.value == self.hd[FORMS[name][0]]) and out.sentinels_intact() and rt.sentinels_intact() and bad.sentinels_intact()
        return out.view({4: np.int32, 8: np.int64}[nbytes]).astype(np.int64), rt.view(np.uint32).reshape(-1, 2).astype(np.int64), int(bad.view(np.uint32)[0])


scene = functools.lru_cache(None)(Scene)


@pytest.mark.parametrize("name", list(FORMS))
def test_ragged_labels_and_token_ranges(name):
    s = scene()
    toff, sp, regs, roff, lens = s.form(name)
    if name == "normalized_bytes":                  # this form rests on nothing of the library's: the pairs are the oracle's
        from span_recipe import oracle_spans
        assert (sp == np.concatenate([oracle_spans(s.orc, s.norm(t), True) for t in s.strs if t])).all()
    for ignore, nbytes, shift in ((-100, 4, 0), (-1, 8, 0), (0, 4, 1), (0xFFFFFF, 8, 1)):
        got, rtok, bad = s.labels(name, regs, roff, ignore, nbytes, shift)
        exp, exp_rtok = reference(sp, toff, regs, roff, lens, ignore)
        assert bad == 0 and (exp < 0).any() and (exp_rtok[:, 1] - exp_rtok[:, 0] > 1).any() and (exp_rtok.sum(axis=1) == 0).any()
        assert (got == exp).all(), (name, ignore, nbytes, np.nonzero(got != exp)[0][:8], toff[:10])
        assert (rtok == exp_rtok).all(), (name, np.nonzero((rtok != exp_rtok).any(axis=1))[0][:8], roff[:10])


@pytest.mark.parametrize("L,bos,eos,flags,nbytes,ignore", [(256, None, None, 0, 4, -100), (257, 1, 2, PAD_LEFT, 8, -1), (255, 1, None, KEEP_TAIL, 8, 0xFFFFFF),
                                                           (258, None, 2, PAD_LEFT | KEEP_TAIL, 4, 0)])
def test_collated_labels_are_a_gather_of_the_ragged_ones(L, bos, eos, flags, nbytes, ignore):
    s = scene()
    toff, sp, regs, roff, lens = s.form("raw_chars")
    ragged = reference(sp, toff, regs, roff, lens, ignore)[0]
    first, nd = 4, 6                                # the documents of 255, 256, 257, 513 and 600 ids and an empty one
    got, _, bad = s.labels("raw_chars", regs, roff, ignore, nbytes, 1, Collate(first, nd, L, 4, 0, spec(bos), spec(eos), flags))
    exp = np.full((nd, L), ignore, np.int64)
    for r in range(nd):
        lab = ragged[toff[first + r]:toff[first + r + 1]]
        m = min(lab.size, L - (bos is not None) - (eos is not None))
        row = [ignore] * (bos is not None) + (lab[lab.size - m:] if flags & KEEP_TAIL else lab[:m]).tolist() + [ignore] * (eos is not None)
        lo = L - len(row) if flags & PAD_LEFT else 0
        exp[r, lo:lo + len(row)] = row
    assert bad == 0 and (got.reshape(nd, L) == exp).all()


def test_errors_and_regions_out_of_order():
    tm, N, _ = mods()
    s = scene()
    toff, sp, regs, roff, lens = s.form("raw_chars")
    before = s.state()
    total, out, pin = int(toff[-1]), Out(int(toff[-1]), 4), Out(roff.size + 2 * regs.size, 8)
    pin.view(np.uint64)[:roff.size] = roff
    rg = lambda text, unit: C.byref(N.Regions(pin.ptr, pin.ptr + 8 * roff.size, text, unit, -100))
    for text, unit, nbytes in ((2, 0, 4), (0, 3, 4), (1, 1, 2), (1, 1, 16)):
        assert N.lib.tm_batch_region_labels(s.b, None, rg(text, unit), out.ptr, nbytes, total, None, None, None) == N.TM_E_INVALID
        assert N.lib.tm_batch_collate_region_labels(s.b, C.byref(Collate(0, 2, 8, 4, 0, spec(None), spec(None), 0)), None, rg(text, unit), out.ptr, nbytes, None) == N.TM_E_INVALID
    assert N.lib.tm_batch_region_labels(s.b, None, rg(1, 1), out.ptr, 4, total - 1, None, None, None) == N.TM_E_NOSPACE
    fresh = C.c_void_p()
    N.check(N.lib.tm_batch_create(s.v.handle, 4096, 4, C.byref(fresh)))
    try:
        assert N.lib.tm_batch_region_labels(fresh, None, rg(0, 0), out.ptr, 4, total, None, None, None) == N.TM_E_INVALID      # no walked ids
        text, offs = tm.pack_documents([s.norm("ab a")])
        N.check(N.lib.tm_batch_upload(fresh, N.ptr(text), N.ptr(offs), 1))
        N.check(N.lib.tm_batch_run(fresh, None))
        assert N.lib.tm_batch_region_labels(fresh, None, rg(1, 0), out.ptr, 4, total, None, None, None) == N.TM_E_INVALID        # no raw text
    finally:
        N.lib.tm_batch_free(fresh)
    assert out.untouched()
    wrong = regs.copy()
    wrong[[0, 1]] = wrong[[1, 0]]                   # a swapped pair in document 0
    k = int(roff[1])
    wrong[k + 1, 0] = wrong[k, 1] - 1               # an overlap in document 1 (one-unit regions: it begins inside the one before)
    assert s.labels("raw_chars", wrong, roff, -100, 4)[2] == 2
    assert all((x == y).all() for x, y in zip(before, s.state()))


def torch_child():                                  # encode_batch(regions=...), in a child process that imports torch first
    import torch
    torch.cuda.init()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tokenmonster_amd import torch_api
    tm, _, _ = mods()
    s = Scene()
    strs = s.strs[3:12]
    raw, offs = tm.pack_documents([t.encode() for t in strs])
    regs = np.array([(2, 9, -7), (9, 12, 3), (40, 41, 5)] * len(strs), np.int64)
    roff = np.arange(len(strs) + 1, dtype=np.uint64) * 3
    ids, toff, ragged, rtok = s.v.tokenize_region_labels_packed(raw, offs, regs, roff, unit="chars", ignore_label=-1)
    n = s.v.n_ids()
    kw = dict(pad_id=n + 1, bos_id=n + 2, pad_left=True)
    plain = torch_api.encode_batch(s.v, strs, 40, **kw)
    exp = np.full((len(strs), 40), -1, np.int64)
    for d in range(len(strs)):
        lab = ragged[int(toff[d]):int(toff[d + 1])][:39]
        exp[d, 40 - lab.size:] = lab
    assert (exp == -7).any() and (rtok[::3, 1] > rtok[::3, 0]).any()         # (the empty documents' regions meet no id)
    for dtype in (torch.int64, torch.int32):
        out = torch_api.encode_batch(s.v, strs, 40, dtype=dtype, regions=(regs, torch.as_tensor(roff.astype(np.int64))), ignore_label=-1, offset_unit="chars", **kw)
        assert out["labels"].is_cuda and out["labels"].dtype == dtype and (out["labels"].cpu().numpy() == exp).all()
        assert torch.equal(out["input_ids"].to(torch.int64), plain["input_ids"])
    again = torch_api.encode_batch(s.v, strs, 40, regions=None, **kw)           # regions=None: exactly what the call returned before
    assert sorted(again) == sorted(plain) == ["attention_mask", "input_ids", "lengths"] and all(torch.equal(again[k], plain[k]) for k in plain)


def test_torch_encode_batch_with_regions_and_without():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]


if __name__ == "__main__":
    torch_child()

"""Every construct of tests/match_cases.py at every byte offset across every seam of the match kernel (tm_kernels.hip: k_match_branch - K1 -, with
k_resolve and the group kernels - K3 - and k_emit_list / k_score_list - K4 - behind it), for five vocabulary forms (capcode 0, capcode 2, capcode 2
without an unk token, capcode 2 with more than 65 536 ids - the R0_WIDE planes, k_emit_list<true> -, and UTF-16), bit-exact against the oracle
(oracle/tm_oracle.c; pinned to the reference runtime on these very constructs by tests/test_match_boundaries_emulated.py).  No tolerances.

The seams, as the constants they are - if the kernel's move, test_the_kernel_still_has_these_seams fails and the sweep does not go blind:

  segment      256 bytes.  Filler of every length o from 256 - len - 1 to 257 in front of the construct: it ends in front of the seam, lies across it at
               every byte, begins behind it.  Two fillers (a one-byte token repeated: the construct begins on a token boundary; fuzz_text), five
               tails (nothing, a forward-delete trigger chosen by the oracle, a one-byte token, a space, 60 bytes of fuzz_text).
  workgroup    four wavefronts, a segment each: wavefronts 0-2 copy D[0..40) and Db[0..40) from their neighbour, wavefront 3 walks all 296
               positions itself.  Every document of the segment sweep stands FOUR times in its batch, its first segment at a global segment index
               of 0, 1, 2 and 3 modulo 4 (one-segment documents of one byte are put in front of it until it does): the seam at 256 falls between
               wavefronts 0|1, 1|2, 2|3 and 3|0.
  document end the document ends with c[:k] for every k, at a total length of 256 j + e, j in 0, 1, 2: e over END_E, and every e in 0 ... 96 for
               the longest chain and the deepest all-accepting path.  (tail_here; the TAIL form of the loop; a sharing wavefront's halo that sees the
               end.)  For e in 39, 40, 41 - dl of the segment in front of the end is NPOS - 1, NPOS, NPOS + 1 - every document stands at all four segment
               indices modulo 4; else the first segment of document (k, e, j) stands at segment index (k + e's index + j) modulo 4.
  long         one document of more than 513 segments with a construct at EVERY segment boundary; construct and straddle (-1 ... 41 bytes in front
               of the boundary) cycle with coprime periods, so every pair falls on some boundary; the boundaries 16 k, 64 k and 512 carry the
               longest chain at straddles 1, 20 and 39.  Plainly and under the hooks 4096, 32768, 1024, 64, 32 and their pairs (K3's groups and fan-out
               4, K4's id-staging form and direct stores, the dense forward-delete array, the wide exit map).
  slab         raw text through the one-pass path (Vocab.tokenize; hook 2048: packed): k growth characters at the head (capitals, or e-acute under
               NFD) put the end of the first 1 KiB piece at r = len(normalize(raw[:1024])) % 256 for every r of SLAB_R; every (construct, straddle
               -1 ... 41 of the PIECE end) pair stands once, r and the growth kind rotating (pair number n: SLAB_R[n % 15], kind (n // 15) % 2), and a
               40-byte chain and a pair of 40-byte tokens, all letters, at every straddle for every r and both kinds.  (Of the constructs the
               normalizer leaves as they are: slab_rows.)
  exit maps    six constructs across a range cut at every byte: all 80 entries of the device's map against the oracle's range walk.

No case is left out of the sweep.  On the emulated device (tests/test_match_boundaries_emulated.py) it is cut by this fixed rule: the segment sweep
with the workgroup positions 0 and 3, every third filler length plus the three at which the construct begins at 255, 256 and 257 and the three at
which it ends there, the token filler only; the document end with j in 0, 1, END_E only and every third k plus the last; the slab sweep with the
40-byte chain only, r in 0, 3, 95, 253; the exit maps at every third cut; the long document cut to 40 segments under hook 4096; the forms capcode 2
and UTF-16 for the segment sweep and the document end, capcode 2 for the others; the ring on the first 300 documents.  That is more than a cut of
seams, workgroup positions, offsets and tails alone: the emulated device runs about 50 KB/s through tokenize, count and score, the constructs here
(runs of 120 and 160 bytes among them) make such a cut alone 11 MB over the five forms, and the child is to stay near 2 MB and two minutes of the CPU suite."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import match_cases as M
import tokenmonster_amd as tm
from conftest import EMULATED
from oracle_bind import Oracle, oracle_stats
from span_recipe import oracle_spans
from tokenmonster_amd import _native as N
from tokenmonster_amd import dist as tmdist
from tokenmonster_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = M.SEG
PAD = M.FILL      # a one-segment document of one byte
FORMS = ["capcode2", "utf16"] if EMULATED else M.FORMS
LEADS = (0, 3) if EMULATED else (0, 1, 2, 3)
FILLERS = ("token",) if EMULATED else ("token", "fuzz")
END_J = (0, 1) if EMULATED else (0, 1, 2)
SLAB_R = [0, 1, 2, 3, 4, 5, 93, 94, 95, 96, 97, 252, 253, 254, 255]
SLAB_R_RUN = [0, 3, 95, 253] if EMULATED else SLAB_R
HOOKS = [4096] if EMULATED else [0, 64, 1024, 1024 | 64, 4096, 4096 | 64, 32768, 32768 | 1024, 32768 | 64, 32]
STATS_PLAIN = ["s1", "s2", "s3", "fast_exit", "no_lookahead_match", "not_found"]
STATS_ALL = ["s1", "s2", "s3", "s1b", "s2b", "s3b", "fast_exit", "no_lookahead_match", "not_found"]

_made = {}


@pytest.fixture(scope="module", autouse=True)
def release_what_was_made():
    """vocabularies are made once per form and shared by this module's tests - and given back when the last of them has run"""
    yield
    for k, x in list(_made.items()):
        if k[0] == "form":
            x.v.close()
    _made.clear()


def kernel_constants():
    src = open(os.path.join(ROOT, "tokenmonster_amd", "csrc", "tm_kernels.hip"), encoding="utf-8").read()
    pipe = open(os.path.join(ROOT, "tokenmonster_amd", "csrc", "tm_pipeline.h"), encoding="utf-8").read()
    assert "constexpr int TAIL_TASK0 = 64, TAIL_TASKS = (NPOS - TAIL_TASK0) / 3" in src and "#define TM_K1_DEFER_DEPTH 12" in src, "the task list or DEFER have moved"
    assert "constexpr int SIDE_STRIDE = 16;" in pipe, "the side list has another size"
    assert "const bool share = wvi + 1 < WAVES && (rw & SP_SAME_DOC) != 0u;" in src and "const bool tail_here = !share && dl <= NPOS;" in src, "share / tail_here have moved"
    assert "if (dl >= NPOS + Lmax) rounds(std::false_type{}); else rounds(std::true_type{});" in src, "the two forms of the A1 loop have moved"
    assert "const int i0 = 4 * lane, i1 = 4 * lane + 256;" in src, "the staging of the text has moved"
    assert "constexpr int SEG = 256;" in pipe and "constexpr int NPOS = SEG + 40;" in pipe and "constexpr int TEXT_LEN = SEG + 96;" in pipe, "SEG, NPOS or TEXT_LEN have moved"
    assert (SEG, M.NPOS, M.TEXT_LEN) == (256, 296, 352)
    assert (M.NPOS - 64) // 3 == M.TAIL_TASKS


def test_the_kernel_still_has_these_seams():
    kernel_constants()


# ---- a form: its vocabulary on the device, its oracle, the tails the oracle chose, its constructs --------------------------------------------------------
class Form:
    def __init__(self, name, norm_flag=0, extra=()):
        self.name = name
        self.capcode, self.charset, self.unk, self.wide, self.maxchars = M.form_props(name)
        toks, capcode, charset, unk = M.tokens(name)
        self.img = synth.build_vocab(list(dict.fromkeys(toks + list(extra))), capcode=capcode, charset=charset, norm_flag=norm_flag, with_unk=unk)
        self.v, self.orc = tm.Vocab(self.img), Oracle(self.img)
        assert (self.v.n_ids() > 65536) == self.wide
        self.fast = M.Fast(self.orc)
        self.fd = M.fd_tails(self.orc, name)
        assert bool(self.fd) == (self.capcode == 2), "the oracle found no tail that triggers a forward-delete state behind a chain"
        self.constructs = M.constructs(name, self.fd[0] if self.fd else None)
        self.by_name = {c.name: c for c in self.constructs}
        self.tails = M.tails(name, self.fd)
        self.fillers = M.fillers(name, self.orc)
        self.seam = M.seam_chars(name)
        self.longest = self.by_name["chain %d" % self.maxchars]
        self.deepest = self.by_name["depth 20"]
        self.cache = {}

    def expect(self, doc):
        e = self.cache.get(doc)
        if e is None:
            e = self.cache[doc] = self.fast.tokenize(doc)
        return e

    def place(self, filler, o, data, tail=b""):
        return M.place(self.name, filler, o, data, tail)


def form(name):
    if ("form", name) not in _made:
        _made[("form", name)] = Form(name)
    return _made[("form", name)]


def _offsets(f, n, full):
    """the filler lengths of the segment sweep for a construct of n characters (EMULATED: every third, and the construct's begin and end at 255, 256, 257)"""
    all_o = list(M.starts(n, f.seam))
    if full or not EMULATED:
        return all_o
    keep = set(all_o[::3]) | {f.seam - 1, f.seam, f.seam + 1} | {f.seam - n - 1, f.seam - n, f.seam - n + 1}
    return [o for o in all_o if o in keep]


def segment_rows(f, kind, full=False):
    """full: the sweep as the device runs it on the real device, whatever this process runs (the not-blind conditions are stated for that)"""
    rows = []
    for c in f.constructs:
        for o in _offsets(f, len(c.data), full):
            for tname, t in f.tails:
                doc = f.place(f.fillers[kind], o, c.data, t)
                for lead in (0,) if full else LEADS:
                    rows.append(((c.name, kind, o, tname, lead), doc, lead))
    return rows


END_PARTS = 6
END_E_EVERYWHERE = (39, 40, 41)      # dl of the segment in front of the end is NPOS - 1, NPOS, NPOS + 1: these stand at all four workgroup positions


def end_constructs(f, part):
    """the constructs of one part of the document-end sweep: by falling weight (its length, times eight where it stands at every e), each to the part
    that is lightest so far - the parts then cost the oracle about the same"""
    if part is None:
        return f.constructs
    weight = lambda c: len(c.data) * (8 if c is f.longest or c is f.deepest else 1)
    parts, load = [[] for _ in range(END_PARTS)], [0] * END_PARTS
    for c in sorted(f.constructs, key=lambda c: -weight(c)):
        k = load.index(min(load))
        parts[k].append(c)
        load[k] += weight(c)
    return parts[part]


def end_rows(f, j, part=None):
    rows = []
    for c in end_constructs(f, part):
        every = c is f.longest or c is f.deepest
        es = list(range(97)) if every and not EMULATED else M.END_E
        ks = list(range(1, len(c.data) + 1))
        if EMULATED:
            ks = sorted(set(ks[::3]) | {len(c.data)})
        for k in ks:
            for ei, e in enumerate(es):
                total = SEG * j + e
                if f.charset == 2:
                    if total % 2:
                        continue
                    total //= 2
                if total < k:
                    continue
                doc = f.place(f.fillers["token"], total - k, c.data[:k])
                for ph in range(4) if e in END_E_EVERYWHERE else ((k + ei + j) % 4,):
                    rows.append(((c.name, "end", k, total, j, ph), doc, ph))
    return rows


class Packed:
    """the documents of `rows`, each with its first segment at its index modulo 4: the next document is the first one left (in the rows' order) that wants
    the index the batch has reached; where none does, a one-byte document is put in"""

    def __init__(self, rows, pad=PAD):
        self.labels, self.docs, self.first_seg = [], [], []
        queue = [[r for r in reversed(rows) if r[2] == ph] for ph in range(4)]
        seg, left = 0, len(rows)
        while left:
            q = queue[seg % 4]
            label, doc = (None, pad) if not q else q.pop()[:2]
            assert doc
            left -= label is not None
            self.labels.append(label)
            self.docs.append(doc)
            self.first_seg.append(seg)
            seg += M.segments(len(doc))
        self.text, self.offs = tm.pack_documents(self.docs)


def score_strips(v, text, offs):
    d = np.ascontiguousarray(text)
    ds = C.c_void_p()
    N.check(N.lib.tm_dataset_upload(N.ptr(d), int(d.size), C.byref(ds)))
    try:
        so = np.ascontiguousarray(offs[:-1], dtype=np.uint64)
        sl = np.ascontiguousarray(np.diff(offs.astype(np.int64)), dtype=np.uint64)
        got = np.zeros(v.n_ids(), dtype=np.uint32)
        tit, ms = C.c_uint64(), np.zeros(32, dtype=np.uint8)
        N.check(N.lib.tm_score(v.handle, ds, N.ptr(so), N.ptr(sl), so.size, N.ptr(got), C.byref(tit), N.ptr(ms)))
        return got, tit.value, ms
    finally:
        N.lib.tm_dataset_free(ds)


def expected_scores(f, docs):
    """the oracle's histogram, tokens-in-text and missing set summed over docs: one walk per DISTINCT document, times how often it stands there"""
    mult = {}
    for d in docs:
        mult[d] = mult.get(d, 0) + 1
    total = np.zeros(f.orc.n_ids(), dtype=np.uint64)
    tit, ms = 0, np.zeros(32, dtype=np.uint8)
    by_m = {}
    for d, m in mult.items():
        by_m.setdefault(m, []).append(d)
    for m, ds in by_m.items():
        f.fast.scores[:] = 0
        for d in ds:
            t, s = f.fast.score(d)
            tit += m * t
            ms |= s
        total += m * f.fast.scores.astype(np.uint64)
    return total, tit, ms


def entry_states(f, rows):
    """the states in which the oracle's walk over each document leaves byte 256 (2 * offset + forward delete): from the oracle alone"""
    seen = set()
    for doc in {r[1] for r in rows if len(r[1]) > SEG}:
        seen.add(f.orc.score_range(doc, 0, SEG, 0)[3])
    return seen


def check_packed(f, rows, what, stats_wanted=None):
    t0 = time.time()
    oracle_stats(reset=True)
    p = Packed(rows, f.place(PAD, 1, b""))
    exp = [f.expect(d) for d in p.docs]
    st = oracle_stats()
    if stats_wanted:
        assert all(st[k] > 0 for k in stats_wanted), (what, st)      # (from the oracle alone, before the device is looked at)
    es, et, em = expected_scores(f, p.docs)
    t1 = time.time()
    ids, toff, missing = f.v.tokenize_packed(p.text, p.offs)
    counts, cmiss = f.v.count_packed(p.text, p.offs)
    gs, gt, gm = score_strips(f.v, p.text, p.offs)
    t2 = time.time()
    print("%s, %s: %d documents (%d of the sweep), %d bytes; oracle %.2f s, device %.2f s" % (f.name, what, len(p.docs), len(rows), p.text.size, t1 - t0, t2 - t1))
    e_toff = np.zeros(len(exp) + 1, dtype=np.uint64)
    np.cumsum([e[0].size for e in exp], out=e_toff[1:])
    e_ids = np.concatenate([e[0] for e in exp]) if exp else np.zeros(0, np.uint32)
    e_miss = np.array([e[1] for e in exp], dtype=np.int64)
    e_cnt = np.array([e[2] for e in exp], dtype=np.int64)
    e_cmiss = np.array([e[3] for e in exp], dtype=np.int64)
    ok = toff.size == e_toff.size and (toff == e_toff).all() and (ids == e_ids).all() and (missing.astype(np.int64) == e_miss).all()
    ok = ok and (counts.astype(np.int64) == e_cnt).all() and (cmiss.astype(np.int64) == e_cmiss).all()
    if not ok:
        bad = []
        for d in range(len(p.docs)):
            got = ids[int(toff[d]):int(toff[d + 1])]
            if got.size != exp[d][0].size or (got != exp[d][0]).any() or int(missing[d]) != exp[d][1] or int(counts[d]) != exp[d][2] or int(cmiss[d]) != exp[d][3]:
                bad.append((p.labels[d], "segment %d" % p.first_seg[d]))
                if len(bad) == 8:
                    break
        raise AssertionError("%s, %s: ids, counts or missing counts that are not the oracle's; the first (construct, kind, offset, tail, position): %s" % (f.name, what, bad))
    assert (gs == es).all() and gt == et and (gm == em).all(), "%s, %s: tm_score with a strip per document is not the sum of the oracle's walks" % (f.name, what)
    return p


# ---- the packed sweep ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", FILLERS)
@pytest.mark.parametrize("name", FORMS)
def test_every_construct_across_the_segment_seam_in_every_wavefront(name, kind):
    kernel_constants()
    f = form(name)
    rows = segment_rows(f, kind)
    # not blind, from the oracle alone: the walk leaves byte 256 in every entry state the form has; every (construct, offset) stands at all positions
    seen = entry_states(f, segment_rows(f, kind, full=True) if EMULATED else rows)
    want = set(range(0, 80, 2)) if f.capcode == 0 else {s for s in range(80) if not (s >> 1) & 1} if f.charset == 2 else set(range(80))
    assert want <= seen, "%s: entry states the sweep never leaves byte 256 in: %s" % (name, sorted(want - seen))
    if kind == "token":
        top = f.by_name["two longest tokens back to back"]
        doc = f.place(f.fillers[kind], f.seam - 1, top.data)
        spans = oracle_spans(f.orc, doc, f.unk).tolist()
        b = SEG - (1 if f.charset == 1 else 2)
        assert [b, b + 40] in spans and [b + 40, b + 80] in spans, "no 40-byte token at the segment's last position with a 40-byte token behind it"
        assert any(r[1] == doc for r in rows)
        if f.charset == 1:
            # the text ends at byte 296 with the 40-byte token at 255 (dl == NPOS where its segment shares nothing): which token begins there hangs on
            # the length of the look-ahead at the last byte - with a NUL behind the text `;` + NUL matches and the greedy token wins
            look = f.by_name["look-ahead at the document's last byte decides"]
            doc = f.place(f.fillers[kind], f.seam - 1, look.data)
            a, b = f.orc.tokenize(doc)[0], f.orc.tokenize(doc + b"\0")[0]
            assert len(doc) == M.NPOS and int(a[SEG - 1]) != int(b[SEG - 1]), "the look-ahead at the document's last byte decides nothing"
            assert {r[2] for r in rows if r[1] == doc} == set(LEADS)
        heads = f.by_name["80 chain heads"]
        o = f.seam - len(heads.data) - 1
        doc = f.place(f.fillers[kind], o, heads.data)
        first = o * (2 if f.charset == 2 else 1)
        n_heads = sum(1 for q in range(first, min(len(doc), SEG)) if f.orc.longest(doc[q:q + 40])[1] == 40)
        assert n_heads > M.TAIL_TASKS and any(r[1] == doc for r in rows), "no segment with more chain heads than the task list holds: %d" % n_heads
        if f.capcode == 2:
            many = f.by_name["18 forward-delete states"]
            doc = f.place(f.fillers[kind], f.seam - len(many.data) - 1, many.data)
            assert len(doc) <= SEG and M.fd_branches(f.orc, doc) >= M.SIDE_STRIDE and any(r[1] == doc for r in rows), "no segment with 16 forward-delete states"
    # ... and over the fuzz filler's half of the sweep the oracle's walk takes every exit it has
    p = check_packed(f, rows, "segment sweep, %s filler" % kind, None if kind == "token" else STATS_ALL if f.capcode == 2 else STATS_PLAIN)
    at = {}
    for label, s in zip(p.labels, p.first_seg):
        if label is not None:
            at.setdefault(label[:4], set()).add(s % 4)
    assert all(v == set(LEADS) for v in at.values())


@pytest.mark.gpu
@pytest.mark.parametrize("j,part", [(j, p) for j in END_J for p in ([None] if j == 0 else range(END_PARTS))], ids=lambda x: "all" if x is None else str(x))
@pytest.mark.parametrize("name", FORMS)
def test_every_construct_cut_at_every_byte_by_the_document_end(name, j, part):
    """(one test is one j and, for the documents of more than a segment, a sixth of the constructs: most of its time is the oracle's)"""
    kernel_constants()
    f = form(name)
    rows = end_rows(f, j, part)
    assert part is None or sorted(c.name for q in range(END_PARTS) for c in end_constructs(f, q)) == sorted(f.by_name)
    if f.longest in end_constructs(f, part):
        lens = {len(r[1]) for r in rows if r[0][0] == f.longest.name}
        want = {SEG * j + e for e in (range(97) if not EMULATED else M.END_E) if SEG * j + e > 0 and (f.charset == 1 or e % 2 == 0)}
        assert want <= lens, sorted(want - lens)
    p = check_packed(f, rows, "document end, j = %d, part %s" % (j, part))
    assert {s % 4 for label, s in zip(p.labels, p.first_seg) if label is not None} == {0, 1, 2, 3}
    if f.charset == 1:
        at = {}
        for label, s_ in zip(p.labels, p.first_seg):
            if label is not None and label[3] - SEG * j in END_E_EVERYWHERE:
                at.setdefault(label[:5], set()).add(s_ % 4)
        assert at and all(v == {0, 1, 2, 3} for v in at.values())


# ---- the long document -----------------------------------------------------------------------------------------------------------------------------------
STRADDLES = list(range(-1, 42))      # bytes (characters, UTF-16) of the construct in front of the boundary; -1: it begins one behind it


def long_document(f):
    """-> (document, {(construct, straddle)} placed, [(boundary, construct, straddle)], the constructs that fit between two boundaries).  The
    (construct, straddle) cycle counts the boundaries that are no multiple of 16 - those are the longest chain's - and runs through one whole period"""
    seam = f.seam
    cs = [c for c in f.constructs if len(c.data) <= seam - 42]
    assert len(cs) % len(STRADDLES) != 0      # (43 straddles, a prime: coprime periods)
    nseg = 40 if EMULATED else len(cs) * len(STRADDLES) * 16 // 15 + 3
    out, pos, placed, log, n = bytearray(), 0, set(), [], 0
    for b in range(1, nseg):
        if b % 16 == 0:
            c, s = f.longest, (1, 20, 39)[(b // 16) % 3]
        else:
            c, s = cs[n % len(cs)], STRADDLES[n % len(STRADDLES)]
            n += 1
        start = seam * b - s
        assert start >= pos
        out += M.FILL * (start - pos) + c.data
        pos = start + len(c.data)
        placed.add((c.name, s))
        log.append((b, c.name, s))
    out += M.FILL * 17
    doc = bytes(out)
    return (M.widen(doc) if f.charset == 2 else doc), placed, log, cs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["capcode2"] if EMULATED else ["capcode2", "capcode2-wide", "utf16"])
def test_a_construct_at_every_boundary_of_a_long_document(name):
    kernel_constants()
    f = form(name)
    doc, placed, log, cs = long_document(f)
    if not EMULATED:
        assert len(doc) > 513 * SEG and placed >= {(c.name, s) for c in cs for s in STRADDLES}, "not every (construct, straddle) pair is on a boundary"
        for step in (16, 64):
            assert {s for b, n, s in log if b % step == 0} == {1, 20, 39}
        assert [(n, s) for b, n, s in log if b == 512] == [(f.longest.name, 39)]
    docs = [doc, doc[:2 * SEG + 6], PAD, doc[:9 * SEG]]
    exp = [f.fast.tokenize(d) for d in docs]
    f.fast.scores[:] = 0
    et, em = f.fast.score(doc)
    es = f.fast.scores.copy()
    text, offs = tm.pack_documents(docs)
    whole = np.frombuffer(doc, dtype=np.uint8)
    for hook in HOOKS:
        old = N.lib.tm_debug_flags(hook)
        try:
            assert N.lib.tm_debug_flags(-1) == hook, "test hooks not armed"
            ids, toff, missing = f.v.tokenize_packed(text, offs)
            counts, cmiss = f.v.count_packed(text, offs)
            gs, gt, gm = score_strips(f.v, whole, np.array([0, whole.size], dtype=np.uint64))
        finally:
            N.lib.tm_debug_flags(old)
        for d in range(len(docs)):
            got = ids[int(toff[d]):int(toff[d + 1])]
            if got.size != exp[d][0].size or (got != exp[d][0]).any():
                k = int(np.argmax(got[:min(got.size, exp[d][0].size)] != exp[d][0][:min(got.size, exp[d][0].size)])) if got.size and exp[d][0].size else 0
                at = int(oracle_spans(f.orc, docs[d], f.unk)[k][0]) if d > 0 or EMULATED else -1
                raise AssertionError("hook %d, document %d: the ids differ from id %d on (byte %d; boundary, construct, straddle near it: %s)" % (
                    hook, d, k, at, [x for x in log if abs(x[0] * SEG - at) < 2 * SEG]))
            assert (int(missing[d]), int(counts[d]), int(cmiss[d])) == exp[d][1:], (hook, d)
        assert (gs == es).all() and gt == et and (gm == em).all(), "hook %d: the histogram of the long document" % hook


# ---- the slab sweep ------------------------------------------------------------------------------------------------------------------------------------------
def slab_form():
    if ("form", "slab") not in _made:
        _made[("form", "slab")] = Form("capcode2", norm_flag=1, extra=["́".encode(), "é".encode(), b"Ca", b"C"])
    return _made[("form", "slab")]


GROWTH = {"capital": b"A ", "e-acute": "é".encode()}      # each grows by one byte: C + a + space; e + the two bytes of U+0301


def slab_rows(f):
    """-> [(label, raw document)], {r: how many documents}"""
    heads = {}
    for kind, g in GROWTH.items():
        for k in range(0, 256):
            head = g * k
            raw = head + M.FILL * (1024 - len(head))
            r = len(f.v.normalize(raw)) % SEG
            heads.setdefault((kind, r), (head, len(f.v.normalize(raw)) - 1024))
    rows, seen = [], {}

    def add(c, s, r, kind):
        head, grow = heads[(kind, r)]
        start = 1024 - s      # the construct begins s bytes in front of the end of the first piece (raw and normalized: nothing in front of it but the head grows)
        raw = head + M.FILL * (start - len(head)) + c.data + M.FILL * 60
        rows.append(((c.name, "slab", s, r, kind), raw))
        seen[r] = seen.get(r, 0) + 1

    kinds = list(GROWTH)
    n = 0
    # the constructs the raw path can bring about: those the normalizer leaves as they are (capcode 2 puts a delete marker between a sign and a letter
    # behind it: the chains whose head byte is a digit or a sign are none of them; the 40-byte chain that branches at its end is all letters)
    stable = [c for c in f.constructs if bytes(f.v.normalize(M.FILL * 4 + c.data + M.FILL * 4)).endswith(M.FILL * 4 + c.data + M.FILL * 4)]
    top, pair = f.by_name["branch three bytes before the end"], f.by_name["two all-letter longest tokens back to back"]
    assert top in stable and pair in stable and len(top.data) == 40 and len(pair.data) == 80 and len(stable) >= 12, [c.name for c in stable]
    if not EMULATED:
        for c in stable:
            for s in STRADDLES:
                add(c, s, SLAB_R[n % 15], kinds[(n // 15) % 2])
                n += 1
    for r in SLAB_R_RUN:
        for kind in kinds:
            for s in STRADDLES:
                add(top, s, r, kind)
                if not EMULATED:
                    add(pair, s, r, kind)      # (the look-ahead of a 40-byte token at the far end of the staged bytes, read from the second slab)
    return rows, seen


@pytest.mark.gpu
@pytest.mark.parametrize("hook", [0, 2048])
def test_every_construct_across_the_end_of_a_normalizer_piece(hook):
    """the one-pass path: the match kernel stages its segments from the normalizer's slabs (len0; a dword across the end of a piece, in the segment's own
    256 bytes and in its second word per lane); hook 2048: the same text packed.  Expected: the oracle on Vocab.normalize(document), as fuzz_cases.one_raw"""
    kernel_constants()
    f = slab_form()
    rows, seen = slab_rows(f)
    assert set(seen) == set(SLAB_R_RUN if EMULATED else SLAB_R), "not every r occurs: %s" % sorted(seen)
    docs = [r[1] for r in rows]
    norm = [bytes(f.v.normalize(d)) for d in docs]
    for (label, raw), nd in zip(rows, norm):
        piece = bytes(f.v.normalize(raw[:1024]))
        assert nd.startswith(piece) and len(piece) % SEG == label[3], label
        c = f.by_name[label[0]]
        assert nd[len(piece) - label[2]:].startswith(c.data) if label[2] >= 0 else nd[len(piece) + 1:].startswith(c.data), label
    exp = [f.expect(d) for d in norm]
    old = N.lib.tm_debug_flags(hook)
    try:
        assert N.lib.tm_debug_flags(-1) == hook, "test hooks not armed"
        got = f.v.tokenize(docs)
    finally:
        N.lib.tm_debug_flags(old)
    bad = [rows[d][0] for d in range(len(docs)) if got[d].size != exp[d][0].size or (got[d] != exp[d][0]).any()]
    assert not bad, "hook %d: ids of the one-pass path that are not the oracle's on the normalized text; the first (construct, slab, straddle, r, growth): %s" % (hook, bad[:8])


# ---- the ring ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_ring_on_the_documents_of_the_segment_sweep():
    """Vocab.tokenize_pipeline(raw=True) with chunks of 16 KiB: chunk ends fall among the documents of the segment sweep (token filler, workgroup position
    0), and the ring's own emit kernel writes the ids"""
    f = slab_form()
    plain = form("capcode2")
    docs = list(dict.fromkeys(r[1] for r in segment_rows(plain, "token") if r[2] == 0))
    docs = docs[:300] if EMULATED else docs
    norm = [bytes(f.v.normalize(d)) for d in docs]
    exp = [f.expect(d) for d in norm]
    text, offs = tm.pack_documents(docs)
    blob, boff, bmiss, enc, st = f.v.tokenize_pipeline(text, offs, raw=True, chunk_bytes=16 * 1024, lanes=2)
    e_ids = np.concatenate([e[0] for e in exp])
    e_toff = np.zeros(len(exp) + 1, dtype=np.uint64)
    np.cumsum([e[0].size for e in exp], out=e_toff[1:])
    print("the ring: %d documents, %d raw bytes, stats %s" % (len(docs), text.size, st))
    assert st["chunks"] > 1, st
    assert (np.asarray(boff) == e_toff * enc).all(), "the ring: other token counts"
    w = np.zeros((e_ids.size, 4), dtype=np.uint8)
    w[:, :enc] = np.asarray(blob[:e_ids.size * enc]).reshape(e_ids.size, enc)
    assert (w.view(np.uint32).ravel() == e_ids).all(), "the ring: the ids are not the oracle's on the normalized text"


# ---- the exit maps: all 80 entry states --------------------------------------------------------------------------------------------------------------------
RANGE_TAILS = [0, 1, 40, 255]      # range lengths are 256 j + one of these


def range_text(f, c, tail):
    """one text with c + tail in it once for every s in 0 ... len(c), and cuts: the cut of placement s falls s bytes into the construct; the ranges between
    the cuts have lengths 256 j + {0, 1, 40, 255} in rotation (j = 0: 255 only - a range that is followed by more text has at least 64 bytes): the last segment
    of a range of 257 or 296 bytes is 1 or 40 bytes short AND followed by text, so an entry state beyond it passes through it whole"""
    big = [SEG * j + t for j in (1, 2) for t in RANGE_TAILS] + [255]
    out, cuts, n = bytearray(M.FILL * 3), [0], 0
    step = 3 if EMULATED else 1
    ss = list(range(0, len(c.data) + 1, step))
    while len(ss) < len(big):      # (a short construct: again, until every range length has stood)
        ss += ss
    for s in ss:
        length = big[n % len(big)]
        cut = cuts[-1] + length
        start = cut - s
        if start < len(out):      # (the range is too short to clear what is written: one more segment)
            cut += SEG * ((len(out) - start + SEG - 1) // SEG)
            start = cut - s
        out += M.FILL * (start - len(out)) + c.data + tail + M.FILL * 2
        cuts.append(cut)
        n += 1
    out += M.FILL * (cuts[-1] + 300 - len(out))
    cuts.append(len(out))
    return bytes(out), cuts


def steps_into_fd(f, data):
    """the positions p the oracle can arrive at in a forward-delete state: one step from every plain state (q, 0) of the text, and from every forward-delete
    state so found; from the oracle alone"""
    d = np.frombuffer(data, dtype=np.uint8)
    fn = f.orc.L.tmo_score_range
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint32)]
    scores = np.zeros(f.orc.n_ids(), dtype=np.uint32)
    ms, tit, ex = np.zeros(32, dtype=np.uint8), C.c_uint64(0), C.c_uint32(0)
    reach, todo = set(), [(q, 0) for q in range(d.size)]
    while todo:      # ... and from every forward-delete state found that way, to a fixed point
        q, fd = todo.pop()
        fn(f.orc.h, d.ctypes.data, d.size, q, fd, q + 1, scores.ctypes.data, C.byref(tit), ms.ctypes.data, C.byref(ex))
        nxt = q + 1 + (ex.value >> 1)
        if ex.value & 1 and nxt not in reach and nxt < d.size:
            reach.add(nxt)
            todo.append((nxt, 1))
    return reach


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["longest chain", "chain 33", "depth 13", "forward-delete tail", "multi-word", "missing byte"])
def test_all_eighty_entries_of_the_exit_map_with_a_construct_across_the_cut(which):
    kernel_constants()
    f = form("capcode2")
    c, tail = {"longest chain": (f.longest, b""), "chain 33": (f.by_name["chain 33"], b""), "depth 13": (f.by_name["depth 13"], b""),
               "forward-delete tail": (f.by_name["chain 5"], f.fd[0]), "multi-word": (f.by_name["multi-word"], b""),
               "missing byte": (f.by_name["a byte without a token"], b"")}[which]
    if which == "forward-delete tail":
        c = M.Construct("chain 5 + tail", c.data + tail, "a chain token, the forward-delete trigger behind it: the cut falls into the trigger as well")
        tail = b""
    data_b, cuts = range_text(f, c, tail)
    data = np.frombuffer(data_b, dtype=np.uint8)
    lens = {b - a for a, b in zip(cuts, cuts[1:-1])}
    assert lens >= {255, 256, 257, 296, 511, 512, 513, 552, 767}, sorted(lens)
    fd_reach = steps_into_fd(f, data_b)
    if which == "forward-delete tail":      # (from the oracle alone) some range is entered in a forward-delete state the walk can be in
        assert any(p in fd_reach for a in cuts[:-1] for p in range(a, a + 40))
    exp_s, exp_t, exp_m = f.orc.score(data)
    all_exits, hists, handles = [], [], []
    checked = unreachable = 0
    try:
        for a, b in zip(cuts, cuts[1:]):
            own = np.ascontiguousarray(data[a:min(b + tmdist.HALO, data.size)])
            ds = C.c_void_p()
            N.check(N.lib.tm_dataset_upload(N.ptr(own), own.size, C.byref(ds)))
            handles.append(ds)
            eng = tmdist.HipRange(f.v, ds, b - a, continues=b < data.size, text_ends_in_halo=data.size - b < tmdist.HALO)
            ex = eng.begin()
            for e in range(80):
                p = a + e // 2
                if p > data.size:
                    continue
                if ex[e] == tmdist.UNREACHABLE:
                    # only a state the oracle cannot be in: a forward-delete state at a position no step of its walk arrives at in that state
                    assert e & 1 and p not in fd_reach, "range [%d, %d): entry state %d is unreachable on the device, the oracle can be in it" % (a, b, e)
                    unreachable += 1
                else:
                    assert int(ex[e]) == f.orc.score_range(data, a, b, e)[3], "range [%d, %d), entry state %d (cuts %s)" % (a, b, e, cuts[:6])
                    checked += 1
            all_exits.append(ex)
            eng.finish(tmdist.resolve_entry(all_exits, len(all_exits) - 1))
            s_ = np.zeros(f.v.n_ids(), dtype=np.uint32)
            t_, m_ = C.c_uint64(), np.zeros(32, dtype=np.uint8)
            N.check(N.lib.tm_score_read(f.v.handle, ds, N.ptr(s_), C.byref(t_), N.ptr(m_)))
            hists.append((s_, t_.value, m_))
    finally:
        for ds in handles:
            N.lib.tm_dataset_free(ds)
    print("%s: %d ranges, %d entries compared, %d unreachable" % (which, len(cuts) - 1, checked, unreachable))
    assert checked >= 40 * (len(cuts) - 1)
    got_s = sum(h[0].astype(np.uint64) for h in hists)
    assert (got_s == exp_s).all() and sum(h[1] for h in hists) == exp_t
    assert (np.bitwise_or.reduce(np.stack([h[2] for h in hists])) == exp_m).all()
    assert which == "missing byte" or any(tmdist.resolve_entry(all_exits, r) != 0 for r in range(1, len(all_exits)))      # some cut fell inside a token

"""Every construct of tests/filter_cases.py at every byte offset across every seam of the device FILTER pass (tm_norm.hip: k_pf_filter,
k_pf_long<false|true>, k_pf_begin, pf_scan_span, pf_emit_span), with the document in every state of its numbers (PfDoc) and every tail, under
every set of the byte-level flags, against the host normalizer (synth.normalize_batch: tm_normalize.cpp - pinned to the reference runtime for
all 256 flag values by tests/test_builder_normalizer.py, and on these very constructs by tests/test_filter_boundaries_emulated.py).  The
vocabulary is 256 one-byte tokens with capcode 2.

The seams, stated here as the constants they are - if the kernel's constants move, test_the_kernel_still_has_these_seams fails and the sweep
does not go blind:

  4, 8              LANE: a lane's dword; p1 / p2 / n1 / n2 are shifts against the neighbouring lane's dword         tm_norm.hip:838-841, :916-923
  252, 256, 260     STEP -/+ LANE and STEP: 256 bytes per step of the sweep; lane 0 takes the step before through
                    carry / carry_s, lane 63 the step after through the prefetched xn                               tm_norm.hip:836-839, :911-918, :929-930
  512               the second step seam: carry and xn once they have been handed on                                the same
  4096, 4348, 8192  PF_SPAN, PF_SPAN + 252, 2 * PF_SPAN: the ends of a wavefront's span in a document of more than
                    PF_WHOLE bytes (three launches, pf_add_span combines the spans' numbers; the emit sweep of a
                    span begins at (rb & ~3) - 4, so its step seams are rb - 4 + 256 k) - and the same three in
                    documents of at most PF_WHOLE bytes, where they are plain step seams                            tm_norm.hip:790-799, :877-882, :909-910, :1019
  16384 | 16385     PF_WHOLE: one wavefront per document | a wavefront per span; documents of exactly 16383, 16384,
                    16385 and 20481 bytes (the last span of the last holds ONE byte) with the construct first, last
                    and across byte 16384                                                                            tm_norm.hip:799, :992-993, :1018
  head              start 0..5: nothing in front of lane 0, and the emit sweep's base is 0 up to a = 7              tm_norm.hip:909-910
  end               the construct at 8..11 in front of every tail: every document length mod 4 (pf_load masks the
                    last dword)                                                                                       tm_norm.hip:809-814

The short batch (seams below 4096, head, end) is the full product construct x start x state x tail, less the states whose prefix is longer than
the start (filter_cases.place: at the seams 4 and 8 only the short prefixes fit).  It runs under all 64 combinations of the bits 4, 8, 16, 32,
64, 128 and under 255 and 2|8|16|32|128 (bits 1 and 2 ride along once).

The long batch (seams from 4096, the length switch, the named documents) runs under LONG_FLAGS, twelve sets.  Its states and tails are cut by this
rule: placement number k (constructs, seams and starts counted in order) stands once behind state STATES_LONG[k mod 8] in front of tail
TAILS_LONG[k mod 5], once behind STATES_LONG[(k + 3) mod 8] in front of TAILS_LONG[(k + 2) mod 5] - a state of every kind (none, one drop, two
drops, a quote first, a quote suppressed, a CR LF drop, 3 and 300 blanks), and 8 and 5 are coprime: every pair occurs.  Each such document
exists twice: padded with filler to 16385 + k mod 16 bytes (behind the tail; in front of a tail of blanks, which stay the last bytes), and
unpadded.  NAMED are documents put in by hand - the kinds test_the_sweep_is_what_it_says asks for, whatever the rotation gives - and any
document that ever failed stays there by name.

No construct is kept out of any flag set: the number of documents the device leaves to the host is stated EXACTLY for every flag set by
filter_cases.host_doc (malformed UTF-8; under accents the three-byte mark U+20DD; under trim + leadingspace the documents without leading
blanks whose last non-blank byte ends a character of more than one byte that is not a replaced quote - the cut leaves half of it).  DOCUMENTS
are kept out of the 17 flag sets with trim AND leadingspace: without quotemarks the last kind alone is 43 % of the short batch, and a document
left to the host tests nothing of the kernel - so of the documents the rules say the cut leaves half a character of, only every sixteenth (in
the batch's order) is in the batch of such a flag set (class Batch); every other document is in every flag set's batch.  With that at most a
quarter of either batch is the host's under every flag set (checked at import, from those rules, on the CPU: 8 to 19 %, 23 % at the most in the cut for the emulated device).

On the emulated device (tests/test_filter_boundaries_emulated.py) the sweep is cut by fixed rule: the seams 4, 256 and 4096, head and end, the
twelve flag sets of LONG_FLAGS for both batches, the states of STATES_LONG and the tails of TAILS_LONG in the short batch, the one document
length 16385 at the switch, and 1500 documents of the short batch through the ring and under hook 2048."""
import os
import time

import numpy as np
import pytest

import filter_cases as F
import tokenmonster_amd as tm
from conftest import EMULATED
from tokenmonster_amd import _native as N
from tokenmonster_amd import synth
from tokenmonster_amd.vocab import PinnedBuffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE, STEP, SPAN, WHOLE = 4, 256, 4096, 16384
SHORT_SEAMS = (LANE, STEP) if EMULATED else (LANE, 2 * LANE, STEP - LANE, STEP, STEP + LANE, 2 * STEP)
LONG_SEAMS = (SPAN,) if EMULATED else (SPAN, SPAN + STEP - LANE, 2 * SPAN)
SWITCH_LENGTHS = (WHOLE + 1,) if EMULATED else (WHOLE - 1, WHOLE, WHOLE + 1, 5 * SPAN + 1)
EXAMPLE_FLAGS = 2 | 8 | 16 | 32 | 128      # lowercase collapse trim quotemarks unixlines: the reference's own example
LONG_FLAGS = [8 | 16, 8 | 16 | 128, 16 | 128, 128, 8, 32, 32 | 64, 8 | 16 | 32 | 64, 8 | 16 | 32 | 64 | 128, 4 | 8 | 16 | 32, 4 | 64, 255]
SHORT_FLAGS = list(LONG_FLAGS) if EMULATED else F.FLAGS64 + [255, EXAMPLE_FLAGS]
SHORT_STATES = F.STATES_LONG if EMULATED else [s[0] for s in F.STATES]
SHORT_TAILS = F.TAILS_LONG if EMULATED else [t[0] for t in F.TAILS]
RING_DOCS = 1500 if EMULATED else None      # how many documents of the short batch go through the ring and under hook 2048
CAPCODE = 2


def _chunks(xs, n):
    return [tuple(xs[i:i + n]) for i in range(0, len(xs), n)]


SHORT_GROUPS = _chunks(SHORT_FLAGS, 6)      # one test is one group of flag sets
LONG_GROUPS = _chunks(LONG_FLAGS, 3)

_made = {}


@pytest.fixture(scope="module", autouse=True)
def release_what_was_made():
    """the documents and references of this module are made once and shared by its tests - and given back when the last of them has run"""
    yield
    _made.clear()


def kernel_constants():
    src = open(os.path.join(ROOT, "tokenmonster_amd", "csrc", "tm_norm.hip"), encoding="utf-8").read()
    assert "#define TM_PF_SPAN %du" % SPAN in src and "#define TM_PF_WHOLE %du" % WHOLE in src, \
        "tm_norm.hip no longer says TM_PF_SPAN 4096u and TM_PF_WHOLE 16384u: the seams of this sweep are not the kernel's"
    assert "PF_SPAN = TM_PF_SPAN, PF_WHOLE = TM_PF_WHOLE" in src and "n <= PF_WHOLE ? (n ? 1u : 0u)" in src, "tm_norm.hip: the one-span / many-spans switch has moved"
    assert "for (uint32_t base = rb; base < re && (want_s || want_a); base += 256u)" in src and "for (; base < ehi; base += 256u)" in src \
        and "pf_load(win, base + 4u * lane, n)" in src, "tm_norm.hip: the filter pass no longer sweeps 256 bytes per step, a dword per lane"
    assert "uint32_t base = elo & ~3u;\n  if (base >= 4u) base -= 4u;" in src, "tm_norm.hip: a span's emit sweep no longer begins a dword early"


def test_the_kernel_still_has_these_seams():
    kernel_constants()


# ---- the documents -----------------------------------------------------------------------------------------------------------------------------------
class View:
    """the documents of a batch that run under one flag set: labels [(construct, seam, start, state, tail)], documents, packed when first asked
    for; host_docs: how many of them the RULES say are the host's"""

    def __init__(self, name, rows, cut_host):
        self.name = name
        self.labels = [r[0] for r in rows]
        self.docs = [r[1] for r in rows]
        self.constructs = [r[2] for r in rows]
        self.by_rule = {r: sum(1 for row in rows if row[2] is not None and row[2].rule == r) for r in F.RULES}
        self.cut_host = cut_host      # the documents of which trim + leadingspace leave half a character (and whose construct does not make them the host's anyway)
        self._packed = None

    @property
    def text(self):
        return self.packed()[0]

    @property
    def offs(self):
        return self.packed()[1]

    def packed(self):
        if self._packed is None:
            self._packed = tm.pack_documents(self.docs)
        return self._packed

    def host_docs(self, flag):
        return self.cut_host + sum(n for r, n in self.by_rule.items() if F.RULES[r][0](flag))


class Batch:
    """Under a flag set with trim AND leadingspace a document without leading blanks loses its last non-blank byte as well; where that byte ends
    a character of more than one byte - any but a replaced quote - the document is the host's.  Without quotemarks in the set that is nearly
    half the batch, so of the documents the rules say the cut leaves half a character of, only EVERY SIXTEENTH (in the batch's order) is in that
    flag set's batch; every other document is in every flag set's."""

    def __init__(self, name, rows):
        self.name, self.rows = name, rows
        # the documents the cut can leave half a character of: no leading blank, the last non-blank byte above 7F
        self.cut = [k for k, r in enumerate(rows) if r[1] and r[1][0] > 32 and r[1].rstrip(b"\x00\t\n\v\f\r ")[-1:] >= b"\x80"]
        self._views, self._halved = {}, {}

    def view(self, flag):
        both = (flag & 96) == 96
        key = flag & (F.ACCENTS | F.QUOTES | F.COLLAPSE | F.UNIX) if both else None      # all of the flags that the rules and the model of the quotes look at
        if key not in self._views:
            rows, kept = self.rows, 0
            if both:
                model = flag & (F.QUOTES | F.COLLAPSE | F.UNIX)      # (what the verdict on the last quote hangs on)
                if model not in self._halved:
                    self._halved[model] = [k for k in self.cut if F.host_doc(self.rows[k][1], flag, None)]
                halved = [k for k in self._halved[model] if not (self.rows[k][2] is not None and F.RULES[self.rows[k][2].rule][0](flag))]
                out = set(halved) - set(halved[::16])
                rows, kept = [r for k, r in enumerate(self.rows) if k not in out], len(halved[::16])
            self._views[key] = View(self.name, rows, kept)
        return self._views[key]


def _add(rows, label, doc, c):
    if doc is not None:
        rows.append((label, doc, c))


def short_rows():
    rows = []
    for c in F.CONSTRUCTS:
        n = len(c.data)
        places = [(seam, start) for seam in SHORT_SEAMS for start in F.starts(n, seam)]
        places += [("head", start) for start in range(0, 6)] + [("end", start) for start in range(8, 12)]
        for seam, start in places:
            for state in SHORT_STATES:
                for tail in SHORT_TAILS:
                    _add(rows, (c.name, seam, start, state, tail), F.place(c, seam, start, state, tail), c)
    return rows


# documents put in by hand: (name, bytes).  q = a quote, 2 = a double space; the spans of 4096 bytes they lie in, in order
_Q, _X = "’".encode(), F.FILLER
NAMED = [
    ("q in span 0, 2 in span 2, q in span 3", _X * 100 + _Q + _X * (2 * SPAN) + b"  " + _X * SPAN + _Q + _X * SPAN),
    ("2 in span 0, q in spans 1 and 2, 2 in span 3, q in span 4", _X * 9 + b"  " + _X * SPAN + _Q + _X * SPAN + _Q + _X * SPAN + b"  " + _X * SPAN + _Q + _X * 9),
    ("2 as the last bytes of span 1, 2 as the first of span 2", _X * (2 * SPAN - 2) + b"  " + b"  " + _X * (2 * SPAN + 77) + _Q),
    ("blank spans at both ends", F.BLANKS * 1500 + _X + b"  " + _Q + _X * (3 * SPAN) + _Q + b" \t" * 2500),
    ("blank from end to end, five spans", b" \t\n " * (5 * SPAN // 4) + b" "),
    ("one non-blank byte in span 2 of five", b"\t" * (2 * SPAN + 5) + b"x" + b"\t" * (3 * SPAN - 5)),
]


def long_rows():
    rows, k = [], 0
    for c in F.CONSTRUCTS:
        n = len(c.data)
        for seam in LONG_SEAMS:
            for start in F.starts(n, seam):
                for j in (0, 1):
                    state, tail = F.STATES_LONG[(k + 3 * j) % 8], F.TAILS_LONG[(k + 2 * j) % 5]
                    _add(rows, (c.name, seam, start, state, tail + ", padded"), F.place(c, seam, start, state, tail, WHOLE + 1 + k % 16), c)
                    _add(rows, (c.name, seam, start, state, tail), F.place(c, seam, start, state, tail), c)
                k += 1
        for total in SWITCH_LENGTHS:      # the length switch: the construct first, last, and across byte 16384
            state, tail = F.STATES_LONG[k % 8], F.TAILS_LONG[k % 5]
            _add(rows, (c.name, "first of %d" % total, 0, "none", tail), F.place(c, 0, 0, "none", tail, total), c)
            _add(rows, (c.name, "last of %d" % total, total - n, state, "nothing"), F.place(c, total, total - n, state, "nothing", total), c)
            k += 1
            if total > WHOLE:
                for start in F.starts(n, WHOLE):
                    state, tail = F.STATES_LONG[k % 8], F.TAILS_LONG[k % 5]
                    _add(rows, (c.name, "%d of %d" % (WHOLE, total), start, state, tail), F.place(c, WHOLE, start, state, tail, total), c)
                    k += 1
    for name, doc in NAMED:
        rows.append(((name, "named", 0, "none", "nothing"), doc, None))
    return rows


def batch(which):
    if which not in _made:
        _made[which] = Batch(which, short_rows() if which == "short" else long_rows())
    return _made[which]


def _at_most_a_quarter_is_the_hosts():
    """a document left to the host tests nothing of the kernel.  Counted from the rules; the documents made for the count are let go again, a
    test that needs them makes them (batch())"""
    for b, flags in ((Batch("short", short_rows()), SHORT_FLAGS + [EXAMPLE_FLAGS]), (Batch("long", long_rows()), LONG_FLAGS)):
        for flag in flags:
            v = b.view(flag)
            assert 4 * v.host_docs(flag) <= len(v.docs), "more than a quarter of the %s batch is the host's under the flags %d: %d of %d" % (b.name, flag, v.host_docs(flag), len(v.docs))


_at_most_a_quarter_is_the_hosts()


def vocab(flag):
    return tm.Vocab(synth.build_vocab([bytes([c]) for c in range(256)], capcode=CAPCODE, charset=1, norm_flag=flag))


def expected(b, flag):
    """the host normalizer's text and offsets (kept only for the example flags, which three tests share)"""
    key = ("e", b.name, flag)
    if key in _made:
        return _made[key]
    e = synth.normalize_batch(b.text, b.offs, CAPCODE, flag)
    if flag == EXAMPLE_FLAGS:
        _made[key] = e
    return e


def check(b, flag):
    b = b.view(flag)
    t0 = time.time()
    etext, eoff = expected(b, flag)
    t1 = time.time()
    v = vocab(flag)
    try:
        got, goff, nfb = v.normalize_packed_device(b.text, b.offs)
    finally:
        v.close()
    t2 = time.time()
    host = b.host_docs(flag)
    print("flags %3d, %s batch: %d documents, %d raw bytes, %d expected on the host (%.1f %%), %d were; reference %.2f s, device %.2f s" % (
        flag, b.name, len(b.docs), b.text.size, host, 100.0 * host / len(b.docs), nfb, t1 - t0, t2 - t1))
    assert goff.size == eoff.size
    if not ((goff == eoff).all() and got.size == etext.size and got.tobytes() == etext.tobytes()):
        bad = []
        for k in range(len(b.docs)):
            if got[int(goff[k]):int(goff[k + 1])].tobytes() != etext[int(eoff[k]):int(eoff[k + 1])].tobytes():
                bad.append(b.labels[k] + (flag,))
                if len(bad) == 8:
                    break
        raise AssertionError("flags %d, %s batch: documents that are not the host normalizer's; the first (construct, seam, start, state, tail, flag): %s" % (flag, b.name, bad))
    assert nfb == host, "flags %d, %s batch: %d documents took the host path, the rules say %d" % (flag, b.name, nfb, host)


def test_the_sweep_is_what_it_says():
    """the sweep's own side, without a device.  By the model of the document's numbers (filter_cases.numbers) the batches hold, under 8|16, at
    least one document of each kind the filter pass treats differently; every construct straddles every seam at every offset; and under 8|16
    the model's verdict on every quote - replaced or left alone - is what the host normalizer's output shows (that checks the model, not the
    kernel).  zlo differs from z only where quotes are replaced, so that pair is looked for under 8|16|32|64."""
    flag = F.QUOTES | F.COLLAPSE
    kinds = dict.fromkeys(["a quote suppressed", "a quote replaced", "s1 in one step, s2 in the next", "s1 in one span, s2 in a later span",
                           "fq in a span in front of the span of s1", "a beyond byte 256", "z more than 256 bytes in front of the end",
                           "trim + leadingspace cut a replaced quote (zlo = z - 2)", "trim + leadingspace cut into a suppressed quote (zlo = z)"], 0)
    for b in (batch("short").view(0), batch("long").view(0)):      # (flags 0: every document)
        etext, eoff = synth.normalize_batch(b.text, b.offs, 0, flag)      # capcode 0: the filtered text itself
        for k, doc in enumerate(b.docs):
            r = F.numbers(doc, flag)
            many = len(doc) > WHOLE
            for t, replaced in r.quotes:
                kinds["a quote replaced" if replaced else "a quote suppressed"] += 1
            if r.s2 is not None:
                kinds["s1 in one step, s2 in the next"] += r.s1 // STEP + 1 == r.s2 // STEP
                kinds["s1 in one span, s2 in a later span"] += many and r.s1 // SPAN < r.s2 // SPAN
            if r.s1 is not None and r.fq is not None:
                kinds["fq in a span in front of the span of s1"] += many and r.fq // SPAN < r.s1 // SPAN
            if r.a is not None:
                kinds["a beyond byte 256"] += r.a > STEP
                kinds["z more than 256 bytes in front of the end"] += len(doc) - 1 - r.z > STEP
            if r.quotes:
                left = F.quotes_left(etext[int(eoff[k]):int(eoff[k + 1])].tobytes())
                assert left == F.expected_quotes(doc, flag), (b.labels[k], left)
    both = flag | F.TRIM | F.LEAD      # ... on the documents that RUN under 8|16|32|64: fifteen of sixteen of the second kind are kept out of that batch
    for b in (batch("short").view(both), batch("long").view(both)):
        for doc in b.docs:
            r = F.numbers(doc, both)
            if r.a == 0 and r.quotes and r.quotes[-1][0] == r.z:
                kinds["trim + leadingspace cut a replaced quote (zlo = z - 2)" if r.zlo == r.z - 2 else "trim + leadingspace cut into a suppressed quote (zlo = z)"] += 1
    assert all(kinds.values()), kinds
    for c in F.CONSTRUCTS:
        n = len(c.data)
        for seam in SHORT_SEAMS + LONG_SEAMS + (WHOLE,):
            assert list(F.starts(n, seam)) == list(range(max(seam - n - 1, 0), seam + 2))
    # every state of the table is in the short batch at a step seam, every kind of state in the long one; documents on either side of the switch
    labels = batch("short").view(0).labels
    fits = [s for s in SHORT_STATES if len(F.STATE[s][1]) < STEP]      # (300 blanks: in front of the seam 512, and in the long batch)
    assert {(l[3], l[4]) for l in labels if l[1] == STEP} == {(s, t) for s in fits for t in SHORT_TAILS}
    assert EMULATED or {l[3] for l in labels if l[1] == 2 * STEP} == set(SHORT_STATES)
    assert {l[3] for l in batch("long").view(0).labels if l[1] == SPAN} == set(F.STATES_LONG)
    assert {F.STATE[s][2] for s in F.STATES_LONG} == {s[2] for s in F.STATES}
    lens = {len(d) for d in batch("long").view(0).docs}
    assert set(SWITCH_LENGTHS) <= lens and any(WHOLE < n <= WHOLE + 16 for n in lens) and any(SPAN < n <= WHOLE for n in lens)
    # the character accents turns into two OTHER bytes does so by the host's own function (remove_marks, ICU), not by this table's word
    left = bytes(synth.normalize("й".encode(), 0, F.ACCENTS))
    assert len(left) == 2 and left != "й".encode() and left == "и".encode()
    assert bytes(synth.normalize("é ñ É ß x́".encode(), 0, F.ACCENTS)) == "e n E ß x".encode()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", SHORT_GROUPS, ids=["flags-" + "-".join(map(str, g)) for g in SHORT_GROUPS])
def test_every_construct_across_the_lane_and_step_seams(flags):
    kernel_constants()
    for flag in flags:
        check(batch("short"), flag)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", LONG_GROUPS, ids=["flags-" + "-".join(map(str, g)) for g in LONG_GROUPS])
def test_every_construct_across_the_span_seams_and_the_length_switch(flags):
    kernel_constants()
    for flag in flags:
        check(batch("long"), flag)


# ---- the same documents through the ring and with the text packed --------------------------------------------------------------------------------
def ring_batch(device_only=False):
    """the short batch under the example flags (on the emulated device its first RING_DOCS documents) -> (labels, documents, raw text, offsets,
    expected text, expected offsets).  device_only: without the documents the rules say are the host's - a chunk of the ring that holds one is
    done again by the exact path, which throws away what the ring's filter pass made of it"""
    b = batch("short").view(EXAMPLE_FLAGS)
    keep = [k for k in range(len(b.docs)) if not (device_only and F.host_doc(b.docs[k], EXAMPLE_FLAGS, b.constructs[k]))]
    keep = keep if RING_DOCS is None else keep[:RING_DOCS]
    if not device_only and len(keep) == len(b.docs):
        text, offs = b.text, b.offs
        etext, eoff = expected(b, EXAMPLE_FLAGS)
    else:
        text, offs = tm.pack_documents([b.docs[k] for k in keep])
        etext, eoff = synth.normalize_batch(text, offs, CAPCODE, EXAMPLE_FLAGS)
    return [b.labels[k] for k in keep], [b.docs[k] for k in keep], text, offs, etext, eoff


@pytest.mark.gpu
def test_the_ring_runs_the_filter_pass_on_the_same_documents():
    """Vocab.tokenize_pipeline with page-locked buffers and chunks of 64 KiB: the ring (stats: ring == 1, more than one chunk) runs the filter
    pass with the piece count left on the device.  Only the documents the rules leave to the device are sent, and NO chunk may be done again
    by the exact path (ring_exact_chunks == 0): every id then comes from the ring's own filter and normalizer calls.  The ids are those of the
    host-normalized text."""
    labels, docs, text, offs, etext, eoff = ring_batch(device_only=True)
    assert len(docs) >= (RING_DOCS or 100_000)
    v = vocab(EXAMPLE_FLAGS)
    try:
        eids, etoff, _ = v.tokenize_packed(etext, eoff)
        pin, pout = PinnedBuffer(int(text.size)), PinnedBuffer(4 * eids.size + 64)
        pin.array[:text.size] = text
        blob, boff, _, enc, st = v.tokenize_pipeline(pin.array[:text.size], offs, raw=True, chunk_bytes=64 * 1024, lanes=2, out=pout.array)
        blob, boff = np.array(blob[:eids.size * enc]), np.array(boff)
    finally:
        v.close()
    print("the ring: %d documents, %d raw bytes, stats %s" % (len(docs), text.size, st))
    assert st["ring"] == 1 and st["chunks"] >= text.size // (64 * 1024) > 1, st
    assert st["ring_exact_chunks"] == 0 and st["host_fallback_docs"] == 0, st
    assert (boff == etoff * enc).all(), "the ring: other token counts"
    w = np.zeros((eids.size, 4), dtype=np.uint8)
    w[:, :enc] = blob.reshape(eids.size, enc)
    ids = w.view(np.uint32).ravel()
    if not (ids == eids).all():
        k = int(np.argmax(ids != eids))
        d = int(np.searchsorted(etoff, k, side="right")) - 1
        raise AssertionError("the ring: the ids of %s are not those of the host-normalized text" % (labels[d] + (EXAMPLE_FLAGS,),))


@pytest.mark.gpu
def test_the_same_documents_with_the_text_packed():
    """hook 2048, armed as tests/test_gpu_normalize_paths.py arms it: the normalized text packed instead of staying in the slabs"""
    labels, docs, text, offs, etext, eoff = ring_batch()
    v = vocab(EXAMPLE_FLAGS)
    old = N.lib.tm_debug_flags(2048)
    try:
        assert N.lib.tm_debug_flags(-1) == 2048, "test hooks not armed"
        eids, etoff, _ = v.tokenize_packed(etext, eoff)
        ids = v.tokenize(docs)
    finally:
        N.lib.tm_debug_flags(old)
        v.close()
    sizes = np.cumsum(np.array([g.size for g in ids], dtype=np.uint64))
    flat = np.concatenate(ids)
    if not ((sizes == etoff[1:]).all() and (flat == eids).all()):
        bad = [labels[d] + (EXAMPLE_FLAGS,) for d in range(len(ids)) if ids[d].tobytes() != eids[int(etoff[d]):int(etoff[d + 1])].tobytes()]
        raise AssertionError("hook 2048: the ids are not those of the host-normalized text: %s" % bad[:6])

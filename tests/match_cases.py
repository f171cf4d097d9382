"""What the match kernel (tm_kernels.hip: k_match_branch - K1 - with k_resolve and the group kernels - K3 - and k_emit_list / k_score_list - K4)
tells apart, as short byte strings ("constructs") to be placed at every byte offset across the seams of that kernel, behind a filler and in front
of a tail: shared by tests/test_gpu_match_boundaries.py and its emulated twin.  A helper, no tests.

One vocabulary recipe (tokens()): conftest.fuzz_vocab_tokens(rng, capcode, 200) - alternatives, ties, forward-delete pairs over `abcde` and a few
signs - plus tokens over letters and signs that alphabet does not use, so that a walk of K1 reaches what random text over five letters never
does: a chain record, depth TM_K1_DEFER_DEPTH, an entry offset of 39.

  k + head + body   one-child chains of every length 4 ... 40 that end in a letter (the head byte is the chain's own: nothing else shares `k` + head)
  f + head + body;  ... and that end in a sign
  the same without their first byte: suffix links lead into them
  m, mm, ... m*20   a path on which every node accepts: no chain, the walk gets to depth 12 a probe at a time
  kk + body         a 40-byte chain with keys at 10 and 25 bytes
  km + body + rst | uvw   a chain that branches three bytes before its end
  k$ + body ... @   (with the 33-byte chain k + `r` + body) the chain's suffix is a token that goes on with `@`: entered through a suffix link
  k + space + body, and space + body + ;   two ways through the same 41 bytes: which one the walk takes hangs on how long the token at `;` is -
                    at a document's last byte that is the pad byte's business (tail_here)
  z*40, zz, zzz, y*33, yy   every position of a run of `z` stands at the head of a chain
   ghi jln, ...     multi-word tokens
  a one-byte token for every byte of the above and of the fillers, and the same byte with a NUL behind it (the pad byte behind a document's end
  is 0: such a token must not match there); `~` has none (a byte without a token)

The four forms of the issue and the UTF-16 one: FORMS.  For charset 2 every token and every text byte is widened to (byte, 0), tokens have at
most 20 characters and documents an even length: there is then no one-byte key beside the delete token and the non-terminating class of
DESIGN section 7 cannot arise.

Constructs are rows (name, bytes, reason).  Lengths are in CHARACTERS: one byte each for charset 1, two for the UTF-16 form, whose chains are cut
to its 20 characters (lengths() says which stand for which).  The forward-delete tails are not part of this table: they are chosen by asking the
oracle (fd_tails()), because whether a tail sends the walk through a forward-delete state hangs on the scores of the vocabulary."""
import ctypes as C

import numpy as np

import conftest
from oracle_bind import oracle_stats
from tokenmonster_amd import synth

SEG, NPOS, TEXT_LEN, LOOK = 256, 296, 352, 40      # a segment, the positions a wavefront that shares nothing walks, the staged bytes, the longest token
TAIL_TASKS, SIDE_STRIDE, DEFER = 77, 16, 12
FORMS = ["capcode0", "capcode2", "capcode2-nounk", "capcode2-wide", "utf16"]
FILL = b"x"
MISSING = b"~"

HEADS = b"fghijlnopqrstuvwxyz" + b"023456789" + b"-+*/=<>()"      # 37 head bytes: the chain of n characters has HEADS[n - 4]
BODY = b"ghijlnopqrstuvw"
BODY2 = BODY[::-1]
assert len(HEADS) == 37 and len(set(HEADS)) == 37


def _cyc(pattern, n):
    return (pattern * (n // len(pattern) + 1))[:n]


def chain(n, sign=False):
    """the one-child chain of n characters: family `k` ends in a letter, family `f` in a sign"""
    h = HEADS[n - 4:n - 3]
    return b"f" + h + _cyc(BODY2, n - 3) + b";" if sign else b"k" + h + _cyc(BODY, n - 2)


def widen(b):
    return bytes(x for ch in b for x in (ch, 0))


def form_props(form):
    """-> (capcode, charset, with_unk, wide, longest token in characters)"""
    return (0 if form == "capcode0" else 2, 2 if form == "utf16" else 1, form != "capcode2-nounk", form == "capcode2-wide", 20 if form == "utf16" else 40)


def lengths(maxchars):
    """the chain lengths of the constructs: below the minimum, the two halves of the record, the record and probes behind it.  In the UTF-16 form
    a character is two bytes: 8 and 9 characters are the 16 | 17 bytes of the first half, 16 and 17 (cut: 20 is the longest) the 32 | 33"""
    return [4, 5, 16, 17, 31, 32, 33, 40] if maxchars == 40 else [4, 5, 8, 9, 15, 16, 17, 20]


MID = b"kk" + _cyc(BODY, 38)
BRANCH = b"km" + _cyc(BODY, 35)
LOOKC = b"k " + _cyc(BODY, 38)      # with LOOKC[1:] + `;` a token too: `k` and that token beat the greedy LOOKC only while the token at `;` is one byte long
WORDS = [b" ghi jln", b" ghi jln opq", b" ghi", b"ghi", b" jln", b"jln", b" opq"]


def extra_tokens(maxchars):
    """the tokens beside the fuzz vocabulary, in bytes of charset 1 (at most maxchars long)"""
    t = []
    for n in range(4, maxchars + 1):
        for sign in (False, True):
            t.append(chain(n, sign))
            if n >= 5:
                t.append(chain(n, sign)[1:])
    t += [b"m" * k for k in range(1, 21)]
    mid = MID[:maxchars]
    t += [mid, mid[:10], mid[:maxchars * 5 // 8], mid[1:]]
    br = BRANCH[:maxchars - 3]
    t += [br + b"rst", br + b"uvw", (br + b"rst")[1:]]
    sx = chain(min(33, maxchars))
    t += [sx[1:-1] + b"@", (sx[1:-1] + b"@gh")[:maxchars]]
    zl, yl = maxchars, min(33, maxchars - 3)
    t += [b"z" * zl, b"zz", b"zzz", b"y" * yl, b"yy"]
    t += WORDS
    look = LOOKC[:maxchars]
    t += [look, look[1:] + b";"]
    used = set(b"".join(t)) | set(FILL) | set(b"abcde .,1_\nxyz@;!")
    assert MISSING[0] not in used
    t += [bytes([c]) for c in sorted(used)]
    # ... and each of those bytes with a NUL behind it: at the last byte of a document the two-byte direct map reads the pad byte, which is 0 - the
    # token must not match there (tail_here: that byte goes through root[]), and does match where the text really holds a NUL (fuzz_text has some)
    t += [bytes([c, 0]) for c in sorted(used)]
    assert all(len(x) <= maxchars for x in t)
    return t


def tokens(form, seed=5):
    """the vocabulary of a form -> (token list, capcode, charset, with_unk)"""
    capcode, charset, unk, wide, maxchars = form_props(form)
    rng = np.random.default_rng(seed)
    toks = conftest.fuzz_vocab_tokens(rng, capcode, 200)
    if capcode == 2:
        toks = toks + [b"D", b"C", b"W"]
    toks = list(dict.fromkeys([t for t in toks if len(t) <= maxchars] + extra_tokens(maxchars)))
    if charset == 2:
        toks = [widen(t) for t in toks]
        if capcode == 2 and b"D" not in toks:
            toks.append(b"D")
    if wide:      # more than 65 536 ids, as test_walk_with_an_id_per_byte_and_more pads: tokens no text here holds
        toks += [bytes([0x7F, 0x30 + k % 40, 0x30 + (k // 40) % 40, 0x30 + k // 1600]) for k in range(66_000)]
    return toks, capcode, charset, unk


def image(form, norm_flag=0):
    toks, capcode, charset, unk = tokens(form)
    return synth.build_vocab(toks, capcode=capcode, charset=charset, norm_flag=norm_flag, with_unk=unk)


# ---- the constructs ----------------------------------------------------------------------------------------------------------------------------------
class Construct:
    __slots__ = ("name", "data", "why")

    def __init__(self, name, data, why):
        self.name, self.data, self.why = name, data, why

    def __repr__(self):
        return "Construct(%s)" % self.name


def _fd_run(fd_word, n):
    """n forward-delete triggers in a row, a sign between them"""
    return b"".join(b"." + fd_word for _ in range(n))


def constructs(form, fd_word=None):
    """the rows of a form; fd_word: a tail fd_tails() found (the row of 16 and more forward-delete states is made of it).  Bytes of charset 1:
    place() widens them for the UTF-16 form"""
    capcode, charset, unk, wide, maxchars = form_props(form)
    L = lengths(maxchars)
    rows = [
        ("1 byte", b"g", "root[]: a one-byte token"),
        ("2 bytes", b"yy", "the direct map"),
        ("3 bytes", b"zzz", "the first suffix link"),
    ]
    for d in (11, 12, 13, 20) if charset == 1 else (5, 6, 7, 10, 20):
        rows.append(("depth %d" % d, b"m" * d, "every node accepts: kept in the loop below depth 12, handed over at DEFER"))
    why = ["below the minimum: probes only", "the shortest chain record", "the first half of the record, whole", "one byte into the second half",
           "one short of the record", "the record, whole", "the record and a probe behind it", "the longest token: record plus probes"]
    for n, y in zip(L, why):
        rows.append(("chain %d" % n, chain(n), y))
    for n in (L[1], L[3], L[6], L[7]):
        rows.append(("chain %d;" % n, chain(n, True), "... ending in a sign"))
    big, top = chain(L[6]), chain(L[7])
    rows += [
        ("chain broken at its last byte", big[:-1] + b"@", "the record matches up to its last byte: the walk falls back to `k`; the suffix goes on with `@`: entered through a suffix link"),
        ("chain broken at byte 1", big[:1] + b"." + big[2:], "the direct map misses: every byte behind it is a position of its own"),
        ("mid-chain key, then a mismatch", MID[:maxchars * 5 // 8 + 2] + b"!", "the key at 5/8 of the chain is the match, two bytes deeper the text leaves the chain"),
        ("chain through a suffix link", b"m" + top[1:], "the chain without its first byte, behind a byte that matches on its own"),
        ("branch three bytes before the end", BRANCH[:maxchars - 3] + b"uvw", "a chain that ends in a node with two children"),
        ("two longest tokens back to back", top + chain(L[7], True), "the second is the look-ahead of the first: the far end of the staged text"),
        ("look-ahead at the document's last byte decides", LOOKC[:maxchars] + b";", "greedy, or `k` and the rest: the look-ahead at `;` decides, and `;` + NUL is a token - with nothing behind it the pad byte must not make it match"),
        ("two all-letter longest tokens back to back", BRANCH[:maxchars - 3] + b"uvw" + MID[:maxchars], "as the pair above, of letters only: what the capcode normalizer leaves as it is (the raw path)"),
        ("multi-word", b" ghi jln opq", "tokens of one, two and three words on one path"),
        ("a byte without a token", b"g" + MISSING + b"g", "missing: the unk id, or no id at all"),
        ("80 chain heads", b"z" * (80 + maxchars), "more chain heads than the task list holds: the redo bitmap"),
    ]
    if capcode == 2 and fd_word:
        rows.append(("18 forward-delete states", _fd_run(fd_word, 18), "more than SIDE_STRIDE - 1 in one segment: the dense array"))
        rows.append(("15 forward-delete states", _fd_run(fd_word, 15), "the side list, full"))
    out = [Construct(*r) for r in rows]
    assert len({c.name for c in out}) == len(out)
    return out


# ---- the oracle, called without an allocation per document -------------------------------------------------------------------------------------------
class Fast:
    """Oracle.tokenize / count / score for many short documents: the same C entries (oracle_bind.Oracle binds them), buffers reused"""

    def __init__(self, orc):
        self.orc = orc
        self.out = np.empty(4096, dtype=np.uint32)
        self.miss = C.c_longlong()
        self.scores = np.zeros(orc.n_ids(), dtype=np.uint32)
        self.tit = C.c_uint64(0)
        self.ms = np.zeros(32, dtype=np.uint8)

    def _buf(self, doc):
        d = np.frombuffer(doc, dtype=np.uint8)
        if 2 * d.size + 8 > self.out.size:
            self.out = np.empty(2 * d.size + 8, dtype=np.uint32)
        return d

    def tokenize(self, doc):
        """-> (ids, missing, count, missing of count)"""
        d = self._buf(doc)
        L, h = self.orc.L, self.orc.h
        n = L.tmo_tokenize(h, d.ctypes.data, d.size, self.out.ctypes.data, self.out.size, C.byref(self.miss))
        ids, miss = self.out[:n].copy(), self.miss.value
        cnt = L.tmo_count(h, d.ctypes.data, d.size, C.byref(self.miss))
        return ids, miss, int(cnt), self.miss.value

    def score(self, doc):
        """accumulates like Oracle.score -> (tokens in text, missing set) of THIS document"""
        d = np.frombuffer(doc, dtype=np.uint8)
        tit, ms = C.c_uint64(0), np.zeros(32, dtype=np.uint8)
        self.orc.L.tmo_score(self.orc.h, d.ctypes.data, d.size, self.scores.ctypes.data, C.byref(tit), ms.ctypes.data)
        return tit.value, ms


def fd_branches(orc, doc):
    """how many forward-delete branches the oracle's walk over doc takes"""
    oracle_stats(reset=True)
    orc.tokenize(doc)
    st = oracle_stats()
    return st["s1b"] + st["s2b"] + st["s3b"]


def fd_tails(orc, form, want=3):
    """Tails that send the walk through a forward-delete state, CHOSEN BY ASKING THE ORACLE: the candidates are the words of the fuzz vocabulary's
    ' word' tokens without their space, bare and with a sign or a space behind them; kept are the first `want` that trigger behind a one-byte
    token, behind the longest chain of either family and behind the deepest all-accepting path.  (charset-1 bytes; [] for capcode 0)"""
    toks, capcode, charset, unk = tokens(form)
    if capcode != 2:
        return []
    maxchars = form_props(form)[4]
    w = (lambda b: widen(b)) if charset == 2 else (lambda b: b)
    narrow = [bytes(t[::2]) if charset == 2 else t for t in toks[:400]]
    cands = []
    for t in narrow:
        if len(t) > 2 and t[:1] == b" " and all(c in b"abcde" for c in t[1:]):
            cands += [t[1:] + b".", t[1:] + b" ", t[1:]]
    fronts = [b"g", chain(maxchars), chain(maxchars, True), b"m" * 20, b"."]
    out = []
    for cand in sorted(dict.fromkeys(cands), key=len):      # (the shortest first: eighteen of them fit a segment of the UTF-16 form)
        if all(fd_branches(orc, w(FILL * 4 + f + cand)) > fd_branches(orc, w(FILL * 4 + f)) for f in fronts):
            out.append(cand)
            if len(out) == want:
                break
    return out


# ---- the seams ----------------------------------------------------------------------------------------------------------------------------------------
def fillers(form, orc=None, seed=77):
    """-> {kind: bytes of at least 3 * SEG}: a one-byte token repeated (the construct begins on a token boundary), and fuzz_text - of the first
    seed from 77 on at which the oracle's walk over its first 200 bytes (every construct of at most 40 bytes has that much filler in front) takes every exit the form has (oracle_bind.STAT_NAMES; the plain ones for capcode 0):
    asked of the oracle, as the tails are"""
    capcode, charset = form_props(form)[:2]
    want = [k for k in ("s1", "s2", "s3", "s1b", "s2b", "s3b", "fast_exit", "no_lookahead_match", "not_found") if capcode == 2 or not k.endswith("b")]
    for sd in range(seed, seed + 200):
        fz = conftest.fuzz_text(np.random.default_rng(sd), capcode, 3 * SEG + 8)
        if orc is None:
            break
        oracle_stats(reset=True)
        orc.tokenize(widen(fz[:100]) if charset == 2 else fz[:200])
        st = oracle_stats()
        if all(st[k] > 0 for k in want):
            break
    else:
        raise AssertionError("no fuzz_text of 200 seeds takes every exit of the walk")
    return {"token": FILL * (3 * SEG + 8), "fuzz": fz}


def tails(form, fd, seed=78):
    """the short list: nothing, a forward-delete trigger (capcode 2), a one-byte token, a space, 60 bytes of fuzz_text"""
    capcode = form_props(form)[0]
    t = [("nothing", b"")]
    if fd:
        t.append(("forward delete", fd[0]))
    t += [("one byte", b"g"), ("space", b" "), ("fuzz 60", conftest.fuzz_text(np.random.default_rng(seed), capcode, 60))]
    return t


def starts(n, seam=SEG):
    """filler lengths in front of a construct of n characters: from seam - n - 1 to seam + 1"""
    return range(max(seam - n - 1, 0), seam + 2)


def place(form, filler, o, data, tail=b""):
    """filler[:o] + construct + tail, in characters; widened for the UTF-16 form (every seam is then met at o = seam / 2 and at the odd byte
    beside it - a character lies across it)"""
    doc = filler[:o] + data + tail
    return widen(doc) if form == "utf16" else doc


def seam_chars(form, seam=SEG):
    return seam // 2 if form == "utf16" else seam


END_E = [0, 1, 2, 39, 40, 41, 42, 79, 80, 81, 95, 96]


def segments(n):
    return max(1, (n + SEG - 1) // SEG)

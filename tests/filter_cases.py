"""What the device FILTER pass (tm_norm.hip: k_pf_filter, k_pf_long, pf_scan_span, pf_emit_span - the byte-level flags quotemarks 8, collapse 16,
trim 32, leadingspace 64, unixlines 128 and what accents 4 does to the two-byte characters) tells apart, as short byte strings ("constructs")
to be placed at every byte offset across the seams of that kernel, behind a prefix that puts the document in a chosen STATE of its numbers
(PfDoc: first and second single drop, a quote in front of the first, the first and last non-blank byte) and in front of a chosen TAIL:
shared by tests/test_gpu_filter_boundaries.py and its emulated twin.  A helper, no tests.

Each construct carries a one-line reason and a RULE that says under which flags a document that contains it is the HOST normalizer's.  The
rules are what the product documents (tm_norm.hip:762-788, :1084-1086, README.md) and are NOT read off a run of the kernel: the sweep
asserts that the device's count of host documents equals what host_doc() says, exactly.

numbers() is a pure-Python model of the document's numbers, written from the header comment of the filter pass (tm_norm.hip:767-775).  It
is no reference for the kernel's bytes - that is the host normalizer - it only says which quotes the in-place quirk leaves alone, so that
the sweep can prove it is not blind (a document of every kind is in it) and the host rule of trim + leadingspace can be stated."""
import re

ACCENTS, QUOTES, COLLAPSE, TRIM, LEAD, UNIX = 4, 8, 16, 32, 64, 128
FILLER = b"x"
# the 64 combinations of the byte-level flags and accents, in rising order
FLAGS64 = [sum(b for i, b in enumerate((ACCENTS, QUOTES, COLLAPSE, TRIM, LEAD, UNIX)) if m >> i & 1) for m in range(64)]


def _u(s):
    return s.encode("utf-8")


# ---- the rules: flags -> a document that holds the construct is the host's whatever else it holds; and why ---------------------------------------
RULES = {
    "device": (lambda f: False, "stays on the device under every flag set"),
    "malformed": (lambda f: True, "not well-formed UTF-8 whatever the filter pass drops or replaces: the normalizer pass refuses it"),
    "mark3": (lambda f: bool(f & ACCENTS), "a three-byte non-spacing mark: under accents it would have to go, and the filter pass only knows "
                                           "the two-byte characters (tm_norm.hip:1084-1086, :1132)"),
}

# ---- the constructs: (name, bytes, rule, why it is here) --------------------------------------------------------------------------------------------
_TABLE = [
    ("2 spaces", b"  ", "device", "the second goes under collapse: one single drop"),
    ("3 spaces", b"   ", "device", "two single drops in a row: s1 and s2 one byte apart"),
    ("space tab space", b" \t ", "device", "no drop: the byte in front of the second space is a tab"),
    ("CR LF", b"\r\n", "device", "the CR goes under unixlines; with collapse it is a single drop (at the LF)"),
    ("CR CR LF", b"\r\r\n", "device", "only the second CR goes"),
    ("space CR LF", b" \r\n", "device", "a space in front of the pair: not a double space"),
    ("CR LF CR LF", b"\r\n\r\n", "device", "two drops two bytes apart"),
    ("CR", b"\r", "device", "a CR with no LF behind it stays"),
    ("CR space", b"\r ", "device", "... also in front of a space"),
    ("‘", _u("‘"), "device", "E2 80 98 -> '"),
    ("’", _u("’"), "device", "E2 80 99 -> '"),
    ("“", _u("“"), "device", "E2 80 9C -> \""),
    ("”", _u("”"), "device", "E2 80 9D -> \""),
    ("E2 80 94", _u("—"), "device", "an em dash: the third byte is no quote's (pf_isq4 masks with FA)"),
    ("E2 80 9A", _u("‚"), "device", "a low quote: 9A & FA = 9A"),
    ("E2 80 9E", _u("„"), "device", "a low double quote: 9E & FA = 9A"),
    ("E2 81 99", _u("⁙"), "device", "the second byte is not 80"),
    ("E2 80", b"\xe2\x80", "malformed", "two bytes of a quote"),
    ("80 99", b"\x80\x99", "malformed", "the last two bytes of a quote"),
    ("E2 E2 80 99", b"\xe2\xe2\x80\x99", "malformed", "a quote behind a stray E2: replaced or not, the E2 stays"),
    ("E2 83 9D", _u("⃝"), "mark3", "U+20DD, an enclosing mark: begins like a quote, and the one character here that accents leaves to the host"),
    ("’ 2 spaces", _u("’  "), "device", "a quote, then a drop: a quote candidate in front of the drop (qb)"),
    ("2 spaces ’", _u("  ’"), "device", "a drop, then a quote: suppressed when that drop is the document's only one"),
    ("’ CR LF", _u("’\r\n"), "device", "a quote, then the other kind of drop"),
    ("CR LF ’", _u("\r\n’"), "device", "a CR LF in front of a quote: a drop only under 16|128"),
    ("‘’", _u("‘’"), "device", "two quotes in a row: the second and third byte of one, the first of the next in one dword"),
    ("“ ”", _u("“ ”"), "device", "two double quotes a space apart"),
    ("é", _u("é"), "device", "accents leaves one byte, e"),
    ("É", _u("É"), "device", "accents leaves one byte, E"),
    ("ñ", _u("ñ"), "device", "accents leaves one byte, n"),
    ("ß", _u("ß"), "device", "accents leaves it alone"),
    ("U+0301", _u("́"), "device", "a two-byte mark: accents leaves nothing of it"),
    ("й", _u("й"), "device", "accents leaves two OTHER bytes, и (D0 B9 -> D0 B8; checked against the host's remove_marks by the CPU tests)"),
    ("é’", _u("é’"), "device", "a character accents shortens directly in front of a quote"),
    ("é 2 spaces", _u("é  "), "device", "... and in front of a drop"),
]


class Construct:
    __slots__ = ("name", "data", "rule", "why")

    def __init__(self, name, data, rule, why):
        self.name, self.data, self.rule, self.why = name, data, rule, why

    def well_formed(self):
        try:
            self.data.decode("utf-8")
            return True
        except UnicodeDecodeError:
            return False

    def __repr__(self):
        return "Construct(%s)" % self.name


CONSTRUCTS = [Construct(*row) for row in _TABLE]
assert len({c.name for c in CONSTRUCTS}) == len(CONSTRUCTS) and all(c.rule in RULES and c.why for c in CONSTRUCTS)
assert all((c.rule == "malformed") == (not c.well_formed()) for c in CONSTRUCTS)
# the reference runtime's normalize does not go through ICU: what it makes of malformed UTF-8 is not this project's U+FFFD - these stay out of the
# reference-anchor test, and only out of it
REFERENCE_REFUSES = {c.name for c in CONSTRUCTS if not c.well_formed()}


def _fill(pattern, n):
    return (pattern * (n // len(pattern) + 1))[:n] if n > 0 else b""


BLANKS = b" \t\n"      # blanks for the ends of a document that are no drops themselves: no two spaces in a row, no CR LF

# ---- the states: (name, prefix, kind) - what stands at the head of the document --------------------------------------------------------------------
STATES = [
    ("none", b"", "none"),
    ("one drop", b"a  b", "one drop"),
    ("two drops", b"a  b  c", "two drops"),
    ("quote, drop", _u("’a  b"), "quote first"),                 # qb = 1: nothing is suppressed
    ("drop, quote", _u("a  ’b"), "quote suppressed"),           # that quote stays, and so does every quote up to the next drop
    ("CR LF drop", b"a\r\nb", "CR LF drop"),                          # a single drop only under 16|128
] + [("%d blanks" % k, _fill(BLANKS, k), "blanks") for k in (1, 2, 3, 4, 5, 300)]      # a moves, and with it the emit sweep's base; 300: beyond a step
STATE = {s[0]: s for s in STATES}
# one state of every kind, for the documents of more than 16384 bytes (and both ends of the blanks)
STATES_LONG = ["none", "one drop", "two drops", "quote, drop", "drop, quote", "CR LF drop", "3 blanks", "300 blanks"]

# ---- the tails: (name, bytes) - what stands behind the construct ------------------------------------------------------------------------------------
TAILS = [
    ("nothing", b""),
    ("y", b"y"),
    ("drop, quote", _u("c  d’")),                # a second (or first) drop, then a quote as the last non-blank character
    ("1 blank", b" "),
    ("3 blanks", _fill(BLANKS, 3)),
    ("300 blanks", _fill(BLANKS, 300)),               # the backward search for z spans more than one step
    ("y’", _u("y’")),                            # a quote last: replaced (zlo = z - 2) or suppressed (zlo = z), as the state and the construct have it
    ("y’ 3 blanks", _u("y’") + _fill(BLANKS, 3)),
]
TAIL = dict(TAILS)
TAILS_LONG = ["nothing", "y", "drop, quote", "300 blanks", "y’"]      # five, the states above eight: k mod 5 and k mod 8 meet in every pair
BLANK_TAILS = {"1 blank", "3 blanks", "300 blanks"}


def place(construct, seam, start, state, tail, total=0):
    """state prefix + filler up to `start` + construct + tail, or None when the prefix is longer than `start` (seam is what start is measured
    from - it does not change the document, it names the case).  total > 0: padded with filler to `total` bytes - behind the tail, but IN FRONT
    of a tail of blanks, so that those stay the document's last bytes; None when it does not fit."""
    data = construct.data if isinstance(construct, Construct) else construct
    prefix, t = STATE[state][1], TAIL[tail]
    if len(prefix) > start:
        return None
    doc = prefix + FILLER * (start - len(prefix)) + data
    if total:
        pad = total - len(doc) - len(t)
        if pad < 0:
            return None
        return doc + FILLER * pad + t if tail in BLANK_TAILS else doc + t + FILLER * pad
    return doc + t


def starts(n, seam):
    """for a construct of n bytes: every straddling offset, plus one byte clear on either side"""
    return range(max(seam - n - 1, 0), seam + 2)


# ---- the model of the document's numbers -------------------------------------------------------------------------------------------------------------
_QUOTE = re.compile(rb"\xe2\x80[\x98\x99\x9c\x9d]")
_DROP = {False: re.compile(rb"(?<= ) "), True: re.compile(rb"(?<= ) |(?<=\r)\n")}
_NONBLANK = re.compile(rb"[^\x00-\x20]")
_BLANK = bytes(range(33))


class Numbers:
    __slots__ = ("s1", "s2", "fq", "qb", "a", "z", "zlo", "quotes")


def numbers(doc, flags):
    """tm_norm.hip:767-775 in plain words.  s1 / s2: the first and second SINGLE DROP - under collapse a space whose byte in front is a space,
    under collapse + unixlines also an LF whose byte in front is a CR (the reference's fused loop drops one byte there).  fq: the third byte of
    the first quote.  The text has shrunk by exactly ONE byte between s1 and s2 provided no quote was replaced in front of s1 (qb): there the
    in-place look-behind of the reference finds a moved byte and the quote stays - `quotes` is [(position of the third byte, replaced)].
    a / z: the first and last byte above 32; zlo: where the last non-blank OUTPUT byte begins (z - 2 when that is a replaced quote)."""
    r = Numbers()
    r.s1 = r.s2 = r.fq = r.a = r.z = r.zlo = None
    if flags & COLLAPSE:
        it = _DROP[bool(flags & UNIX)].finditer(doc)
        m = next(it, None)
        if m:
            r.s1 = m.start()
            m = next(it, None)
            if m:
                r.s2 = m.start()
    third = [m.start() + 2 for m in _QUOTE.finditer(doc)]
    r.fq = third[0] if third else None
    r.qb = r.fq is not None and (r.s1 is None or r.fq < r.s1)
    r.quotes = [(t, bool(flags & QUOTES) and not (r.s1 is not None and not r.qb and r.s1 < t and (r.s2 is None or t < r.s2))) for t in third]
    m = _NONBLANK.search(doc)
    if m:
        r.a = m.start()
        r.z = len(doc) - 1
        while doc[r.z] <= 32:
            r.z -= 1
        r.zlo = r.z - 2 if r.quotes and r.quotes[-1] == (r.z, True) else r.z
    return r


def host_doc(doc, flags, construct):
    """is this document the host normalizer's under these flags (capcode 2)?  From rules, not from a run:
      * it holds a construct whose rule says so (malformed UTF-8; under accents a three-byte mark), or
      * trim + leadingspace on a text WITHOUT leading blanks cut the last non-blank BYTE as well (tm_norm.hip:774-775): when that byte is the
        end of a character of two or three bytes - a quote that was not replaced among them - half a character is left: malformed, the host's
        (a replaced quote is one byte, ', and goes whole)"""
    if construct is not None and RULES[construct.rule][0](flags):
        return True
    if (flags & (TRIM | LEAD)) == (TRIM | LEAD) and doc and doc[0] > 32:
        last = doc.rstrip(_BLANK)[-3:]
        if last[-1] < 0x80:
            return False
        if not (flags & QUOTES and _QUOTE.fullmatch(last)):
            return True
        r = numbers(doc, flags)
        return r.zlo == r.z
    return False


def expected_quotes(doc, flags):
    """what is left of the quotes of `doc`, in order, as the model has it: ' or " for a replaced one, its three bytes for one left alone"""
    out = []
    for t, replaced in numbers(doc, flags).quotes:
        out.append((b"'" if doc[t] < 0x9C else b'"') if replaced else doc[t - 2:t + 1])
    return out


_LEFT = re.compile(rb"\xe2\x80[\x98\x99\x9c\x9d]|['\"]")


def quotes_left(text):
    """the quotes of a filtered text (no construct, state, tail or filler holds an ASCII quote), in order"""
    return _LEFT.findall(text)

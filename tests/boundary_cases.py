"""Every kind of character the device normalizer (tm_norm.hip) and the device capcode decoder (tm_decode.hip: k_dec_capcode) tell apart, as
short byte strings ("constructs") to be placed at every byte offset across the seams of those kernels: shared by
tests/test_gpu_normalize_boundaries.py, tests/test_gpu_decode_boundaries.py and their emulated twins.  A helper, no tests.

Each construct carries a one-line reason and a RULE that says with which vocabularies a document that contains it is the HOST normalizer's.
The rules are what the product documents - README.md, the docstrings of the *_stays_on_the_device tests (tests/test_gpu_parity.py),
tokenmonster_amd/csrc/tm_norm_masks.h and the table builders of tm_normalize.cpp it points to - and are NOT read off a run of the kernel:
the sweep asserts that the device's count of host documents equals what this table says, exactly.

A document left to the host tests nothing of the kernel, so at most a quarter of the constructs may be the host's under the capcode-2 NFD
vocabulary (checked at import)."""

# ---- the rules: (capcode, normalization flags) -> the document is the host's; and why, in words -----------------------------------------------
NFD, LOWER = 1, 2

RULES = {
    "device": (lambda c, f: False,
               "stays on the device with every vocabulary"),
    "host": (lambda c, f: True,
             "the device's tables have no entry for it (or it is not well-formed UTF-8): the host's with every vocabulary"),
    "splits": (lambda c, f: c == 0 and bool(f & NFD),
               "NFD splits it in two or three characters; without capcode the device pass keeps lengths, so there - and only there - it is the host's"),
    "idot": (lambda c, f: not (c == 2 and bool(f & (NFD | LOWER))),
             "İ without NFD: lower case of another length (i, one byte); with NFD or the lowercase flag it is a letter and a mark, "
             "which the pass takes only with capcode 2 (it changes lengths)"),
    "lea_capital": (lambda c, f: not (c == 2 and bool(f & NFD)),
                    "a three-byte capital: only the NFD table of Latin Extended Additional (capcode 2) takes it; without NFD it is a "
                    "three-byte letter with case, with NFD and no capcode it would change lengths"),
}


def on_host(rule, capcode, flags):
    return RULES[rule][0](capcode, flags)


# ---- the constructs: (name, bytes, rule, the decoder leaves its normalized form to the host, why it is here) ------------------------------------
def _u(s):
    return s.encode("utf-8")


_TABLE = [
    # ASCII capcode shapes
    ("Hello", b"Hello", "device", "one capital, then lower case: 'C' mode"),
    ("HELLO", b"HELLO", "device", "a run of capitals: 'W' mode"),
    ("H", b"H", "device", "a capital alone: what follows it in the filler decides its marker"),
    ("it's", b"it's", "device", "an apostrophe between lower-case letters joins them"),
    ("IT'S", b"IT'S", "device", "an apostrophe inside a run of capitals stays in the block"),
    ("A1B", b"A1B", "device", "a digit inside a block: 'D' in front of the capital behind it"),
    ("2ND", b"2ND", "device", "a block that begins with a digit"),
    ("don’t", _u("don’t"), "device", "U+2019 counts as an apostrophe: three bytes of class AP"),
    ("DON’T", _u("DON’T"), "device", "U+2019 inside a run of capitals"),
    ("…", _u("…"), "device", "general punctuation: three inert bytes of class O"),
    # two-byte characters
    ("ß", _u("ß"), "device", "a lower-case letter without a capital of its length"),
    ("µ", _u("µ"), "device", "a lower-case letter whose capital is in another script"),
    ("Ж", _u("Ж"), "device", "a two-byte capital: both bytes replaced from the table"),
    ("ЖУК", _u("ЖУК"), "device", "a run of two-byte capitals"),
    ("ǅ", _u("ǅ"), "device", "a title-case letter: a letter that is neither upper nor lower case"),
    ("é", _u("é"), "splits", "NFD: an ASCII letter and a two-byte mark, three bytes from two"),
    ("É", _u("É"), "splits", "the same with a marker in front"),
    ("ÉTÉ", _u("ÉTÉ"), "splits", "a run of capitals with two decomposing ones"),
    ("й", _u("й"), "splits", "NFD: a two-byte letter and a two-byte mark"),
    ("Й", _u("Й"), "splits", "the same, a capital"),
    ("ά", _u("ά"), "splits", "Greek: a two-byte letter and a two-byte mark"),
    ("ÿ", _u("ÿ"), "splits", "the last character of Latin-1"),
    ("Ÿ", _u("Ÿ"), "splits", "its capital lies in another lead byte's row of the table"),
    ("İ", _u("İ"), "idot", "a capital whose lower case has another length"),
    # Latin Extended Additional
    ("Ḁ", _u("Ḁ"), "lea_capital", "a letter and one mark, a capital"),
    ("ḁ", _u("ḁ"), "splits", "a letter and one mark: the third lane emits nothing"),
    ("ế", _u("ế"), "splits", "a letter and two marks: five bytes from three"),
    ("Ế", _u("Ế"), "lea_capital", "a capital and two marks"),
    ("ớ", _u("ớ"), "splits", "a letter, the horn and a mark above"),
    # three-byte characters
    ("世", _u("世"), "device", "an ideograph: a letter without case, inert"),
    ("の", _u("の"), "device", "a kana that NFD leaves alone"),
    ("が", _u("が"), "splits", "a voiced kana: the kana and U+3099, six bytes from three"),
    ("ヴ", _u("ヴ"), "splits", "a voiced katakana"),
    ("パ", _u("パ"), "splits", "a semi-voiced katakana: U+309A"),
    ("가", _u("가"), "splits", "a Hangul syllable of two jamo: the third lane emits nothing"),
    ("한", _u("한"), "splits", "a Hangul syllable of three jamo: nine bytes from three"),
    ("값", _u("값"), "splits", "a Hangul syllable with a double final consonant"),
    ("Thai tone", _u("\u0e01\u0e48\u0e33"), "device", "ก่ำ: a Thai tone mark of canonical class 107 between two letters"),
    ("Devanagari vowel", _u("\u0915\u093f"), "device", "कि: a spacing vowel sign, a mark of class 0"),
    ("nukta virama", _u("\u0958\u094d"), "splits", "U+0958 U+094D: a nukta letter as one code point and a virama behind it - the classes 7 and 9 are in order"),
    ("Bengali vowel", _u("\u0995\u09cb"), "splits", "U+0995 U+09CB: a two-part vowel sign, a mark NFD splits in two marks"),
    # four-byte characters and sequences
    ("😀", _u("😀"), "device", "an emoji: four inert bytes"),
    ("thumb+tone", _u("\U0001f44d\U0001f3fd"), "device", "👍🏽: an emoji and a skin-tone modifier, eight bytes"),
    ("flag", _u("\U0001f1f0\U0001f1f7"), "device", "🇰🇷: two regional indicators"),
    ("heart+FE0F", _u("\u2764\ufe0f"), "device", "❤️: a three-byte symbol and the variation selector U+FE0F, a mark of class 0"),
    ("keycap", _u("1\ufe0f\u20e3"), "device", "1️⃣: a digit, U+FE0F and the enclosing keycap - marks behind a digit"),
    ("𠮷", _u("𠮷"), "device", "an ideograph of plane 2: a four-byte letter without case"),
    # pre-decomposed input
    ("e+0301", _u("e\u0301"), "device", "a letter and its mark already apart"),
    ("e+0323+0301", _u("e\u0323\u0301"), "host", "two two-byte marks in a row, in order: the device does not know their classes"),
    ("e+0301+0323", _u("e\u0301\u0323"), "host", "two marks that must change places"),
    ("A+030A", _u("A\u030a"), "device", "a capital and a mark that NFD does not compose"),
    # characters known to need the host
    ("ẞ", _u("ẞ"), "host", "a three-byte capital without a decomposition, lower case of two bytes"),
    ("Ａ", _u("Ａ"), "host", "a fullwidth capital: a three-byte letter with case"),
    ("𐐀", _u("𐐀"), "host", "a Deseret capital: a four-byte letter with case"),
    # malformed UTF-8
    ("80", b"\x80", "host", "a continuation byte alone"),
    ("C3", b"\xc3", "host", "a lead byte with nothing behind it"),
    ("E4 B8", b"\xe4\xb8", "host", "two of three bytes"),
    ("F0 9F 98", b"\xf0\x9f\x98", "host", "three of four bytes"),
    ("C0 AF", b"\xc0\xaf", "host", "an overlong form"),
    ("ED A0 80", b"\xed\xa0\x80", "host", "a surrogate"),
    ("F4 90 80 80", b"\xf4\x90\x80\x80", "host", "beyond U+10FFFF"),
    ("FF", b"\xff", "host", "a byte no UTF-8 has"),
]


class Construct:
    __slots__ = ("name", "data", "rule", "why")

    def __init__(self, name, data, rule, why):
        self.name, self.data, self.rule, self.why = name, data, rule, why

    def host(self, capcode, flags):
        return on_host(self.rule, capcode, flags)

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
# a document left to the host tests nothing of the kernel
assert 4 * sum(c.host(2, NFD) for c in CONSTRUCTS) <= len(CONSTRUCTS), "more than a quarter of the constructs are the host's under capcode 2 + NFD"

# The reference runtime's normalize replaces nothing in malformed UTF-8 where this project's host normalizer goes through ICU (U+FFFD): the
# malformed constructs stay out of the reference-anchor test (tests/test_normalize_boundaries_emulated.py) and only out of it.
REFERENCE_REFUSES = {c.name for c in CONSTRUCTS if not c.well_formed()}

# What the device DECODER leaves to the host decoder, of the NFD capcode-2 normalized form of a construct (tm_decode.hip: "a three- or four-byte
# letter with case, and any byte sequence that is not well-formed UTF-8"): the host normalizer turns malformed bytes into U+FFFD, a character
# the decoder passes on, and Latin Extended Additional into ASCII letters and marks, so what is left is
DECODER_HOST = {"Ａ": "lower-cased by capcode to U+FF41, a three-byte letter with case",
                "𐐀": "lower-cased by capcode to U+10428, a four-byte letter with case"}
# ... and what does not come back as NFD of the raw text from normalize -> tokenize -> decode (the decoder's reference for the well-formed ones)
NO_ROUND_TRIP = {"ẞ": "capcode lower-cases it to ß, whose capital is not ẞ"}

# ---- the fillers: what carries state across a seam -------------------------------------------------------------------------------------------------
FILLERS = {
    "lower": (b"x", b"y"),                   # lower case: nothing carried
    "capital": (b"Q", b"R"),                 # the capital run is carried, with ub / ua above and below 64
    "digit": (b"7", b"3"),                   # a block without a capital
    "space": (b" ", b" "),                   # every space may become a marker
    "mixed": (b"xQ 7'", b"Zz 1'"),           # every class within five bytes: a piece of it normalizes to 2049 bytes, one more than its slab
    "words": (b"the Quick 7th fox's IT ", b"Lazy dog 42 it's OK "),      # every class as running text: no 64 block bytes in a row, no piece that doubles
    # one block of capitals and digits from end to end, a capital every 67 bytes: whether a piece's first byte is inside a word, and how the
    # block at its end ends, then hangs on the one byte at the far edge of a 64-byte margin; behind the construct 66 digits and a capital
    # that is a run's first letter or a later one ('W' mode: the two are written differently)
    "block": (b"Q" + b"7" * 66, b"3" * 66 + b"Q "),
}


def _fill(pattern, n):
    return (pattern * (n // len(pattern) + 1))[:n] if n > 0 else b""


def place(construct, seam, start, filler, tail):
    """filler[:start] + construct + filler2[:tail]: the construct's first byte is byte `start` of the document (seam is what start is measured from - it
    does not change the document, it names the case)"""
    data = construct.data if isinstance(construct, Construct) else construct
    before, after = FILLERS[filler]
    return _fill(before, start) + data + _fill(after, tail)


def starts(n, seam):
    """for a construct of n bytes: every straddling offset, plus one byte clear on either side"""
    return range(max(seam - n - 1, 0), seam + 2)

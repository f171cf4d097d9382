"""CPU: tm_normalize_origins - the host normalizer with the owner of every byte it writes (tokenmonster_amd/csrc/tm_normalize.cpp) - against
the sequential model of tests/origin_recipe.py where the model applies (NFD, lowercase, capcode 0 / 2), against vectors worked by hand for the
other flags and for marks NFD reorders, and by its properties over random documents for every flag set the normalizer takes."""
import ctypes as C

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository on sys.path)
import origin_recipe as R
from tokenmonster_amd import _native as N, synth


def origins(data, capcode, flag):
    d = N.as_u8(data)
    out, own, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    N.check(N.lib.tm_normalize_origins(N.ptr(d), d.size, capcode, flag, C.byref(out), C.byref(n), C.byref(own)))
    o = np.frombuffer(C.string_at(own.value, 4 * n.value), dtype=np.uint32).astype(np.int64) if n.value else np.zeros(0, dtype=np.int64)
    N.lib.tm_free(own)
    return N.take(out, n.value), o


# characters whose properties are old and stable: ASCII, Latin-1, Latin Extended-A and Additional, Greek without the final sigma, Cyrillic,
# General Punctuation, Hangul, kana with voiced forms, Devanagari and Thai with their marks in canonical order
DOCS = [s.encode("utf-8") for s in [
    "",
    "Hello", "HELLO", "HEllo", "A1b", "it's", "IT'S", "It’s", "IT’S ok",
    "Hello World", "hello World", "say HELLO there", "a HEllo b", "x.Hello", "x.HELLO!", "(HEllo)", "7Up", "7UP", "7up 7 UP",
    "A", "a", "AB", "Ab", "aB", "ABc", "ABC d", "A b", "A B C", " A", " Ab", " AB ", "  AB", "A1B2c", "A1 B", "AB'Cd", "AB1c", "USA's", "McDonald's BIG Mac",
    "the quick brown fox", "The Quick BROWN fOX 123 go2 4U", "e.g. This, That; THOSE: x'Y",
    "1a 1A a1 A1 11 1 a", "don't DON'T Don't dON'T", "'Tis 'TIS", "a'b'c A'B'C",
    "É", "é", "Éa", "ÉCOLE école École", "Ärger ÄRGER ärger", "naïve NAÏVE Naïve", "Łódź ŁÓDŹ", "Ĉu ĈU", "ÿ Ÿ",
    "Ấn ẤN ấn Ệ ệ", "Αθήνα ΑΘΉΝΑ αθήνα Άλφα", "Москва МОСКВА москва Ёж ёж ЙОД йод",
    "한국어 한 HELLO 한글 가 각", "がぎぐ ガギグ パピプ ぱ か", "हिन्दी की कि", "ภาษาไทย น้ำ", "mixed 한A가B ÉÉé Ёё 12",
    "— “quoted” ‘single’ … ok", "It’S", "A’B c", "Ab’C",
    "A" * 70 + "b", "A" * 70 + " b", "9" * 70 + "A", "a" + "B" * 5 + "c" + "D" * 3,
]]
SETS = [(0, 0), (0, 1), (0, 2), (0, 3), (2, 0), (2, 1), (2, 2), (2, 3)]


@pytest.mark.parametrize("capcode,flag", SETS)
def test_the_model_and_the_library_agree(capcode, flag):
    for doc in DOCS:
        plain = synth.normalize(doc, capcode, flag)
        mb, mo = R.normalize_with_owners(doc, capcode, flag)
        assert mb == plain, "the model's bytes differ from tm_normalize on %r (capcode %d, flags %d)" % (doc, capcode, flag)
        gb, go = origins(doc, capcode, flag)
        assert gb == plain, (doc, capcode, flag)
        assert go.tolist() == mo.tolist(), "owners of %r (capcode %d, flags %d): %s, the model says %s" % (doc, capcode, flag, go.tolist(), mo.tolist())


def test_owners_of_the_markers_by_hand():
    # "Hello": D W ␣ h are the H's, the rest their own
    b, o = origins(b"Hello", 2, 0)
    assert b == b"DC hello" and o.tolist() == [0, 0, 0, 0, 1, 2, 3, 4]
    # (a lower-case letter at the document's start has its "D " too) a space before a capital: the W over the space is the space's, the space behind it the capital's
    b, o = origins(b"a HI", 2, 0)
    assert b == b"D aW hi" and o.tolist() == [0, 0, 0, 1, 2, 2, 3]
    # "HEllo": the run's later capital gets its "DC " after the fact (mark_run_letters)
    b, o = origins(b"HEllo", 2, 0)
    assert b == b"DC hDC ello" and o.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 3, 4]
    # without capcode and flags nothing moves
    b, o = origins("aé한".encode(), 0, 0)
    assert b == "aé한".encode() and o.tolist() == [0, 1, 1, 3, 3, 3]
    # Hangul under NFD: three jamo, all the syllable's
    b, o = origins("a각".encode(), 0, 1)
    assert b == "a\u1100\u1161\u11a8".encode() and o.tolist() == [0] + [1] * 9


# (flags, raw, normalized, owners): worked by hand from the definition (include/tm_build.h)
HAND = [
    (4, "é x".encode(), b"e x", [0, 2, 3]),                                       # accents: the mark goes, the letter is the character's
    (8, "a’b".encode(), b"a'b", [0, 1, 4]),                                       # quotemarks: three bytes to one
    (16, b"a   b", b"a b", [0, 1, 4]),                                            # collapse: the first space stays
    (24, "a  ’b".encode(), "a ’b".encode(), [0, 1, 3, 3, 3, 6]),                  # ... and the in-place quirk: after ONE dropped byte the quote is left alone
    (24, "a   ’b".encode(), b"a 'b", [0, 1, 4, 7]),                               # (after two it is replaced)
    (32, b"  ab \n", b"ab", [2, 3]),                                              # trim
    (64, b"ab", b" ab", [0, 0, 1]),                                               # leadingspace: the invented space is the first unit's
    (64, b" ab", b" ab", [0, 1, 2]),
    (96, b"\t ab  ", b" ab", [1, 2, 3]),                                          # trim + leadingspace: a blank of the document becomes the space
    (96, b"ab c", b" ab ", [0, 0, 1, 2]),                                         # ... and without one the last non-blank byte goes too
    (128, b"a\r\nb", b"a\nb", [0, 2, 3]),                                         # unixlines: the '\r' goes
    (144, b"a \r\nb  c", b"a \nb c", [0, 1, 3, 4, 5, 7]),                         # unixlines + collapse, the fused loop
    (1, "a\u0301\u0323".encode(), "a\u0323\u0301".encode(), [0, 0, 0, 0, 0]),                # two marks NFD swaps: one unit from the letter on
    (1, "xa\u0301\u0323y".encode(), "xa\u0323\u0301y".encode(), [0, 1, 1, 1, 1, 1, 6]),
    (1, "a\u0323\u0301".encode(), "a\u0323\u0301".encode(), [0, 1, 1, 3, 3]),                # in canonical order already: every character its own
]


@pytest.mark.parametrize("k", range(len(HAND)))
def test_hand_worked_vectors(k):
    flag, raw, norm, own = HAND[k]
    assert synth.normalize(raw, 0, flag) == norm, "the vector itself: tm_normalize gives %r" % synth.normalize(raw, 0, flag)
    b, o = origins(raw, 0, flag)
    assert b == norm and o.tolist() == own, (b, o.tolist())


def test_hand_worked_vector_with_capcode_behind_a_filter():
    # collapse + capcode 2: the dropped space falls to the span in front; the W is the kept space's, "␣h" the H's
    b, o = origins(b"a  Hi", 2, 16)
    assert b == synth.normalize(b"a  Hi", 2, 16) == b"D aC hi" and o.tolist() == [0, 0, 0, 1, 3, 3, 4]


def _char_starts(raw):
    """offsets at which a unit may begin: the first byte of a well-formed sequence, or a byte that belongs to none"""
    ok = np.ones(len(raw), dtype=bool)
    i = 0
    while i < len(raw):
        for n in (4, 3, 2):
            try:
                if len(raw[i:i + n].decode("utf-8")) == 1:
                    ok[i + 1:i + n] = False
                    i += n - 1
                    break
            except UnicodeDecodeError:
                pass
        i += 1
    return ok


ALPHABET = [c.encode("utf-8") for c in "aaabcdeXYZQ  \t\r\n\n.,'’‘“”019éÉüßñŁấỆΑλжЁ한각がガｶ้่̣́̀日🙂—"] + [b"\xff", b"\xc3", b"\xe2\x80", b"\r\n", b"  ", b"   "]
def check_properties(raw, capcode, flag):
    b, o = origins(raw, capcode, flag)
    assert b == synth.normalize(raw, capcode, flag), (raw, capcode, flag)
    assert o.size == len(b)
    if o.size:
        assert (np.diff(o) >= 0).all(), (raw, capcode, flag, o.tolist())
        assert o.min() >= 0 and o.max() < len(raw), (raw, capcode, flag, o.tolist())
        assert _char_starts(raw)[o].all(), (raw, capcode, flag, o.tolist())


@pytest.mark.parametrize("capcode", [0, 2])
def test_properties_over_random_documents(capcode):
    """every flag set the normalizer takes: bytes equal tm_normalize's, owners never decrease, every owner a character start inside the document"""
    rng = np.random.default_rng(1000 + capcode)
    for flag in range(256):
        for _ in range(12):
            n = int(rng.integers(0, 40))
            check_properties(b"".join(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), size=n)), capcode, flag)
    for flag in (0, 1, 3, 7, 24, 96, 144, 255):          # and longer ones
        for _ in range(20):
            n = int(rng.integers(100, 600))
            check_properties(b"".join(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), size=n)), capcode, flag)


def test_refused_arguments():
    out, own, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    d = N.as_u8(b"abc")
    assert N.lib.tm_normalize_origins(N.ptr(d), 3, 1, 0, C.byref(out), C.byref(n), C.byref(own)) == N.TM_E_INVALID      # capcode 1 has no statement
    assert N.lib.tm_normalize_origins(N.ptr(d), 3, 2, 0, None, C.byref(n), C.byref(own)) == N.TM_E_INVALID

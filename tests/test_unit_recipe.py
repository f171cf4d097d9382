"""CPU: the unit rule of include/tokenmonster_hip.h.  tests/unit_recipe.py (numpy) against Python's codecs on well-formed text, and
tm_utf8_units (tokenmonster_amd/csrc/tm_normalize.cpp, the host statement of the rule) against the recipe at EVERY offset of well-formed and
malformed documents."""
import numpy as np
import pytest

import unit_recipe as UR
from tokenmonster_amd import _native as N

WELL_FORMED = [
    "plain ascii",
    "é",
    "a é Ω я ế あが 한 😀 z",                       # 1-, 2-, 3- and 4-byte characters
    "😀😀é한a" * 7,
    "ạ́ NFD: é ế が",                    # combining marks are characters of their own
    "\U0001F642é한" + "x" * 300 + "\U0001F600",
]
MALFORMED = [
    b"\x80abc",                            # a lone continuation byte at the start
    b"ab\x80\x80\x80\x80cd \x80\x80\x80\x80",      # four continuation bytes in a row
    b"abc\xe3",                            # a lead byte at the end
    b"ab\xf8cd\xf8\x80\x80\x80\x80",        # 0xF8
    b"",                                   # the empty document
    b"\x80", b"\x80\x80\x80\x80\x80", b"\xf0\x9f", b"\xff\xfe\xc3",
]


def lib_units(doc, unit, x, round_down):
    d = N.as_u8(doc)
    return int(N.lib.tm_utf8_units(N.ptr(d) if d.size else None, d.size, unit, x, round_down))


@pytest.mark.parametrize("text", WELL_FORMED)
def test_recipe_equals_pythons_codecs_at_character_boundaries(text):
    raw = text.encode("utf-8")
    cp, u16 = UR.U_table(raw, UR.CODEPOINTS), UR.U_table(raw, UR.UTF16)
    dcp, du16 = UR.D_table(raw, UR.CODEPOINTS), UR.D_table(raw, UR.UTF16)
    boundaries = [x for x in range(len(raw) + 1) if x == len(raw) or (raw[x] & 0xC0) != 0x80]
    assert len(boundaries) == len(text) + 1
    for x in boundaries:
        assert cp[x] == dcp[x] == len(raw[:x].decode())
        assert u16[x] == du16[x] == len(raw[:x].decode().encode("utf-16-le")) // 2
    # inside a character: D rounds down to the character's begin, U has counted the character
    for x in set(range(len(raw) + 1)) - set(boundaries):
        lo = max(b for b in boundaries if b < x)
        assert dcp[x] == cp[lo] and cp[x] == cp[lo] + 1 and du16[x] == u16[lo]
    sizes = {len(c.encode()) for c in "".join(WELL_FORMED)}
    assert sizes == {1, 2, 3, 4}


@pytest.mark.parametrize("k", range(len(WELL_FORMED) + len(MALFORMED)))
def test_tm_utf8_units_equals_the_recipe_at_every_offset(k):
    raw = (WELL_FORMED[k].encode("utf-8") if k < len(WELL_FORMED) else MALFORMED[k - len(WELL_FORMED)])
    for unit in (UR.BYTES, UR.CODEPOINTS, UR.UTF16):
        U, D = UR.U_table(raw, unit), UR.D_table(raw, unit)
        for x in range(len(raw) + 1):
            assert lib_units(raw, unit, x, 0) == U[x], (unit, x)
            assert lib_units(raw, unit, x, 1) == D[x], (unit, x)


def test_the_rule_on_malformed_text_by_hand():
    # every non-continuation byte is one unit; a continuation byte with no non-continuation byte within three in front of it stays where it is
    assert UR.U_table(b"\x80abc", UR.CODEPOINTS).tolist() == [0, 0, 1, 2, 3]
    assert UR.char_start_table(b"\x80abc").tolist() == [0, 1, 2, 3, 4]
    assert UR.char_start_table(b"ab\x80\x80\x80\x80c").tolist() == [0, 1, 1, 1, 1, 5, 6, 7]
    assert UR.U_table(b"a\xf8\x80", UR.UTF16).tolist() == [0, 1, 3, 3]
    assert UR.convert([[0, 0], [1, 3], [2, 2]], "aé".encode(), UR.CODEPOINTS).tolist() == [[0, 0], [1, 2], [1, 1]]
    assert lib_units(b"abc", 3, 1, 0) == 2 ** 64 - 1 and lib_units(b"abc", UR.CODEPOINTS, 99, 0) == 3

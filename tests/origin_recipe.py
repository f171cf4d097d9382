"""A plain sequential model of the normalizer WITH OWNERS, for the flag sets inside {NFD 1, lowercase 2} and capcode 0 / 2 (shared by
tests/test_origin_recipe.py and tests/test_gpu_raw_spans.py).

normalize_with_owners(data, capcode, norm_flag) -> (normalized bytes, own): one character of the raw document at a time - `unicodedata` for
its NFD and lower-case form, then the capcode level 2 encoder of javascript/tokenmonster.js:900-1005 as tokenmonster_amd/csrc/tm_normalize.cpp
states it (capcode_encode, mark_run_letters) - and with every byte it appends, the raw offset of the character that byte belongs to:
the character's own bytes, the marker bytes written in front of its letter ("D ", "DC ", "DW ", the space behind a 'W' / 'C' that took the
place of a raw space); a 'W' / 'C' that overwrites a raw space stays the space's.

It is for well-formed UTF-8 whose combining marks stand in canonical order (the model normalizes character by character and says so with an
assertion) and whose characters have old, stable properties, so that Python's Unicode data and ICU's agree.  Its bytes are checked against
tm_normalize wherever it is used: a difference is a failure of the test that uses it.

raw_spans(spans, own, raw_len) maps normalized (begin, end) pairs through `own` by the definition of include/tokenmonster_hip.h."""
import unicodedata as ud

import numpy as np


def _chars(data):
    """-> [(offset, character)] of well-formed UTF-8"""
    text = bytes(data).decode("utf-8")            # (raises on anything else: the model is not for it)
    out, off = [], 0
    for ch in text:
        out.append((off, ch))
        off += len(ch.encode("utf-8"))
    return out


def _cls(ch):
    """the classes of tm_normalize.cpp: classify"""
    o = ord(ch)
    if o < 0x80:
        if "a" <= ch <= "z":
            return {"lower", "letter"}
        if "A" <= ch <= "Z":
            return {"upper", "letter"}
        if "0" <= ch <= "9":
            return {"digit"}
        return set()
    cat = ud.category(ch)
    return {"Lu": {"upper", "letter"}, "Ll": {"lower", "letter"}, "Lt": {"letter"}, "Lm": {"letter"}, "Lo": {"letter"}, "Nd": {"digit"},
            "Mn": {"mark"}, "Me": {"mark"}, "Mc": {"mark"}}.get(cat, set())


def _lower1(ch):
    """what capcode writes for a capital: its simple lower-case form"""
    if ord(ch) < 0x80:
        return chr(ord(ch) | 0x20)
    low = ch.lower()
    return low if len(low) == 1 else ch


class _Last:
    def __init__(self, ch=None):
        c = _cls(ch) if ch is not None else set()
        self.space = ch == " "
        self.letter = "letter" in c
        self.apostrophe = ch in ("'", "’")
        self.mark = "mark" in c
        self.digit = "digit" in c

    def joiner(self):
        return self.letter or self.apostrophe or self.mark


def _mark_run_letters(buf, start):
    """every lower-case letter behind `start` gets "DC " in front of it - owned by that letter - an existing "D " in front of one becomes
    "DC "; a "D " in front of anything else is skipped together with the element behind it"""
    tail = buf[start:]
    del buf[start:]
    i, n = 0, len(tail)
    while i < n:
        if tail[i][0] == "D" and i + 1 < n and tail[i + 1][0] == " ":
            if i + 2 < n and "lower" in _cls(tail[i + 2][0]):
                own = tail[i + 2][1]
                buf += [("D", own), ("C", own), (" ", own), tail[i + 2]]
                i += 3
            else:
                buf += tail[i:i + 3]
                i += 3
            continue
        if "lower" in _cls(tail[i][0]):
            own = tail[i][1]
            buf += [("D", own), ("C", own), (" ", own)]
        buf.append(tail[i])
        i += 1


def _capcode_encode(src):
    """src: [(character, owner)] -> the same with the markers"""
    buf = []
    goback = word_token_pos = 0
    last, last2 = _Last(), _Last()
    in_word = multi = False
    for ch, own in src:
        c = _cls(ch)
        apostrophe = ch in ("'", "’")
        if in_word:
            if "upper" in c:
                if not last.joiner():
                    buf += [("D", own), (" ", own)]
                multi = True
                buf.append((_lower1(ch), own))
            else:
                if "lower" in c:
                    in_word = False
                    buf[word_token_pos] = ("C", buf[word_token_pos][1])
                    if multi:
                        _mark_run_letters(buf, goback)
                    if not last.joiner():
                        buf += [("D", own), (" ", own)]
                elif "digit" in c:
                    if not last.digit:
                        buf += [("D", own), (" ", own)]
                elif not (apostrophe or "mark" in c):
                    in_word = False
                buf.append((ch, own))
        else:
            if "lower" in c:
                if not (last.space or last.letter or (last2.letter and last.apostrophe) or last.mark):
                    buf += [("D", own), (" ", own)]
                buf.append((ch, own))
            elif "upper" in c:
                if last.space:
                    word_token_pos = len(buf) - 1
                    buf[word_token_pos] = ("W", buf[word_token_pos][1])      # over the raw space: the space's
                    buf.append((" ", own))
                else:
                    buf.append(("D", own))
                    word_token_pos = len(buf)
                    buf += [("W", own), (" ", own)]
                buf.append((_lower1(ch), own))
                goback = len(buf)
                multi = False
                in_word = True
            elif "digit" in c:
                if not (last.space or last.digit):
                    buf += [("D", own), (" ", own)]
                buf.append((ch, own))
            else:
                buf.append((ch, own))
        last2, last = last, _Last(ch)
    return buf


def normalize_with_owners(data, capcode, norm_flag):
    assert capcode in (0, 2) and norm_flag & ~3 == 0, "the model is for NFD, lowercase and capcode 0 / 2"
    seq = []
    for off, ch in _chars(data):
        parts = ud.normalize("NFD", ch) if norm_flag & 1 else ch
        if norm_flag & 2:
            parts = "".join(p.lower() for p in parts)
        seq += [(p, off) for p in parts]
    if norm_flag & 1:      # character by character is the whole text's NFD only while no mark changes places
        whole = ud.normalize("NFD", bytes(data).decode("utf-8"))
        if norm_flag & 2:
            whole = "".join(p.lower() for p in whole)
        assert whole == "".join(p for p, _ in seq), "the model is for marks in canonical order"
    if capcode == 2:
        seq = _capcode_encode(seq)
    out, own = bytearray(), []
    for ch, o in seq:
        b = ch.encode("utf-8")
        out += b
        own += [o] * len(b)
    return bytes(out), np.array(own, dtype=np.int64)


def raw_spans(spans, own, raw_len):
    """normalized pairs [n, 2] of ONE document -> raw pairs, by the definition: (own[nb], next(ne - 1)) for ne > nb, else (x, x) with
    x = next(nb - 1), or 0 when nb == 0; next(n) = the first own[n'] > own[n] behind n, or the raw length"""
    own = np.asarray(own, dtype=np.int64)
    nxt = np.full(own.size, raw_len, dtype=np.int64)
    for n in range(own.size - 2, -1, -1):
        nxt[n] = own[n + 1] if own[n + 1] > own[n] else nxt[n + 1]
    out = np.zeros((len(spans), 2), dtype=np.int64)
    for k, (nb, ne) in enumerate(np.asarray(spans, dtype=np.int64).reshape(-1, 2)):
        if ne > nb:
            out[k] = (own[nb], nxt[ne - 1])
        else:
            x = nxt[nb - 1] if nb > 0 else 0
            out[k] = (x, x)
    return out

"""CPU: the claim the streaming encoder's raw path rests on (tm_encoder_feed_raw, tm_encoder.hip).  Behind a line feed - and behind a tab or
one of the ASCII punctuation bytes the encoder falls back to when a line outgrows a piece - the normalizer is in the state it starts a text
in, so for every cut position p with raw[p - 1] in that set

    normalize(raw[:p]) + normalize(raw[p:]) == normalize(raw)

for every set of flags the encoder accepts (any of nfd 1, lowercase 2, accents 4, collapse 16, unixlines 128; never quotemarks 8, trim 32,
leadingspace 64) and capcode 0 and 2.  Host normalizer only (tm_normalize, which the suite pins to the reference runtime for all 256 flag
values): nothing here needs a device."""
import itertools

import numpy as np

from tokenmonster_amd import synth

SEPARATORS = b"\n\t.,;:!?()[]{}<>=/-\""
ACCEPTED_BITS = (1, 2, 4, 16, 128)
PARTS = ["HELLO", "Hello", "hello", "A", "I", "AB", "WORLD", "iPhone", "a", "bc", "1", "23", "4567", "'", "’", "don't", "DON'T", "IT’S",
         "café", "CAFÉ", "É", "niño", "é", "Ȩ́", "ä́", "̧́", "́", "ü", "Ü",
         "привет", "МИР", "Мир", "漢字", "が", "パ", "゙", "한글",
         "\U0001F600", "ＡＢ", "ἀ", "ẛ̣", " ", " ", "  ", "   ", "\r", "\r\n", "\n", "\n\n", " \n", "\t"]
PARTS_B = [p.encode() for p in PARTS] + [bytes([c]) for c in SEPARATORS] + [b"\xff", b"\xc3", b"\xe2\x80", b"\xf0\x9f"]


def corpus(rng, n_strings):
    out = []
    for _ in range(n_strings):
        k = int(rng.integers(2, 14))
        out.append(b"".join(PARTS_B[int(i)] for i in rng.integers(0, len(PARTS_B), size=k)))
    return out


def test_normalizer_has_no_state_behind_a_separator():
    rng = np.random.default_rng(20260101)
    texts = corpus(rng, 400)
    flag_sets = [sum(c) for r in range(len(ACCEPTED_BITS) + 1) for c in itertools.combinations(ACCEPTED_BITS, r)]
    assert len(flag_sets) == 32
    cuts = cuts_lf = 0
    for capcode in (0, 2):
        for flags in flag_sets:
            for t in texts:
                whole = None
                for p in range(1, len(t)):
                    if t[p - 1] not in SEPARATORS:
                        continue
                    if whole is None:
                        whole = bytes(synth.normalize(t, capcode, flags))
                    a, b = bytes(synth.normalize(t[:p], capcode, flags)), bytes(synth.normalize(t[p:], capcode, flags))
                    assert a + b == whole, "capcode %d flags %d: cut at %d behind %r of %r" % (capcode, flags, p, t[p - 1:p], t)
                    cuts += 1
                    cuts_lf += t[p - 1] == 0x0A
    assert cuts_lf > 5_000 and cuts > 40_000, (cuts_lf, cuts)      # a condition on the corpus, not on the code


def test_a_cut_elsewhere_does_change_the_text():
    """the other half: the claim is about the separators, not a property every byte has - a cut inside a capital run, between a letter and
    its mark, between '\\r' and '\\n' and inside a run of blanks gives other bytes (so the encoder must not cut there)"""
    def split_differs(t, p, capcode, flags):
        n = lambda x: bytes(synth.normalize(x, capcode, flags))
        return n(t[:p]) + n(t[p:]) != n(t)
    assert split_differs(b"HELLO WORLD", 3, 2, 1)
    assert split_differs("e\u0301\u0327".encode(), 3, 2, 1)
    assert split_differs(b"a\r\nb", 2, 0, 128)
    assert split_differs(b"a  b", 2, 0, 16)

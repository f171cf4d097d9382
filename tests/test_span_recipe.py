"""CPU: the recipe the span tests take their expected values from (tests/span_recipe.py: the oracle's scoring walk chained one token boundary
at a time) on the committed fixtures.  This checks the yardstick, not the feature: the recipe must give one span per id of the fixture, count
the fixture's missing characters, and every span's text must be the tail of its token's key (the tail, not the key: a "D " duplicate's key
begins with a marker the text does not have, a forward-delete token's with a space it does not consume, an alternative is cut short)."""
import base64
import glob
import os

import numpy as np

import conftest
from oracle_bind import Oracle
from span_recipe import SpanStats, check_order, oracle_spans

FIXTURES = sorted(glob.glob(os.path.join(conftest.GOLDEN_DIR, "fuzz_*.json"))) + [os.path.join(conftest.GOLDEN_DIR, "englishcode2048.json")]


def fixture_cases():
    for path in FIXTURES:
        g = conftest.load_golden(path)
        img = base64.b64decode(g["vocab_b64"])
        docs = [base64.b64decode(d) for d in g["docs_b64"]]
        yield path, img, docs, g["ids"], g["missing"]


def vocab_has_unk(orc, docs):
    """whether a character without a token leaves an id: asked of the oracle itself"""
    for c in range(256):
        ids, miss = orc.tokenize(bytes([c]))
        if miss:
            return ids.size == 1
    return False


def test_recipe_on_the_committed_fixtures():
    total = SpanStats()
    assert len(FIXTURES) == 4
    for path, img, docs, ids, missing in fixture_cases():
        orc = Oracle(img)
        has_unk = vocab_has_unk(orc, docs)
        keys = {}
        for d, doc in enumerate(docs):
            st = SpanStats()
            spans = oracle_spans(orc, doc, has_unk, st)
            exp, miss = orc.tokenize(doc)
            assert exp.tolist() == ids[d] and miss == missing[d], (path, d)
            assert spans.shape[0] == len(ids[d]), (path, d)
            assert st.missing_unk + st.missing_nounk == missing[d], (path, d)
            check_order(spans)
            assert spans.size == 0 or (spans[0, 0] >= 0 and spans[-1, 1] <= len(doc))
            for (a, e), t in zip(spans.tolist(), ids[d]):
                if t not in keys:
                    keys[t] = orc.decode_raw(np.array([t], dtype=np.uint32))
                if e - a == 1 and has_unk and keys[t] == b"":
                    continue                   # (the unk token has no key)
                assert keys[t].endswith(doc[a:e]), (path, d, a, e, t)
            total.add(st)
    assert (total.docs, total.ids, total.zero, total.delete, total.missing_unk + total.missing_nounk) == (91, 76241, 211, 2309, 4432), total

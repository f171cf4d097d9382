"""-m "not gpu": tests/test_gpu_match_boundaries.py (every construct of tests/match_cases.py across the seams of the match kernel: segment, workgroup,
document end, long document, normalizer slab, ring, exit maps) on the emulated device - tools/emu, the kernel sources compiled for the host
(tests/conftest.py, TM_EMU=1) - in a child process, cut down by the fixed rule that module states.  A pass here is about the kernels' logic; the
-m gpu run is the claim.

And the anchor of the sweep's expected side: every construct alone, and across byte 256 at straddles 0, 1 and len - 1 in front of each tail, through
the REFERENCE runtime's tokenize (oracle/_ref) equals the oracle (oracle/tm_oracle.c), which the sweep compares the device with - ids, missing
counts and the count call."""
import os
import re
import subprocess
import sys

import pytest

import match_cases as M
from oracle_bind import Oracle, Reference, have_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_match_boundaries_on_the_emulated_device():
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_match_boundaries.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert re.search(r"^26 passed, 1 deselected", out, re.M) and " failed" not in out, out[-2000:]


@pytest.mark.skipif(not have_ref(), reason="the reference runtime (oracle/_ref) is built only where the reference tree is present")
@pytest.mark.parametrize("form", M.FORMS)
def test_the_oracle_equals_the_reference_on_every_construct(form):
    img = M.image(form)
    orc, ref = Oracle(img), Reference(img)
    fd = M.fd_tails(orc, form)
    assert bool(fd) == (M.form_props(form)[0] == 2)
    cs = M.constructs(form, fd[0] if fd else None)
    tails = M.tails(form, fd)
    fill = M.fillers(form, orc)["token"]
    seam = M.seam_chars(form)
    n = 0
    for c in cs:
        docs = [M.place(form, b"", 0, c.data)]
        for s in (0, 1, len(c.data) - 1):
            docs += [M.place(form, fill, seam - s, c.data, t) for _, t in tails]
        for doc in docs:
            eids, emiss = ref.tokenize_normalized(doc)
            ids, miss = orc.tokenize(doc)
            assert ids.tolist() == eids.tolist() and miss == emiss, (form, c.name, doc)
            assert orc.count(doc) == ref.count_normalized(doc), (form, c.name, doc)
            n += 1
    assert n == len(cs) * (1 + 3 * len(tails))

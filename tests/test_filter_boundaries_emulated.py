"""-m "not gpu": tests/test_gpu_filter_boundaries.py (every construct of tests/filter_cases.py across the seams of the device filter pass, in
every state of the document, under the byte-level flag sets) on the emulated device - tools/emu, the kernel sources compiled for the host
(tests/conftest.py, TM_EMU=1) - in a child process, cut down by the fixed rule that module states (the seams 4, 256 and 4096, twelve flag sets,
one state of every kind, five tails, one document length at the switch).  A pass here is about the kernels' logic; the -m gpu run is the claim.

And the anchor of the sweep's expected side: each construct alone and behind each state prefix through the REFERENCE runtime's normalize
(oracle/_ref) equals this project's host normalizer, which the sweep compares the device with, for the 64 combinations of the flags 4, 8, 16,
32, 64 and 128."""
import os
import re
import subprocess
import sys

import pytest

import filter_cases as F
from oracle_bind import Reference, have_ref
from tokenmonster_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS64 = F.FLAGS64


def test_filter_boundaries_on_the_emulated_device():
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_filter_boundaries.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert re.search(r"^8 passed, 2 deselected", out, re.M) and " failed" not in out, out[-2000:]


@pytest.mark.skipif(not have_ref(), reason="the reference runtime (oracle/_ref) is built only where the reference tree is present")
@pytest.mark.parametrize("flags", [tuple(FLAGS64[i:i + 16]) for i in range(0, 64, 16)], ids=lambda g: "flags-%d-to-%d" % (g[0], g[-1]))
def test_the_host_normalizer_equals_the_reference_on_every_construct(flags):
    n = 0
    for flag in flags:
        ref = Reference(synth.build_vocab([bytes([c]) for c in range(256)], capcode=2, charset=1, norm_flag=flag))
        for c in F.CONSTRUCTS:
            if c.name in F.REFERENCE_REFUSES:      # malformed UTF-8 ("E2 80", "80 99", "E2 E2 80 99"): left out of this test, and only of it
                continue
            docs = [c.data] + [F.place(c, 0, len(s[1]) + 2, s[0], "y") for s in F.STATES] + [F.place(c, 0, len(s[1]), s[0], "drop, quote") for s in F.STATES]
            for doc in docs:
                assert ref.normalize(doc) == bytes(synth.normalize(doc, 2, flag)), (c.name, flag, doc)
                n += 1
    assert n == len(flags) * (1 + 2 * len(F.STATES)) * (len(F.CONSTRUCTS) - len(F.REFERENCE_REFUSES))
    assert F.REFERENCE_REFUSES == {"E2 80", "80 99", "E2 E2 80 99"}

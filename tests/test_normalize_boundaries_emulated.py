"""-m "not gpu": tests/test_gpu_normalize_boundaries.py (every construct of tests/boundary_cases.py across the seams of the device normalizer) on
the emulated device - tools/emu, the kernel sources compiled for the host (tests/conftest.py, TM_EMU=1) - in a child process, cut down by the
fixed rule that module states (the seams 64 and 1024, the capital and mixed fillers, 3 bytes of tail, hook 0 beyond the first vocabulary: about
1 MB per call).  A pass here is about the kernels' logic; the -m gpu run is the claim.

And the anchor of the sweep's expected side: each construct alone and inside the capital filler through the REFERENCE runtime's normalize
(oracle/_ref) for the (2, 1) and (0, 0) vocabularies equals this project's host normalizer, which the sweep compares the device with."""
import os
import subprocess
import sys

import pytest

import boundary_cases as B
from oracle_bind import Reference, have_ref
from tokenmonster_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normalize_boundaries_on_the_emulated_device():
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_normalize_boundaries.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert "12 passed" in out and " failed" not in out, out[-2000:]


@pytest.mark.skipif(not have_ref(), reason="the reference runtime (oracle/_ref) is built only where the reference tree is present")
@pytest.mark.parametrize("capcode,flags", [(2, 1), (0, 0)])
def test_the_host_normalizer_equals_the_reference_on_every_construct(capcode, flags):
    ref = Reference(synth.build_vocab([bytes([c]) for c in range(256)], capcode=capcode, charset=1, norm_flag=flags))
    n = 0
    for c in B.CONSTRUCTS:
        if c.name in B.REFERENCE_REFUSES:      # malformed UTF-8: left out of this test, and only of it
            continue
        for doc in (c.data, B.place(c, 0, 70, "capital", 70), B.place(c, 0, 3, "capital", 0)):
            assert ref.normalize(doc) == bytes(synth.normalize(doc, capcode, flags)), (c.name, capcode, flags, doc)
            n += 1
    assert n == 3 * (len(B.CONSTRUCTS) - len(B.REFERENCE_REFUSES))

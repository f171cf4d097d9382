"""-m "not gpu": tests/test_gpu_decode_boundaries.py (every construct of tests/boundary_cases.py across the seams of the device capcode decoder) on
the emulated device - tools/emu, the kernel sources compiled for the host (tests/conftest.py, TM_EMU=1) - in a child process, cut down by the
fixed rule that module states (the seams 64 and 1024, the long documents for every eighth construct).  A pass here is about the kernels'
logic; the -m gpu run is the claim."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_boundaries_on_the_emulated_device():
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_decode_boundaries.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert "4 passed" in out and " failed" not in out, out[-2000:]

"""-m "not gpu": tests/test_gpu_batch_buffers.py (the grow-only buffers a batch owns, over rounds of different sizes on one batch) on the
emulated device - tools/emu, the kernel sources compiled for the host (tests/conftest.py, TM_EMU=1) - in a child process.  A pass here is about
the host code's logic; the -m gpu run is the claim."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_buffers_on_the_emulated_device():
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_batch_buffers.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert " passed" in out and " failed" not in out, out[-2000:]

"""-m "not gpu": tests/test_gpu_pairs.py and tests/test_gpu_pairs_torch.py (tm_batch_pair, tm_batch_pair_windows, their spans and the torch wrappers) on
the emulated device - tools/emu, the kernel sources compiled for the host (tests/conftest.py, TM_EMU=1) - in a child process.  A pass here is about
the kernels' logic; the -m gpu run is the claim."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pairs_on_the_emulated_device():
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_pairs.py", "tests/test_gpu_pairs_torch.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert " passed" in out and " failed" not in out, out[-2000:]

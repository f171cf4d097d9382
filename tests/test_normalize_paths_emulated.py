"""-m "not gpu": tests/test_gpu_normalize_paths.py (the five outcomes of tm_batch_normalize, the filter pass, capcode 0, the streaming encoder's raw
pieces) on the emulated device - tools/emu, the kernel sources compiled for the host (tests/conftest.py, TM_EMU=1) - in a child process.  A pass
here is about the host path's logic; the -m gpu run is the claim."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normalize_paths_on_the_emulated_device():
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_normalize_paths.py", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert "33 passed" in out and " failed" not in out, out[-2000:]

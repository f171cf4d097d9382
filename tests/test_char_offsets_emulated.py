"""-m "not gpu": tests/test_gpu_char_offsets.py (tm_batch_spans_in / tm_batch_collate_spans_in / tm_batch_windows_spans_in / tm_tokenize_batch_spans_in)
on the emulated device - tools/emu, the kernel sources compiled for the host (tests/conftest.py, TM_EMU=1) - in a child process; the torch cases need a
real device and stay out.  A pass here is about the kernels' logic; the -m gpu run is the claim."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_char_offsets_on_the_emulated_device():
    env = dict(os.environ, TM_EMU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_char_offsets.py", "-q", "-m", "gpu", "-k", "not torch", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-4000:]
    assert " passed" in out and " failed" not in out, out[-2000:]

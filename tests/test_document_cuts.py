"""CPU: the piece layout and the cut search behind tm_tokenize_document and the streaming encoder (tokenmonster_amd/csrc/tm_cuts.h) in a
stand-alone program of their own (tools/cuts_check.cpp), built with the address and undefined-behaviour sanitizers and run here: pieces tile
the document, every piece behind another is at least the minimum range long, nobody looks past the end, and a raw cut lies behind a byte of
the fallback set within the piece size."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cuts_under_sanitizers(tmp_path):
    cxx = next(c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c))
    exe = str(tmp_path / "cuts_check")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tokenmonster_amd", "csrc"),
                        os.path.join(ROOT, "tools", "cuts_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"cuts ok" in r.stdout, r.stdout.decode(errors="replace")

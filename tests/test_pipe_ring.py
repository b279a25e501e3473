"""The wave-pair FIFO's index and bounded-wait arithmetic (csrc/kernels/
pipe_ring.hpp) is plain C++ shared with the device code: a stand-alone host
program (tests/host/pipe_ring_check.cpp) replays the two waves' protocol —
ring wrap, counters near 2^32, the skipped priming rows, items back to back,
the wait bound across a clock wrap — built with AddressSanitizer and
UndefinedBehaviorSanitizer. No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "cuda-hip-mpi-heat-equation-test_amd", "csrc", "kernels")
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def test_pipe_ring_host_check_under_sanitizers(tmp_path):
    cxx = CXX if os.path.exists(CXX) else shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the host check")
    exe = str(tmp_path / "pipe_ring_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", KERNELS, os.path.join(ROOT, "tests", "host", "pipe_ring_check.cpp"),
                    "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pipe_ring_check ok" in out.stdout

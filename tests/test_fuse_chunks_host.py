"""CPU: the chunk arithmetic of a fused mc_step_many call (csrc/mc_fuse.h):
K steps as ceil(K / S) launches of at most S steps, the five byte offsets
first * stride in int64, an overflowing k * stride refused, and the
MARLCOV_FUSE_STEPS parse.  tests/native/fuse_chunks_check.cpp includes the
header, is compiled host-only with AddressSanitizer and UBSan, and checks
K = 0, 1, S - 1, S, S + 1 and 200 at S = 64, S = 16, S = 1, zero and non-zero
strides, and overflowing offsets."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunks_tile_the_call_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    exe = tmp_path / "fuse_chunks_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), os.path.join(ROOT, "tests", "native", "fuse_chunks_check.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok", lines[-1]
    assert "K 200 S 64 -> 4 launches" in lines
    assert "K 40 S 16 -> 3 launches" in lines
    assert "K 40 S 1 -> 40 launches" in lines
    assert "K 0 S 64 -> 0 launches" in lines

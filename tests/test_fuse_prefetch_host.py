"""CPU: the fused loop's action prefetch (csrc/mc_fuse.h fuse_prefetch_step):
step k of a launch prefetches the next step's action row, and the launch's
last step its own row again, so that no address past the launch's last row is
formed.  tests/native/fuse_prefetch_check.cpp includes the header, is compiled
host-only with AddressSanitizer and UBSan, and reads every prefetched row of
calls of K = 1 .. 200 steps at S = 1, 2, 3 and 64 through the kernel's address
expression, over heap buffers of exactly K rows."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prefetch_stays_inside_the_launch_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    exe = tmp_path / "fuse_prefetch_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "fuse_prefetch_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok", lines[-1]
    assert "K 200 S 64 stride 8: 200 prefetches inside the buffer" in lines
    assert "K 7 S 3 stride 8: 7 prefetches inside the buffer" in lines
    assert "K 65 S 1 stride 24: 65 prefetches inside the buffer" in lines

"""CPU: the fused loop's record prefetch (csrc/mc_fuse.h fuse_predict_cell,
csrc/mc_vistab.h vis_item_offset).  Step k of a fused launch predicts every
robot's cell after step k + 1 and loads the items' tiles of those cells'
visibility records a step ahead.  tests/native/vis_prefetch_check.cpp includes
the headers, is compiled host-only with AddressSanitizer and UBSan, compares
the predictor with a literal restatement of the single-robot move rule over
every action byte and every cell of a 20 x 26 map, and walks the shared
address expression over heap buffers of exactly vis_table_bytes(G, Wp, Lp)
bytes for G = 1 and 3, garbage cells included."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predictor_and_prefetch_addresses_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    exe = tmp_path / "vis_prefetch_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "vis_prefetch_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok", lines[-1]
    assert lines[0] == "predictor: %d cases" % (20 * 26 * 256 * 2), lines[0]
    bytes_per_grid = 20 * 26 * 128
    per_grid = 20 * 26 * 256 * 2 * 17
    junk = 5 * 9 ** 4 * 16
    assert lines[1] == f"G 1: {per_grid + junk} prefetch reads inside the table of {bytes_per_grid} bytes", lines[1]
    assert lines[2] == f"G 3: {3 * per_grid + junk} prefetch reads inside the table of {3 * bytes_per_grid} bytes", lines[2]

"""CPU: the shorter forms the carried step kernels compute with
(csrc/mc_internal.h edge_clip, csrc/mc_env_select.h ItemGeo).
tests/native/step_diet2_check.cpp includes the headers, is compiled host-only
with AddressSanitizer and UBSan, and compares each with the general form it
replaces: the two-mask clip with tile_in_grid for every tile of every Wp, Lp in
8..40, the items' geometry with stage_load's divisions for every lane and item,
and the dedup rounds built from it with the pairs some lane has; a State whose
TW is not window_tiles(H) is refused by shape_matches."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_and_geometry_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    exe = tmp_path / "step_diet2_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "step_diet2_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok", lines[-1]
    tiles = sum(((w + 7) // 8) * ((l + 7) // 8) for w in range(8, 41) for l in range(8, 41))
    assert lines[0] == f"clip: {tiles} tiles", lines[0]
    assert lines[1] == f"geometry: {2 * 32 + 2 * 64} items", lines[1]

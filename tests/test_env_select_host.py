"""CPU: which env-kernel instantiation runs a state, and its launch geometry
(csrc/mc_env_select.h: the row list, select_env_row, env_takes_vis_table,
env_geometry).  tests/native/env_select_check.cpp includes that header alone,
is compiled host-only with AddressSanitizer and UBSan and run as a child
process.  For each of the 27 rows it builds a State from the row's own shape
fields and checks that exactly that row is selected (by its label, which
tells ShapeC2, ShapeC2B and ShapeC2BV apart) and that its public name is the
literal listed there; that a row's needs are the ones its kernel derives
(C5 and generic rows none, C4 rows 32-bit offsets, C2 rows also ray programs,
C2 V rows also the table); the fallbacks one step at a time (no table: the
march row; no ray programs, MARLCOV_SPECIALIZE=0, maps past 4 GB, or a C2
state at 128 lanes: the generic kernel of the same lanes and word; C5 rows stay
past 4 GB); and the lanes, envs per workgroup and word size of the twelve
ORGANIC configurations of tests/test_gpu_launch_shapes.py with the MARLCOV_NT
rule (below the computed lanes: ignored; above: one env per workgroup)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_fallbacks_and_geometry_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    exe = tmp_path / "env_select_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), os.path.join(ROOT, "tests", "native", "env_select_check.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert r.stdout.strip().split("\n") == ["rows 27", "geometry 12", "ok"], r.stdout[-4000:]


def test_organic_table_is_the_gpu_suites():
    """The host check's copy of the ORGANIC table names the same cases with the
    same variants as tests/test_gpu_launch_shapes.py."""
    import re
    src = open(os.path.join(ROOT, "tests", "native", "env_select_check.cpp")).read()
    rows = re.findall(r'\{"(\w+)", (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},', src)
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_launch_shapes.py")).read()
    cases = dict(re.findall(r'"(\w+)": \((?:lidar|square)\(.*?"(env_kernel<[^"]+>)"\)', gpu, re.S))
    assert len(rows) == 12 and sorted(n for n, *_ in rows) == sorted(cases)
    for name, n, beams, rng, nt, epw, wb in rows:
        assert cases[name] == f"env_kernel<{nt},{epw},u{8 * int(wb)},generic>", name
        call = re.search(rf'"{name}": \((lidar|square)\(([^)]*)\)', gpu)
        args = [a.strip() for a in call.group(2).split(",")]
        want = [n, beams, rng] if call.group(1) == "lidar" else [n, rng]
        assert args[:len(want)] == want and (call.group(1) == "square") == (beams == "0"), name

"""CPU: the tile form of the visibility table's records (csrc/mc_vistab.h
vis_tiles_as, the function the build kernel runs after vis_record).
tests/native/vis_tiles_check.cpp includes it, is compiled host-only with
AddressSanitizer and UBSan and run as a child process.  On a 40 x 33 map with
10 % obstacles and lidars of half-width H = 10, 3 and 1 it builds the unsplit
and the split record of every cell and compares every bit of every tile with a
per-cell restatement from vis_record's rows and vis_blocked (the rows
themselves are checked against the oracle's lidar by test_vis_table_host.py).
The program also reports what the cells covered: every (x - H) & 7, (y - H) & 7
residue pair, and windows that leave the map on each of its four sides."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_vis_table_host import beam_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WP, LP = 40, 33
CASES = [(21, 10.0, 10), (21, 3.0, 3), (13, 1.0, 1)]  # beams, range, H


def test_tile_records_match_the_rows_under_sanitizers(tmp_path):
    from oracle.cpu_ref import lidar_beam_table, lidar_thetas
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    rs = np.random.RandomState(4321)
    grid = rs.choice([1.0, -1.0], size=(WP, LP), p=[0.9, 0.1])  # no border ring: windows leave the map over free cells
    txt = tmp_path / "cases.txt"
    ncases = 0
    with open(txt, "w") as f:
        for nb, rng, H in CASES:
            beams, words, k1 = beam_records(lidar_beam_table(lidar_thetas(nb)), rng, WP, LP)
            assert 1 <= max(b[0] for b in beams) <= H
            for common in (0, 1):
                f.write(f"{WP} {LP} {H} {nb} {common} {k1 if common else 0} {max(WP, LP)}\n")
                for K, axis, sign, msign, bits in beams:
                    f.write(f"{K} {axis if common else axis | 2} {sign} {msign} {bits}\n")
                for row in words:
                    f.write(" ".join(f"{w:x}" for w in row) + "\n")
                for x in range(WP):
                    f.write("".join("#" if grid[x, y] < 0 else "." for y in range(LP)) + "\n")
                ncases += 1
    exe = tmp_path / "vis_tiles_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), os.path.join(ROOT, "tests", "native", "vis_tiles_check.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe), str(txt)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"ok {ncases} cases", lines[-1]
    assert len(lines) == ncases + 1
    for (nb, rng, H), pair in zip(CASES, zip(lines[0:-1:2], lines[1:-1:2])):
        for line in pair:
            tok = line.split()
            assert tok[:4] == ["case", str(WP), str(LP), str(H)], line
            assert int(tok[5], 16) == (1 << 64) - 1, f"not every residue pair was covered: {line}"
            assert int(tok[7], 16) == 0xF, f"no window left the map on some side: {line}"
            assert int(tok[9]) > WP * LP, line  # more than the robots' own cells

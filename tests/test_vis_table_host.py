"""CPU: the records of the lidar's visibility table (csrc/mc_vistab.h
vis_record, the function the build kernel runs for every pool cell).
tests/native/vis_table_check.cpp includes it, is compiled host-only with
AddressSanitizer and UBSan, and prints the record of every cell of a 12 x 9 and
a 23 x 31 Bernoulli grid with a border ring, for 21 beams at R = 10 and 13
beams at R = 6.5 -- once marching every beam from its per-start step bits and
once from the common pattern with the step-1 premarks (the form the device
tables have when a table is built).  Every record is compared with the
oracle's lidar run from that cell (oracle/cpu_ref.py LidarRef): free and
obstacle marks together, rows and columns relative to the cell.  Beam records
are derived here from the increment table the way mc_set_beam_table derives
them."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def beam_records(table, rng, Wp, Lp):
    """Per beam (K, axis, sign, msign, common bits), the per-start words
    [nbeams][max(Wp, Lp)] and the step-1 mask, as mc_set_beam_table computes
    them (csrc/mc_capi.hip)."""
    cmax = max(Wp, Lp)
    beams, words, k1 = [], [], 1 << 4
    for xi, yi, di in table:
        if abs(xi) == 1.0:
            axis, sign, minor, cm = 0, (1 if xi > 0 else -1), float(yi), Lp
        else:
            assert abs(yi) == 1.0
            axis, sign, minor, cm = 1, (1 if yi > 0 else -1), float(xi), Wp
        msign = 1 if minor > 0 else (-1 if minor < 0 else 0)
        dist, K = 0.0, 0
        while dist < rng:
            dist += float(di)
            K += 1
        def chain(c0):
            m, cell, w = float(c0), c0, 0
            for k in range(K):
                m += minor
                nxt = int(m)
                if nxt != cell:
                    w |= 1 << k
                cell = nxt
            return w

        row = [chain(c0) if c0 < cm else 0 for c0 in range(cmax)]
        common = chain(64)  # a start far from the border: the common pattern
        beams.append((K, axis, sign, msign, common))
        words.append(row)
        if K >= 1:
            mv = msign if common & 1 else 0
            dx, dy = (sign, mv) if axis == 0 else (mv, sign)
            k1 |= 1 << (3 * (dx + 1) + (dy + 1))
    return beams, words, k1


def ring_grid(rs, Wp, Lp, p):
    g = rs.choice([1.0, -1.0], size=(Wp, Lp), p=[1 - p, p])
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = -1.0
    return g


CASES = [(12, 9, 21, 10.0), (23, 31, 21, 10.0), (12, 9, 13, 6.5), (23, 31, 13, 6.5)]


def test_records_match_the_oracle_lidar_under_sanitizers(tmp_path):
    from oracle.cpu_ref import LidarRef, lidar_beam_table, lidar_thetas
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    rs = np.random.RandomState(1234)
    runs = []  # (grid, H, sensor) per case of the input file
    txt = tmp_path / "cases.txt"
    with open(txt, "w") as f:
        for Wp, Lp, nb, rng in CASES:
            grid = ring_grid(rs, Wp, Lp, 0.12)
            H = max(int(math.ceil(rng)), 2)  # mc_create: max(ceil(range), egoradius)
            beams, words, k1 = beam_records(lidar_beam_table(lidar_thetas(nb)), rng, Wp, Lp)
            assert max(b[0] for b in beams) <= H
            for common in (0, 1):
                f.write(f"{Wp} {Lp} {H} {nb} {common} {k1 if common else 0} {max(Wp, Lp)}\n")
                for K, axis, sign, msign, bits in beams:
                    # per-start form: every beam flagged to read its start's own word
                    f.write(f"{K} {axis if common else axis | 2} {sign} {msign} {bits}\n")
                for row in words:
                    f.write(" ".join(f"{w:x}" for w in row) + "\n")
                for x in range(Wp):
                    f.write("".join("#" if grid[x, y] < 0 else "." for y in range(Lp)) + "\n")
                runs.append((grid, H, LidarRef({"num_lasers": nb, "range": rng})))
    exe = tmp_path / "vis_table_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), os.path.join(ROOT, "tests", "native", "vis_table_check.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe), str(txt)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"ok {len(runs)} cases", lines[-1]
    it = iter(lines[:-1])
    want_cache = {}
    for ci, (grid, H, sensor) in enumerate(runs):
        Wp, Lp = grid.shape
        assert next(it) == f"case {Wp} {Lp} {H}"
        pad = H + 1
        for x in range(Wp):
            for y in range(Lp):
                tok = next(it).split()
                assert (int(tok[0]), int(tok[1])) == (x, y)
                rows = [int(t, 16) for t in tok[2:]]
                assert len(rows) == 2 * H + 1
                key = (ci // 2, x, y)  # the two forms of a case share the oracle's run
                if key not in want_cache:
                    z = np.zeros((Wp + 2 * pad, Lp + 2 * pad))
                    nf, no = sensor.getMeasurement(x, y, grid, z, z, pad)
                    m = (nf + no) > 0
                    win = m[x + pad - H:x + pad + H + 1, y + pad - H:y + pad + H + 1]
                    assert m.sum() == win.sum(), "a mark outside the record's window"
                    want_cache[key] = [sum(1 << c for c in range(2 * H + 1) if win[r, c]) for r in range(2 * H + 1)]
                assert rows == want_cache[key], (ci, x, y, [hex(v) for v in rows], [hex(v) for v in want_cache[key]])
    assert next(it, None) is None

"""CPU: the host-built ray programs of the sparse-beam march
(csrc/mc_internal.h build_ray_prog).  tests/native/ray_prog_check.cpp includes
the builder, is compiled host-only with AddressSanitizer and UBSan, and checks
every lane, ray and step of the programs against a direct replay of the
march's `d0 + bit * d1` chain: offsets equal and within int16, K = -1 for
dead rays.  Beam records are derived here from the sensor's increment table
the way mc_set_beam_table derives them (float64 chain of the minor
coordinate from an interior start)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def beam_records(num_lasers, rng):
    """(K, axis, sign, msign, bits) per beam, as mc_set_beam_table computes
    them (csrc/mc_capi.hip): K steps of `currdist += distinc` below the
    range; bit k = the minor cell moves at step k."""
    from marlcov.sensors import beam_angles, beam_increments
    out = []
    for xi, yi, di in beam_increments(beam_angles(num_lasers)):
        if abs(xi) == 1.0:
            axis, sign, minor = 0, (1 if xi > 0 else -1), float(yi)
        else:
            assert abs(yi) == 1.0
            axis, sign, minor = 1, (1 if yi > 0 else -1), float(xi)
        msign = 1 if minor > 0 else (-1 if minor < 0 else 0)
        dist, K = 0.0, 0
        while dist < rng:
            dist += float(di)
            K += 1
        m, cell, bits = 64.0, 64, 0  # an interior start: the common pattern
        for k in range(K):
            m += minor
            nxt = int(m)
            assert nxt - cell in (0, msign)
            if nxt != cell:
                bits |= 1 << k
            cell = nxt
        out.append((K, axis, sign, msign, bits))
    return out


def test_ray_programs_replay_the_march_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    # N, lanes per env, rays per lane, kmax, row bytes: C2 with two envs per
    # wave and with one, and a 13-beam / R = 6.5 table (4 agents, two per wave)
    c2 = beam_records(21, 10)
    b13 = beam_records(13, 6.5)
    assert max(b[0] for b in c2) == 10 and min(b[0] for b in c2) == 8
    cases = [((4, 32, 3, 10, 4), c2), ((4, 64, 2, 10, 4), c2), ((4, 32, 3, max(b[0] for b in b13), 4), b13)]
    txt = tmp_path / "cases.txt"
    with open(txt, "w") as f:
        for geo, beams in cases:
            f.write(" ".join(map(str, geo)) + f" {len(beams)}\n")
            for b in beams:
                f.write(" ".join(map(str, b)) + "\n")
    exe = tmp_path / "ray_prog_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "marl-coverage_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "ray_prog_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe), str(txt)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"ok {len(cases)} cases", r.stdout

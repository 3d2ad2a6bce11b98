"""CPU: mc_import_maps without a device.

The packing functions of the import kernel (csrc/mc_import.h: a tile word from
a dense plane at any base alignment, the scan and validation of a robots plane)
are plain C++.  tests/native/import_check.cpp includes them and the export's
decode (csrc/mc_export.h), is compiled host-only with AddressSanitizer and
UBSan and run as a child process: on maps of 37 x 45, 34 x 48 and 9 x 5 cells,
at every base offset 0..15 of the plane inside an exactly-sized heap buffer
(an over-read is a sanitizer error), with bytes out of {0, 1, 2, 255}, it
compares every tile word with a per-cell restatement, decodes the tiles back
with export_chunk16, and has the robots scan accept a valid plane and reject a
value above N, a missing number, a duplicate and a robot on a blocked cell.
The counts it prints are compared with values computed from the shapes.

The library side: the two entry points are typed, refuse a null env by name,
and leave the ABI version alone."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = [(37, 45), (34, 48), (9, 5)]
BASES = 16


def test_packing_matches_a_per_cell_restatement_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    exe = tmp_path / "import_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), os.path.join(ROOT, "tests", "native", "import_check.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok 3 maps", lines[-1]
    assert len(lines) == len(MAPS) + 1
    for (wp, lp), line in zip(MAPS, lines):
        tok = line.split()
        assert tok[:3] == ["map", str(wp), str(lp)], line
        got = dict(zip(tok[3::2], map(int, tok[4::2])))
        tr, tc = -(-wp // 8), -(-lp // 8)
        # every tile of the 4 x 4 blocks, at every base offset
        assert got["tiles"] == BASES * 16 * -(-tr // 4) * -(-tc // 4), line
        assert got["cells"] == BASES * wp * lp, line
        # the tiles of the map that its right or bottom edge cuts
        cut = tr * tc - (wp // 8) * (lp // 8)
        assert cut > 0 and got["edge"] == BASES * cut, line
        assert got["robots"] == BASES * 6, line  # one valid plane and five invalid ones


@pytest.fixture(scope="module")
def lib():
    from marlcov import _lib
    return _lib.load()


def test_signatures_constants_and_version():
    import marlcov
    from marlcov import _lib
    typed = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert typed["mc_import_bytes"] == (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32])
    assert typed["mc_import_maps"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int32,
                                                      ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])
    assert _lib.ABI_VERSION == 12
    assert _lib.ERR_IMPORT == 128
    assert _lib.MAP_IMPORTABLE == 112 == marlcov.MAP_IMPORTABLE
    assert _lib.MAP_IMPORTABLE == _lib.MAP_ROBOTS | _lib.MAP_FREE | _lib.MAP_OBST
    assert callable(marlcov.BatchCoverageEnv.set_global_state)


def test_null_env_is_refused_by_name(lib):
    from marlcov import _lib
    assert lib.mc_abi_version() == 12
    assert lib.mc_import_bytes(None, _lib.MAP_IMPORTABLE, 4) == -1
    assert b"mc_import_bytes" in lib.mc_last_error()
    assert lib.mc_import_maps(None, _lib.MAP_IMPORTABLE, None, 4, None, 0, None) == _lib.MC_EINVAL
    assert b"mc_import_maps" in lib.mc_last_error()

"""CPU: mc_export_maps without a device.

The decode functions of the export kernel (csrc/mc_export.h: a 16-byte chunk
of a dense plane at any offset, the pooled count of a tile) are plain C++.
tests/native/export_check.cpp includes them, is compiled host-only with
AddressSanitizer and UBSan and run as a child process: on maps of 37 x 45,
34 x 48 and 9 x 5 cells with random tile words it compares every chunk at
every offset, and every pooled value, with a per-cell restatement.  The
program reports how many chunks ran over a row end, and over two.

The library side: the three entry points are typed, refuse a null env by
name, and leave the ABI version alone."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = [(37, 45), (34, 48), (9, 5)]


def test_decode_matches_a_per_cell_restatement_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    exe = tmp_path / "export_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), os.path.join(ROOT, "tests", "native", "export_check.cpp"),
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
        assert got["chunks"] == 2 * wp * lp, line  # every offset, for one map and for the OR of three
        assert got["rowend"] > 0, line
        assert got["pooled"] == 2 * -(-wp // 8) * -(-lp // 8), line
        if (wp, lp) == (9, 5):
            assert got["rowend2"] > 0, line  # 16 cells of a 5-cell row cross at least two row ends


@pytest.fixture(scope="module")
def lib():
    from marlcov import _lib
    return _lib.load()


def test_signatures_constants_and_version():
    import marlcov
    from marlcov import _lib
    typed = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert typed["mc_map_planes"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32])
    assert typed["mc_export_bytes"] == (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32,
                                                         ctypes.c_int32])
    assert typed["mc_export_maps"][0] is ctypes.c_int and len(typed["mc_export_maps"][1]) == 8
    assert _lib.ABI_VERSION == 12
    assert _lib.MAP_ALL == 127 == marlcov.MAP_ALL
    bits = [_lib.MAP_GRID_NEG, _lib.MAP_GRID_POS, _lib.MAP_VISITED, _lib.MAP_OBST_ANY, _lib.MAP_ROBOTS,
            _lib.MAP_FREE, _lib.MAP_OBST]
    assert bits == [1, 2, 4, 8, 16, 32, 64]
    assert _lib.MAP_NAMES == ("grid_neg", "grid_pos", "visited", "obst_any", "robots", "free", "obst")
    assert marlcov.MAP_ROBOTS == 16 and marlcov.MAP_FREE == 32
    assert _lib.ERR_EXPORT == 1 << 6
    assert callable(marlcov.BatchCoverageEnv.global_state)
    assert callable(marlcov.BatchCoverageEnv.global_state_planes)


def test_null_env_is_refused_by_name(lib):
    from marlcov import _lib
    assert lib.mc_abi_version() == 12
    assert lib.mc_map_planes(None, _lib.MAP_ALL) == -1
    assert b"mc_map_planes" in lib.mc_last_error()
    assert lib.mc_export_bytes(None, _lib.MAP_ALL, 1, 4) == -1
    assert b"mc_export_bytes" in lib.mc_last_error()
    assert lib.mc_export_maps(None, _lib.MAP_ALL, 1, None, 4, None, 0, None) == _lib.MC_EINVAL
    assert b"mc_export_maps" in lib.mc_last_error()

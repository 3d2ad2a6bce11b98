"""CPU: mc_frontier_actions without a device.

The library side: the three entry points are typed, refuse a null env by name
and leave the ABI version alone.  The test helper (tests/frontier_ref.py, what
the GPU tests compare the device with) against the oracle's own dijkstra obs
layer on a closed random walk.  The plain-C++ parts of the call
(csrc/mc_frontier.h: step codes, cell index -> (x, y), argument checks) in
tests/native/frontier_check.cpp, compiled host-only with AddressSanitizer and
UBSan and run as a child process."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from frontier_ref import ACT_STAY, action_from_layer, expected
from oracle.cpu_ref import DecGridRLRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def base_cfg(**kw):
    c = dict(numrobot=1, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0,
             terminal_reward=30, dist_reward=0, train_maxsteps=1000, test_maxsteps=1000,
             egoradius=2, mini_map_rad=0, comm_radius=0, allow_comm=0, map_sharing=0,
             single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
             sensor_config={"num_lasers": 21, "range": 10})
    c.update(kw)
    return c


@pytest.fixture(scope="module")
def lib():
    from marlcov import _lib
    return _lib.load()


def test_signatures_constants_and_version():
    import marlcov
    from marlcov import _lib
    from marlcov.episodes import frontier_policy
    vp = ctypes.c_void_p
    typed = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert typed["mc_frontier_setup"] == (ctypes.c_int, [vp])
    assert typed["mc_frontier_variant"] == (ctypes.c_char_p, [vp])
    assert typed["mc_frontier_actions"] == (ctypes.c_int, [vp, vp, vp, vp, vp])
    assert _lib.ABI_VERSION == 12
    assert _lib.ACT_STAY == 4 == ACT_STAY
    for name in ("frontier", "frontier_actions", "frontier_variant"):
        assert callable(getattr(marlcov.BatchCoverageEnv, name))
    assert callable(frontier_policy)


def test_null_env_is_refused_by_name(lib):
    from marlcov import _lib
    assert lib.mc_abi_version() == 12
    assert lib.mc_frontier_setup(None) == _lib.MC_EINVAL
    assert b"mc_frontier_setup: null env" in lib.mc_last_error()
    assert lib.mc_frontier_actions(None, None, None, None, None) == _lib.MC_EINVAL
    assert b"mc_frontier_actions: null env" in lib.mc_last_error()
    lib.mc_frontier_setup(None)  # (another message in between)
    assert lib.mc_frontier_variant(None) == b""
    assert b"mc_frontier_variant: null env" in lib.mc_last_error()


def test_frontier_policy_refuses_a_super_grid_env():
    from marlcov.episodes import frontier_policy

    class FakeSuper:  # what episodes.py tells a BatchSuperGridEnv by
        planes = object()

    with pytest.raises(ValueError, match="BatchSuperGridEnv"):
        frontier_policy(FakeSuper())


def test_helper_matches_the_oracles_own_obs_layer():
    """At every step of a 40-step random walk, the helper's action is the move
    that the oracle's obs layer 3 (the crop of the same path) shows next to the
    crop centre, and dist / goal describe the same path."""
    cfg = base_cfg(numrobot=3, dijkstra_input=1, egoradius=2, sensor_config={"num_lasers": 9, "range": 3})
    rs = np.random.RandomState(3)
    grid = rs.choice([1.0, -1.0], size=(22, 18), p=[0.85, 0.15])
    np.random.seed(3)
    ref = DecGridRLRef([grid], cfg)
    obs = ref.get_egocentric_observations()
    moves = 0
    for t in range(41):
        for i in range(3):
            act, dist, goal = expected(ref, i)
            assert act == action_from_layer(obs[i][3]), (t, i)
            assert (act == ACT_STAY) == (dist <= 0), (t, i)
            own = (ref._xinds[i], ref._yinds[i])
            l1 = abs(goal[0] - own[0]) + abs(goal[1] - own[1])
            assert (dist >= l1) if dist > 0 else (tuple(goal) == tuple(own)), (t, i, dist, goal, own)
            moves += act != ACT_STAY
        if t == 40:
            break
        obs, _, _ = ref.step(rs.randint(0, 5, size=3).astype(np.int64))
    assert moves > 60  # (of 123: the walk is about moves, not about STAY)


def test_native_parts_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host check cannot be built")
    exe = tmp_path / "frontier_check"
    # (host code only: the sanitizers go to the host compilation alone)
    cmd = [hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I",
           os.path.join(ROOT, "marl-coverage_amd", "csrc"), os.path.join(ROOT, "tests", "native", "frontier_check.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "steps 25"
    # every cell of the extended grid of a 37 x 45 map, ring included
    assert lines[1:4] == [f"pad {p} corners 4 cells {(37 + 2 * p) * (45 + 2 * p)}" for p in (0, 2, 5)]
    assert lines[4] == "checks 14" and lines[5] == "ok" and len(lines) == 6

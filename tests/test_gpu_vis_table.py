"""GPU: the lidar's marks read from the per-grid visibility table (csrc/
mc_vistab.h, mc_env_select.h EnvCfg::VISTAB) instead of marched.  Every case
steps against the oracle (oracle/cpu_ref.py) and compares reward (tolerance
0), done, obs, positions, maps and counters every step, once under
MARLCOV_VIS_TABLE=require (a handle without a table is an error, so the table
is what ran) and once under MARLCOV_VIS_TABLE=0 (the march).  The switches are
read at mc_create, so a case sets them before it builds its env."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_parity import base_cfg, bern, full_obs
from test_gpu_ray_program import border_grids, border_positions, reset_at, steps_vs_oracle
from test_gpu_shapes import run_against_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, L = 40, 33  # non-square: a swapped stride shows
MODES = ["require", "0"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def steps_with(torch, env, cfg, refs, actions, label):
    """The given [T][B][N] moves against the oracle envs ``refs``."""
    for t, acts in enumerate(actions):
        acts = np.ascontiguousarray(acts, dtype=np.uint8)
        obs, rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs_h, rew_h, done_h = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
        st = device_state(env)
        for b in range(env.num_envs):
            o, r, d = refs[b].step(ref_action(acts[b]))
            tag = f"{label} t={t} env {b}"
            assert float(r) == rew_h[b], (tag, float(r), rew_h[b])
            assert bool(d) == bool(done_h[b]), tag
            np.testing.assert_array_equal(obs_h[b], o, err_msg=tag + " obs")
            compare_env(st, b, refs[b], tag)
    env.check()


@pytest.mark.parametrize("mode", MODES)
def test_pool_of_three_grids_with_auto_resets(torch_cuda, monkeypatch, mode):
    """B = 5 (the last wave has an idle slot) on a pool of 3 grids with
    env_grid = [2, 0, 2, 1, 0]: the grid index picks the table's slice.
    maxsteps 7 over 20 steps, sentinel rows and no-op codes."""
    import marlcov
    monkeypatch.setenv("MARLCOV_VIS_TABLE", mode)
    cfg = base_cfg(numrobot=4, maxsteps=7)
    rs = np.random.RandomState(101)
    B = 5
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, W, L, 0.1) for _ in range(3)], auto_reset=True, seed=41,
                                   env_grid=[2, 0, 2, 1, 0])
    assert "<64,2,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    env.reset()
    resets = run_against_oracle(torch_cuda, env, cfg, rs, 20, list(range(B)), 41, f"pool {mode}")
    assert resets >= 2 * B


@pytest.mark.parametrize("mode", MODES)
def test_starts_in_corners_and_along_borders(torch_cuda, monkeypatch, mode):
    """Robots injected in all four corners and along each border: record rows
    and columns fall outside the map and into the last partial tile.  6 steps:
    everyone into the wall behind it, then towards each other, then random."""
    import marlcov
    monkeypatch.setenv("MARLCOV_VIS_TABLE", mode)
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(103)
    env = marlcov.BatchCoverageEnv(cfg, 3, grids=border_grids(rs, W, L, 3), auto_reset=True, seed=43)
    assert "<64,2,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch_cuda, env, cfg, border_positions(W, L))
    walls = np.array([[2, 2, 0, 0], [2, 0, 3, 1], [2, 3, 0, 1]], dtype=np.uint8)      # out of the map
    meet = np.array([[0, 0, 2, 2], [1, 1, 1, 3], [0, 1, 2, 3]], dtype=np.uint8)       # env 2: pairs onto one cell
    acts = [walls, meet, walls[:, ::-1]] + [rs.randint(0, 4, size=(3, 4)) for _ in range(3)]
    steps_with(torch_cuda, env, cfg, refs, acts, f"borders {mode}")


@pytest.mark.parametrize("mode", MODES + ["1"])
def test_beam_table_swaps_rebuild_the_table(torch_cuda, monkeypatch, mode):
    """Angles + 3 degrees (another table), 9 beams (the generic kernel: no
    table; `require` refuses the swap and the env keeps the table before it,
    the default and 0 march), the default 21 again."""
    import marlcov
    from marlcov import _lib
    from marlcov.sensors import beam_angles
    monkeypatch.setenv("MARLCOV_VIS_TABLE", mode)
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(107)
    B = 3
    env = marlcov.BatchCoverageEnv(cfg, B, grids=border_grids(rs, W, L, B), auto_reset=True, seed=47)
    pos = border_positions(W, L)
    rot = beam_angles(21) + np.deg2rad(3.0)
    swaps = [(rot, "<64,2,u32,C2>"), (beam_angles(9), "<64,2,u32,generic>"), (beam_angles(21), "<64,2,u32,C2>")]
    for i, (th, variant) in enumerate(swaps):
        if mode == "require" and len(th) == 9:
            with pytest.raises(_lib.MarlcovError, match="MARLCOV_VIS_TABLE=require"):
                env.sensor.set_thetalist(th)
            th, variant = rot, "<64,2,u32,C2>"  # the sensor put the angles before the swap back
        else:
            env.sensor.set_thetalist(th)
        assert variant in env.kernel_variant(), (i, env.kernel_variant())
        refs = reset_at(torch_cuda, env, cfg, pos, thetalist=th)
        steps_vs_oracle(torch_cuda, env, cfg, rs, refs, 6, f"swap {i} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_new_grids_after_five_steps(torch_cuda, monkeypatch, mode):
    """mc_set_grids with other grids after 5 steps, then a reset: the old
    pool's table must not be read."""
    import marlcov
    from marlcov import _lib
    from marlcov.batch_env import grid_to_int8, pad_grid
    torch = torch_cuda
    monkeypatch.setenv("MARLCOV_VIS_TABLE", mode)
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(109)
    B = 3
    env = marlcov.BatchCoverageEnv(cfg, B, grids=border_grids(rs, W, L, B), auto_reset=True, seed=53)
    pos = border_positions(W, L)
    refs = reset_at(torch, env, cfg, pos)
    steps_vs_oracle(torch, env, cfg, rs, refs, 5, f"old grids {mode}")
    host = np.stack([grid_to_int8(pad_grid(g)) for g in border_grids(rs, W, L, B)])
    dgrids = torch.from_numpy(host).to(env.device)
    _lib.check(env.lib.mc_set_grids(env._h, dgrids.data_ptr(), B, env._stream()), "mc_set_grids")
    refs = reset_at(torch, env, cfg, pos)  # (oracle envs on the device's new grids)
    np.testing.assert_array_equal(device_state(env)["neg"], (host < 0).astype(np.uint8))
    steps_vs_oracle(torch, env, cfg, rs, refs, 6, f"new grids {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_dijkstra_input_c2d(torch_cuda, monkeypatch, mode):
    import marlcov
    monkeypatch.setenv("MARLCOV_VIS_TABLE", mode)
    cfg = base_cfg(numrobot=4, dijkstra_input=1)
    rs = np.random.RandomState(113)
    env = marlcov.BatchCoverageEnv(cfg, 3, grids=border_grids(rs, W, L, 3), auto_reset=True, seed=59)
    assert "<64,2,u32,C2D>" in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch_cuda, env, cfg, border_positions(W, L))
    steps_vs_oracle(torch_cuda, env, cfg, rs, refs, 8, f"c2d {mode}")


def _one_env_per_workgroup():
    """(child process, MARLCOV_EPW=1) <64,1,u32,C2>: lanes 0 .. 31 of the 64
    land the four records."""
    import marlcov
    import torch
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(127)
    env = marlcov.BatchCoverageEnv(cfg, 3, grids=border_grids(rs, W, L, 3), auto_reset=True, seed=61)
    assert "<64,1,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch, env, cfg, border_positions(W, L))
    steps_vs_oracle(torch, env, cfg, rs, refs, 8, "epw1")
    print("epw1 ok")


@pytest.mark.parametrize("mode", MODES)
def test_one_env_per_workgroup(torch_cuda, mode):
    """MARLCOV_EPW=1 is read once per process, so the case runs in a child
    process of its own."""
    env = dict(os.environ, MARLCOV_EPW="1", MARLCOV_VIS_TABLE=mode)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "epw1 ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_size_cap_falls_back_to_the_march(torch_cuda, monkeypatch):
    """MARLCOV_VIS_TABLE_MB=0: no pool fits.  `require` says so; the default
    marches and matches the oracle."""
    import marlcov
    from marlcov import _lib
    monkeypatch.setenv("MARLCOV_VIS_TABLE_MB", "0")
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(131)
    grids = border_grids(rs, W, L, 3)
    monkeypatch.setenv("MARLCOV_VIS_TABLE", "require")
    with pytest.raises(_lib.MarlcovError, match="MARLCOV_VIS_TABLE_MB"):
        marlcov.BatchCoverageEnv(cfg, 3, grids=grids, auto_reset=True, seed=67)
    monkeypatch.delenv("MARLCOV_VIS_TABLE")
    env = marlcov.BatchCoverageEnv(cfg, 3, grids=grids, auto_reset=True, seed=67)
    assert "<64,2,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch_cuda, env, cfg, border_positions(W, L))
    steps_vs_oracle(torch_cuda, env, cfg, rs, refs, 6, "cap 0")


@pytest.mark.parametrize("mode", MODES)
def test_fork_within_a_batch_and_to_a_sibling(torch_cuda, monkeypatch, mode):
    """A fork inside the batch, then into a sibling() (which copies the pool
    and builds a table of its own): two steps on each side."""
    import marlcov
    torch = torch_cuda
    monkeypatch.setenv("MARLCOV_VIS_TABLE", mode)
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(137)
    B = 4
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, W, L, 0.1) for _ in range(B)], auto_reset=False, seed=71)
    env.reset()
    for _ in range(3):
        env.step(torch.from_numpy(rs.randint(0, 4, size=(B, 4)).astype(np.uint8)).to(env.device))
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    # envs 1 and 3 become env 0; their grids differ from env 0's, so they take env 0's grid index along
    src = [-1, 0, -1, 0]
    env.fork(np.asarray(src, dtype=np.int32))
    env.check()
    refs = [refs[b] if s < 0 else copy.deepcopy(refs[s]) for b, s in enumerate(src)]
    steps_with(torch, env, cfg, refs, [rs.randint(0, 4, size=(B, 4)) for _ in range(2)], f"fork {mode}")
    sib = env.sibling(B)
    sib.fork(np.arange(B, dtype=np.int32)[::-1].copy(), source=env)
    sib.check()
    srefs = [copy.deepcopy(refs[B - 1 - b]) for b in range(B)]
    steps_with(torch, sib, cfg, srefs, [rs.randint(0, 4, size=(B, 4)) for _ in range(2)], f"sibling {mode}")
    steps_with(torch, env, cfg, refs, [rs.randint(0, 4, size=(B, 4)) for _ in range(2)], f"after sibling {mode}")


if __name__ == "__main__":
    _one_env_per_workgroup()

"""GPU: the visibility table's records stored as map tiles (csrc/mc_vistab.h
vis_tiles, mc_env_step.h vis_items_load / vis_items_land): every (agent,
tile) item of the step kernel loads its own tile of the record of its robot's
post-move cell, and a reset's initial sense reads the table the same way.
Every case asserts kernel_variant() first and runs under
MARLCOV_VIS_TABLE=require (a handle without a table is an error, so the table
is what ran); every comparison is bitwise / tolerance 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import device_state
from test_gpu_fused_steps import actions, fused_vs_stepped, launches, pair, set_knobs
from test_gpu_parity import base_cfg, bern
from test_gpu_ray_program import reset_at
from test_gpu_vis_table import steps_with

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, L = 40, 33  # non-square: a swapped stride shows
H = 10         # base_cfg's lidar: range 10


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def residue_positions():
    """[8, 4, 2] start cells (padded coordinates).  Over the 8 envs (x - H) & 7
    and (y - H) & 7 of each of robots 0 .. 2 take all 8 values; robot 3 stands
    3 cells from robot 2 in the same row, for the head-on moves."""
    pos = np.zeros((8, 4, 2), dtype=np.int32)
    for b in range(8):
        for i in range(3):
            pos[b, i] = (8 + b + 7 * i, 6 + (3 * b + i) % 8 + 6 * i)
        pos[b, 3] = (pos[b, 2, 0], pos[b, 2, 1] + 3)
    for i in range(3):
        assert {(int(x) - H) & 7 for x in pos[:, i, 0]} == set(range(8))
        assert {(int(y) - H) & 7 for y in pos[:, i, 1]} == set(range(8))
    assert pos[:, :, 0].min() >= 3 and pos[:, :, 0].max() + 2 <= W
    assert pos[:, :, 1].min() >= 2 and pos[:, :, 1].max() + 1 <= L
    return pos


def residue_grids(rs, pos):
    """One Bernoulli grid per env with the cells the scripted moves use free and
    a wall two cells ahead of robot 0 (+x) and of robot 1 (-x)."""
    grids = []
    for b in range(len(pos)):
        g = bern(rs, W, L, 0.1)
        for i in range(4):
            x, y = int(pos[b, i, 0]) - 1, int(pos[b, i, 1]) - 1  # (the grid is padded by one cell)
            g[x - 1:x + 2, y - 1:y + 2] = 1.0
        x, y = int(pos[b, 2, 0]) - 1, int(pos[b, 2, 1]) - 1
        g[x - 1:x + 2, y - 1:y + 5] = 1.0  # between robots 2 and 3
        g[int(pos[b, 0, 0]) - 1 + 2, int(pos[b, 0, 1]) - 1] = -1.0
        g[int(pos[b, 1, 0]) - 1 - 2, int(pos[b, 1, 1]) - 1] = -1.0
        grids.append(g)
    return grids


def residues_case(torch, variant):
    import marlcov
    from marlcov import _lib
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(1401)
    pos = residue_positions()
    B = len(pos)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=residue_grids(rs, pos), auto_reset=True, seed=83)
    assert variant in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch, env, cfg, pos)
    every = lambda a: np.full((B, 4), a, dtype=np.uint8)
    # up, down, left, right: every robot moves, so ox - bx and oy - by take 0 and 1
    steps_with(torch, env, cfg, refs, [every(0), every(2), every(1), every(3)], "tiles moves")
    np.testing.assert_array_equal(env.get_state(_lib.FIELD_POS).cpu().numpy(), pos)
    # robot 0 towards its wall (+x), robot 1 towards its wall (-x), robots 2 and 3 towards each other
    ahead = np.tile(np.array([0, 2, 1, 3], dtype=np.uint8), (B, 1))
    steps_with(torch, env, cfg, refs, [ahead], "tiles ahead")
    p1 = env.get_state(_lib.FIELD_POS).cpu().numpy()
    assert (np.abs(p1 - pos).sum(axis=2) == 1).all()
    # ... and again, twice: into the walls and into each other -- every robot keeps its cell
    steps_with(torch, env, cfg, refs, [ahead, ahead], "tiles blocked")
    np.testing.assert_array_equal(env.get_state(_lib.FIELD_POS).cpu().numpy(), p1)
    steps_with(torch, env, cfg, refs, [rs.randint(0, 4, size=(B, 4))], "tiles random")


def test_residues_and_block_offsets(torch_cuda, monkeypatch):
    """8 envs x 4 robots injected at every (x - H) & 7 and (y - H) & 7; four
    steps that move every robot up, down, left and right, four more into walls
    and into each other; against the oracle every step."""
    monkeypatch.setenv("MARLCOV_VIS_TABLE", "require")
    residues_case(torch_cuda, "<64,2,u32,C2>")


def test_table_against_march_at_every_cell(torch_cuda, monkeypatch):
    """A pool of two maps; every free cell is once robot 0's injected start
    (one env per cell).  One reset under `require` and one under
    MARLCOV_VIS_TABLE=0: the reset's initial sense from the table against the
    march, maps and counters bitwise."""
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(1402)
    grids = [bern(rs, W, L, 0.1) for _ in range(2)]
    spare = [(1, 1), (1, L), (W, 1), (W, L)]  # (padded) cells for robots 1 .. 3: the corners, kept free
    for g in grids:
        for x, y in spare:
            g[x - 1, y - 1] = 1.0
    pos, env_grid = [], []
    for gi, g in enumerate(grids):
        for x, y in zip(*np.nonzero(g > 0)):
            c = (int(x) + 1, int(y) + 1)
            pos.append([c] + [s for s in spare if s != c][:3])
            env_grid.append(gi)
    pos = np.asarray(pos, dtype=np.int32)
    B = len(pos)
    assert B == sum(int((g > 0).sum()) for g in grids) and B > 2000
    fields = [_lib.FIELD_FREE, _lib.FIELD_OBST, _lib.FIELD_VISITED, _lib.FIELD_FREE_COUNT, _lib.FIELD_VISITED_COUNT,
              _lib.FIELD_POS]
    got = {}
    for mode in ("require", "0"):
        monkeypatch.setenv("MARLCOV_VIS_TABLE", mode)
        env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=True, seed=89, env_grid=env_grid)
        assert "<64,2,u32,C2>" in env.kernel_variant(), env.kernel_variant()
        env.reset(positions=pos)
        env.check()
        got[mode] = [env.get_state(f).cpu().numpy() for f in fields]
        del env
    np.testing.assert_array_equal(got["require"][5], pos)
    assert int(got["0"][3].min()) > 0  # every env sensed something
    for f, a, b in zip(fields, got["require"], got["0"]):
        assert a.tobytes() == b.tobytes(), f"state field {f}: the table's reset differs from the march's"


def test_reset_inside_a_fused_launch(torch_cuda, monkeypatch):
    """maxsteps 3, B = 5 (an idle slot), K = 10 through `rollout` (one launch)
    against K `step` calls and the oracle: every env resets inside the launch
    and reset_env's sense reads the table."""
    s = set_knobs(monkeypatch, "require", None)
    cfg = base_cfg(numrobot=4, maxsteps=3)
    rs = np.random.RandomState(1403)
    B, K = 5, 10
    envs = pair(cfg, [bern(rs, W, L, 0.1) for _ in range(B)], B, auto_reset=True, seed=97)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2>", envs[0].kernel_variant()
    assert launches(K, s) == 1
    done = fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 4), 1, "tiles fused resets", cfg, oracle=True)
    assert int(done.sum()) >= 3 * B


def _one_env_per_workgroup():
    """(child process, MARLCOV_EPW=1) <64,1,u32,C2>: one item per lane."""
    import torch
    residues_case(torch, "<64,1,u32,C2>")
    print("epw1 ok")


def test_one_env_per_workgroup(torch_cuda):
    """MARLCOV_EPW=1 is read once per process, so the case runs in a child
    process of its own."""
    env = dict(os.environ, MARLCOV_EPW="1", MARLCOV_VIS_TABLE="require")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "epw1 ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    _one_env_per_workgroup()

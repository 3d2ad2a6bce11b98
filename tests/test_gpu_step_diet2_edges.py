"""GPU: the carried C2 table kernels' edge clip from two masks (edge_clip,
mc_internal.h; store_tiles) and their record addresses in a pool of several
grids (vis_items_load, vis_prefetch), against the oracle after every step
(test_gpu_union_dedup.walk_vs_oracle).

Edge cases: maps whose padded sides leave 1, 2, 3, 6 and 7 valid cells (and a
whole tile) in the last tile row or column -- 19 x 26, 24 x 25, 17 x 17 and
22 x 23 padded cells on the general ShapeC2V kernel, 130 x 130 on the bench
row ShapeC2BV -- with obstacles, so that obstacle marks fall in the last two
tile rows and columns, and robots that walk along the bottom border, the
right border and in the corner.

Pool cases: a pool of 3 different grids with the envs on grids 0, 2 and 2 and
a robot on the pool's last free cell (the last cell of the table itself is a
border cell, where no robot stands); with an in-step auto-reset every third
step and with a sentinel step, both with reset_grid_mode "random", so that the
step after a reset has to address the records of another grid.

Mutants of the new code run against this file: see
tests/test_gpu_union_dedup.py."""
import numpy as np
import pytest

from test_gpu_carried_head import TABLE_ROW
from test_gpu_fused_steps import actions, c2_cfg, launches, pair, set_knobs
from test_gpu_parity import bern
from test_gpu_union_dedup import walk_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def border_case(rs, Wp, Lp):
    """A padded Wp x Lp map with obstacles and free lanes along the bottom row
    (x = Wp - 2) and the right column (y = Lp - 2), the four starts and a
    script: robot 0 walks the bottom border, robot 1 the right border, robot 2
    steps around the corner, robot 3 stays near the origin."""
    g = bern(rs, Wp - 2, Lp - 2, 0.15)
    g[-1, :] = g[:, -1] = g[-2, -2] = 1.0
    g[0, :2] = 1.0
    start = [(Wp - 2, 1), (1, Lp - 2), (Wp - 3, Lp - 3), (1, 1)]
    script = [(1, 0, 0, 1), (1, 0, 1, 4), (1, 0, 2, 3), (1, 0, 3, 4), (3, 2, 1, 1), (3, 2, 0, 3)]
    return g, start, script


@pytest.mark.parametrize("S", [None, 1])
@pytest.mark.parametrize("Wp,Lp", [(19, 26), (24, 25), (17, 17), (22, 23)])
def test_edge_tiles_general_row(torch_cuda, monkeypatch, Wp, Lp, S):
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(100 * Wp + Lp)
    g, start, script = border_case(rs, Wp, Lp)
    acts0 = np.asarray(script, dtype=np.uint8)
    B, K = 3, len(acts0)
    acts = np.stack([np.roll(acts0, -b, axis=0) for b in range(B)], axis=1)
    envs = pair(cfg, [g.copy() for _ in range(B)], B, auto_reset=False, seed=92)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2>", envs[0].kernel_variant()
    for e in envs:
        e.reset(positions=np.asarray([start] * B, dtype=np.int32))
    walk_vs_oracle(torch_cuda, envs, acts, cfg, False, f"edges {Wp}x{Lp} S={S}", launches(K, s))


@pytest.mark.parametrize("S", [None, 1])
def test_edge_tiles_bench_row(torch_cuda, monkeypatch, S):
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(130)
    g, start, script = border_case(rs, 130, 130)
    acts0 = np.asarray(script, dtype=np.uint8)
    B, K = 3, len(acts0)
    acts = np.stack([np.roll(acts0, -b, axis=0) for b in range(B)], axis=1)
    envs = pair(cfg, [g.copy() for _ in range(B)], B, auto_reset=True, seed=93)
    assert envs[0].kernel_label() == "64,2,uint32_t,ShapeC2BV", envs[0].kernel_label()
    for e in envs:
        e.reset(positions=np.asarray([start] * B, dtype=np.int32))
    walk_vs_oracle(torch_cuda, envs, acts, cfg, True, f"edges bench row S={S}", launches(K, s))


def pool(rs):
    """three different 24 x 22 grids (padded 26 x 24) whose last free cell is free"""
    gs = [bern(rs, 24, 22, 0.12) for _ in range(3)]
    for g in gs:
        g[-1, -3:] = g[-3:, -1] = g[0, 0] = 1.0
    return gs


@pytest.mark.parametrize("S", [None, 1])
def test_pool_last_cell(torch_cuda, monkeypatch, S):
    """envs on grids 0, 2, 2; robot 0 of every env starts on the pool's last
    free cell (25 - 1, 23 - 1 of grid 2: the record before the table's last
    border row) and walks away and back."""
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(2101)
    B = 3
    envs = pair(cfg, pool(rs), B, auto_reset=False, seed=94, env_grid=[0, 2, 2])
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    start = [(24, 22), (24, 20), (22, 22), (1, 1)]
    script = [(3, 2, 2, 4), (2, 3, 3, 4), (0, 1, 1, 4), (1, 0, 0, 4), (4, 4, 4, 4), (3, 3, 3, 4)]
    acts0 = np.asarray(script, dtype=np.uint8)
    K = len(acts0)
    acts = np.stack([np.roll(acts0, -b, axis=0) for b in range(B)], axis=1)
    for e in envs:
        e.reset(positions=np.asarray([start] * B, dtype=np.int32))
    _, st = walk_vs_oracle(torch_cuda, envs, acts, cfg, False, f"pool last cell S={S}", launches(K, s))
    assert st["env_grid"].tolist() == [0, 2, 2]


@pytest.mark.parametrize("S", [None, 1])
def test_pool_resets(torch_cuda, monkeypatch, S):
    """maxsteps 3, K = 8: every env resets inside the launch, twice, and draws
    its grid anew at every reset (reset_grid_mode "random")"""
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=3)
    rs = np.random.RandomState(2102)
    B, K = 3, 8
    envs = pair(cfg, pool(rs), B, auto_reset=True, seed=95, env_grid=[0, 2, 2], reset_grid_mode="random")
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    acts = actions(rs, K, B, 4, sentinel_p=0.0)
    done, st = walk_vs_oracle(torch_cuda, envs, acts, cfg, True, f"pool resets S={S}", launches(K, s), regrid=True)
    assert int(done.sum()) >= 2 * B
    assert st["env_grid"].tolist() != [0, 2, 2]  # some reset changed a grid


@pytest.mark.parametrize("S", [None, 1])
@pytest.mark.parametrize("auto_reset", [True, False])
def test_pool_sentinel(torch_cuda, monkeypatch, auto_reset, S):
    """agent 0's byte 255 for env 1 at step 2 and env 2 at step 4"""
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(2103 + auto_reset)
    B, K = 3, 7
    envs = pair(cfg, pool(rs), B, auto_reset=auto_reset, seed=96, env_grid=[0, 2, 2], reset_grid_mode="random")
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    acts = actions(rs, K, B, 4, sentinel_p=0.0)
    acts[2, 1, 0] = acts[4, 2, 0] = 255
    done, _ = walk_vs_oracle(torch_cuda, envs, acts, cfg, auto_reset, f"pool sentinel {auto_reset} S={S}",
                             launches(K, s), regrid=True)
    assert done[2, 1] and done[4, 2]

"""GPU: the visibility-record tiles the fused step loop loads a step ahead
(mc_env_step.h: VisK, vis_prefetch; EnvCfg::CARRY, the one-wave table kernels of
the C2 shapes).  Step k predicts every robot's cell after step k + 1 from its
own target's grid bit alone and loads the items' tiles of those cells' records;
step k + 1 takes them when its wave carries its head and the moves gave every
item's robot the predicted cell, and loads as before otherwise.  So the cases
script every way a prediction goes wrong (robots in each other's way), cross
the tile borders that move a block's and a record's origin, reset and end
launches where prefetched words must not count, run the kernels' other rows,
and run twelve steps in which every prediction is right.

Every case compares, at every step, the reward's bits, done and every obs
layer of the fused rollout with K step calls of a twin env and with the
oracle, and after the call the full device state (ep_pc and ep_len included)
with the twin's and the oracle's (test_gpu_carried_head's comparison)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.cpu_ref import DecGridRLRef
from test_gpu_carried_head import TABLE_ROW, rollout_vs_stepped_vs_oracle
from test_gpu_fused_steps import DEFAULT_S, actions, assert_same_state, c2_cfg, launches, pair, set_knobs
from test_gpu_parity import bern

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 10  # the C2 lidar's range: a record's origin tile is ((x - H) >> 3, (y - H) >> 3)
DX, DY = (1, 0, -1, 0), (0, 1, 0, -1)  # action bytes 0..3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def oracle_walk(cfg, inner, start, acts):
    """The oracle's cells (padded coordinates) before the first and after every
    step of one env's script acts[K][N]: [K + 1][N][2].  (Four lidars cover
    these small maps within a step or two -- percent_covered sums the robots'
    maps -- so the scripted cases run without auto-reset: a covered env keeps
    stepping, done in every step, and the script keeps its cells.)"""
    np.random.seed(0)
    ref = DecGridRLRef([inner], cfg)
    ref.reset(False, None, positions=[tuple(p) for p in start])
    cells = [list(zip(ref._xinds.tolist(), ref._yinds.tolist()))]
    for a in acts:
        ref.step(np.asarray(a, dtype=np.int64))
        cells.append(list(zip(ref._xinds.tolist(), ref._yinds.tolist())))
    return np.asarray(cells), ref._grid.copy()


# ---- 1. scripted mispredictions on an authored map -------------------------
# 18 x 18 free cells (padded 20 x 20: cells 1..18 a side) and one wall cell at
# padded (11, 10).  Cells after each step, robots 0..3:
MIS_START = [(1, 1), (18, 18), (9, 9), (9, 11)]
MIS_SCRIPT = [
    # actions           what the step is for
    (2, 0, 1, 3),     # 0 off the map at x = 0, 1 at x = 19; 2 and 3 both move into (9, 10): 3 fails
    (3, 1, 0, 3),     # 0 off the map at y = 0, 1 at y = 19; 3 enters (9, 10), which 2 left in this step
    (4, 200, 2, 3),   # bytes 4 and 200; 2 moves into 3's cell (9, 10) before 3 moves away: 2 fails
    (0, 2, 0, 4),     # 2 moves into the wall at (11, 10)
    (0, 2, 1, 0),     # plain moves: the step after a misprediction predicts again
    (1, 3, 1, 0),
    (1, 3, 2, 1),
    (0, 2, 3, 1),
]


def mis_grid():
    g = np.ones((18, 18))
    g[10, 9] = -1.0  # padded (11, 10)
    return g


def script_events(cells, grid, acts):
    """The kinds of events of a script, from the oracle's cells alone."""
    Wp, Lp = grid.shape
    ev = set()
    for k, a in enumerate(acts):
        P, Q = cells[k], cells[k + 1]
        tgt = [(int(P[i][0]) + DX[b], int(P[i][1]) + DY[b]) if b <= 3 else None for i, b in enumerate(a)]
        for i, b in enumerate(a):
            if b > 3:
                ev.add(f"byte {b}")
                assert tuple(Q[i]) == tuple(P[i])
                continue
            t, stayed = tgt[i], tuple(Q[i]) == tuple(P[i])
            assert stayed or tuple(Q[i]) == t
            for name, hit in (("x low", t[0] == 0), ("x high", t[0] == Wp - 1), ("y low", t[1] == 0),
                              ("y high", t[1] == Lp - 1)):
                if hit and stayed:
                    ev.add("off the map " + name)
            if stayed and 0 < t[0] < Wp - 1 and 0 < t[1] < Lp - 1 and grid[t] < 0:
                ev.add("obstacle")
            for j in range(len(a)):
                if j == i:
                    continue
                moved_j = tuple(Q[j]) != tuple(P[j])
                if j < i and tgt[j] == t and moved_j and stayed and tuple(P[j]) != t:
                    ev.add("same cell")  # a lower robot took the cell in this step
                if j < i and tuple(P[j]) == t and moved_j and not stayed:
                    ev.add("vacated by a lower robot")
                if j > i and tuple(P[j]) == t and moved_j and stayed:
                    ev.add("higher robot still there")
    return ev


MIS_EVENTS = {"same cell", "vacated by a lower robot", "higher robot still there", "obstacle", "off the map x low",
              "off the map x high", "off the map y low", "off the map y high", "byte 4", "byte 200"}


def test_scripted_mispredictions(torch_cuda, monkeypatch):
    """B = 2, K = 8 in one launch.  Env 0 plays MIS_SCRIPT, env 1 the same
    script one step late (a no-op first), so the two slots of the wave
    mispredict at different steps.  Asserted from the oracle's cells: the
    script holds every kind of event the prefetch has to survive."""
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    acts0 = np.asarray(MIS_SCRIPT, dtype=np.uint8)
    cells, grid = oracle_walk(cfg, mis_grid(), MIS_START, acts0)
    assert grid.shape == (20, 20)
    assert script_events(cells, grid, acts0) == MIS_EVENTS, script_events(cells, grid, acts0)
    B, K = 2, len(acts0)
    acts = np.empty((K, B, 4), dtype=np.uint8)
    acts[:, 0] = acts0
    acts[0, 1], acts[1:, 1] = 4, acts0[:-1]
    envs = pair(cfg, [mis_grid() for _ in range(B)], B, auto_reset=False, seed=71)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    for e in envs:
        e.reset(positions=np.asarray([MIS_START] * B, dtype=np.int32))
    _, _, done, st = rollout_vs_stepped_vs_oracle(torch_cuda, envs, acts, cfg, False, "mispredictions", 1)
    np.testing.assert_array_equal(st["pos"][0], cells[K])
    np.testing.assert_array_equal(st["pos"][1], cells[K - 1])


# ---- 2. tile-border crossings ----------------------------------------------
# 22 x 24 free cells (padded 24 x 26).  Robot 0 walks x = 9, 10, 11 and then
# y = 9, 10, 11: the record's origin tile changes at 10 and the block's at 11;
# robot 1 the same around 17 .. 19 and back; robots 2 and 3 along the corners,
# where most of a block lies outside the map and items outside the record.
CROSS_START = [(9, 9), (17, 17), (1, 1), (22, 24)]
CROSS_SCRIPT = [(0, 0, 1, 2), (0, 0, 1, 3), (1, 1, 0, 2), (1, 1, 0, 3), (2, 2, 3, 0), (2, 3, 2, 1), (3, 3, 1, 0),
                (3, 2, 0, 1)]


def test_tile_border_crossings(torch_cuda, monkeypatch):
    """B = 3 (an idle second slot in the second wave), K = 8 in one launch:
    env b plays the script from step b on, so the waves' slots cross at
    different steps."""
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    acts0 = np.asarray(CROSS_SCRIPT, dtype=np.uint8)
    cells, grid = oracle_walk(cfg, np.ones((22, 24)), CROSS_START, acts0)
    assert grid.shape == (24, 26)
    for r in (0, 1):  # in consecutive steps: the record's origin tile, then the block's, in x and in y
        for ax in (0, 1):
            c = cells[:, r, ax]
            rec, blk = (c - H) >> 3, (c - H - 1) >> 3
            assert any(rec[k] != rec[k + 1] and blk[k + 1] != blk[k + 2] for k in range(len(c) - 2)), (r, ax, c)
    assert (np.abs(np.diff(cells, axis=0)).sum(axis=2) == 1).all()  # every move succeeds: every prediction is right
    assert (cells[:, 2:] <= H).any() and (cells[:, 3, 0] >= 24 - H).all()  # within H of the map's edge
    B, K = 3, len(acts0)
    acts = np.stack([np.roll(acts0, -b, axis=0) for b in range(B)], axis=1)
    envs = pair(cfg, [np.ones((22, 24)) for _ in range(B)], B, auto_reset=False, seed=72)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    for e in envs:
        e.reset(positions=np.asarray([CROSS_START] * B, dtype=np.int32))
    _, _, done, st = rollout_vs_stepped_vs_oracle(torch_cuda, envs, acts, cfg, False, "tile borders", 1)
    np.testing.assert_array_equal(st["pos"][0], cells[K])


# ---- 3. resets and chunk boundaries ----------------------------------------
@pytest.mark.parametrize("S", [2, 3, None])
def test_maxsteps_resets_and_launch_ends(torch_cuda, monkeypatch, S):
    """B = 3, maxsteps 3, K = 7 in launches of 2, 3 and 64 steps: a reset in a
    loop step, in a launch's last step (nothing is prefetched there) and in
    step 0; the second wave's second slot is idle in every step."""
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=3)
    rs = np.random.RandomState(2011)
    B, K = 3, 7
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=73)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    acts = actions(rs, K, B, 4, sentinel_p=0.0)
    assert launches(K, s) == {2: 4, 3: 3, None: 1}[S]
    _, _, done, _ = rollout_vs_stepped_vs_oracle(torch_cuda, envs, acts, cfg, True, f"maxsteps 3 S={S}",
                                                 launches(K, s))
    assert int(done.sum()) >= 2 * B


@pytest.mark.parametrize("auto_reset", [True, False])
def test_sentinels(torch_cuda, monkeypatch, auto_reset):
    """B = 3, K = 8 in one launch: agent 0's byte 255 for env 0 at step 2 and
    env 1 at step 5, with auto-reset (the slot resets: its prefetched tiles are
    of the finished episode) and without (the slot takes the obs-only path and
    its wave loads in the step after)."""
    assert set_knobs(monkeypatch, "require", None) == DEFAULT_S
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(2012 + auto_reset)
    B, K = 3, 8
    envs = pair(cfg, [bern(rs, 22, 24, 0.12) for _ in range(B)], B, auto_reset=auto_reset, seed=74)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    acts = actions(rs, K, B, 4, sentinel_p=0.0)
    acts[2, 0, 0] = acts[5, 1, 0] = 255
    _, _, done, _ = rollout_vs_stepped_vs_oracle(torch_cuda, envs, acts, cfg, auto_reset, f"sentinels {auto_reset}", 1)
    done = done.cpu().numpy().astype(bool)
    assert done[2, 0] and done[5, 1]


def test_state_written_between_two_calls(torch_cuda, monkeypatch):
    """Four fused steps, then the robots of env 0 are put on other cells by
    set_state (both twins), then four more: nothing prefetched by the first
    call's last steps reaches the second call."""
    from marlcov import _lib
    torch = torch_cuda
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(2021)
    B = 2
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=75)
    rollout_vs_stepped_vs_oracle(torch, envs, actions(rs, 4, B, 4, sentinel_p=0.0), cfg, True, "before the write", 1)
    pos = envs[0].get_state(_lib.FIELD_POS).cpu().numpy()
    new = pos.copy()
    new[0] = np.roll(pos[0], 1, axis=0)  # env 0: robot i on robot i - 1's cell
    assert (new[0] != pos[0]).any()
    for e in envs:
        e.set_state(_lib.FIELD_POS, torch.from_numpy(new))
    st = assert_same_state(envs[0], envs[1], "after the write")
    np.testing.assert_array_equal(st["pos"], new)
    rollout_vs_stepped_vs_oracle(torch, envs, actions(rs, 4, B, 4, sentinel_p=0.0), cfg, True, "after the write", 1)


# ---- 4. kernel rows ---------------------------------------------------------
def test_the_bench_row(torch_cuda, monkeypatch):
    """128 x 128 maps, B = 3, K = 10 in one launch: the row bench.py's default
    line times; random moves at an obstacle density that blocks some."""
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(2031)
    B, K = 3, 10
    envs = pair(cfg, [bern(rs, 128, 128, 0.1) for _ in range(B)], B, auto_reset=True, seed=76)
    assert envs[0].kernel_label() == "64,2,uint32_t,ShapeC2BV", envs[0].kernel_label()
    rollout_vs_stepped_vs_oracle(torch_cuda, envs, actions(rs, K, B, 4, sentinel_p=0.0), cfg, True, "bench row", 1)


def _child_epw1():
    """MARLCOV_EPW=1: one env per workgroup.  The misprediction script at B = 2
    and a maxsteps-3 rollout with resets at B = 3."""
    import torch
    cfg = dict(c2_cfg(), maxsteps=1000)
    acts0 = np.asarray(MIS_SCRIPT, dtype=np.uint8)
    B, K = 2, len(acts0)
    acts = np.stack([acts0, np.roll(acts0, 1, axis=0)], axis=1)
    envs = pair(cfg, [mis_grid() for _ in range(B)], B, auto_reset=False, seed=77)
    assert envs[0].kernel_label() == "64,1,uint32_t,ShapeC2V", envs[0].kernel_label()
    for e in envs:
        e.reset(positions=np.asarray([MIS_START] * B, dtype=np.int32))
    rollout_vs_stepped_vs_oracle(torch, envs, acts, cfg, False, "epw 1 mispredictions", 1)
    cfg = dict(c2_cfg(), maxsteps=3)
    rs = np.random.RandomState(2041)
    B, K = 3, 7
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=78)
    rollout_vs_stepped_vs_oracle(torch, envs, actions(rs, K, B, 4, sentinel_p=0.0), cfg, True, "epw 1 maxsteps 3", 1)


def test_one_env_per_workgroup(torch_cuda):
    """MARLCOV_EPW is read once per process: a child process."""
    env = dict(os.environ, MARLCOV_EPW="1", MARLCOV_VIS_TABLE="require")
    env.pop("MARLCOV_FUSE_STEPS", None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "epw1 ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ---- 5. the no-gain path ----------------------------------------------------
def test_every_prediction_right(torch_cuda, monkeypatch):
    """B = 2, K = 12 in one launch on an empty map: the robots walk along
    free rows, every move succeeds (asserted from the oracle's cells), so
    eleven steps in a row take the prefetched tiles; one fused launch ran."""
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    start = [(2, 2), (2, 21), (19, 2), (19, 21)]
    acts0 = np.asarray([(0, 3, 1, 2)] * 6 + [(1, 0, 2, 3)] * 6, dtype=np.uint8)
    cells, _ = oracle_walk(cfg, np.ones((22, 24)), start, acts0)
    assert (np.abs(np.diff(cells, axis=0)).sum(axis=2) == 1).all()
    B, K = 2, len(acts0)
    assert K == 12
    acts = np.stack([acts0] * B, axis=1)
    envs = pair(cfg, [np.ones((22, 24)) for _ in range(B)], B, auto_reset=False, seed=79)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    for e in envs:
        e.reset(positions=np.asarray([start] * B, dtype=np.int32))
    _, _, done, st = rollout_vs_stepped_vs_oracle(torch_cuda, envs, acts, cfg, False, "every prediction right", 1)
    assert st["currstep"].tolist() == [K] * B
    np.testing.assert_array_equal(st["pos"][0], cells[K])


if __name__ == "__main__":
    _child_epw1()
    print("epw1 ok")

"""GPU: the fused step loop's carried lane constants (mc_env_step.h: LaneK,
ObsRoles; EnvCfg::LANEK), its kernel arguments re-read at the phase
boundaries, and the tile index kept from stage_load to store_tiles
(EnvCfg::KEEP_GT).  What the loop carries depends on the lane, the workgroup
and the launch's shape alone, so the cases vary exactly those: a wave whose
second slot is idle for the whole launch (B = 1), chunk boundaries, resets and
sentinels inside a launch, one env per workgroup, the bench row.  The obs
lanes' roles are among the carried constants, so one case scripts the moves --
vacated cells, blocked cells, a wall, the map's edge, no-ops and a robot that
never moves -- and compares every obs layer, the reward's bits and done with
the oracle at every step of one fused launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import device_state, oracle_from_device, ref_action
from test_gpu_fused_steps import (DEFAULT_S, actions, assert_same_state, c2_cfg, fused_vs_stepped, launches, pair,
                                  set_knobs)
from test_gpu_parity import bern

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


# seeds whose K = 5 action rows hold a sentinel after step 0 at 8 % (checked
# below): a sentinel's obs-only / reset path then runs in the loop copy
SLOT_SEEDS = {1: 1603, 2: 1602, 3: 1602}


@pytest.mark.parametrize("S", [2, None])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_slots_chunks_resets_and_sentinels(torch_cuda, monkeypatch, B, S):
    """The C2 table shape on 24 x 22 maps, K = 5 in chunks of 2, 2, 1 (S = 2)
    and in one launch (default S); maxsteps 3, so every env resets inside the
    loop copy; B = 1 leaves the wave's second slot idle in every step, B = 3
    the second wave's.  Fused against stepped and against the oracle."""
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=3)
    rs = np.random.RandomState(SLOT_SEEDS[B])
    K = 5
    grids = [bern(rs, 24, 22, 0.12) for _ in range(B)]
    acts = actions(rs, K, B, 4)
    assert (acts[1:, :, 0] == 255).any(), "no sentinel after step 0: pick another seed"
    envs = pair(cfg, grids, B, auto_reset=True, seed=31 + B)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2>", envs[0].kernel_variant()
    assert envs[0].kernel_label() == "64,2,uint32_t,ShapeC2V", envs[0].kernel_label()
    assert launches(K, s) == (3 if S == 2 else 1) and s == (2 if S == 2 else DEFAULT_S)
    done = fused_vs_stepped(torch_cuda, envs, acts, launches(K, s), f"diet slots B={B} S={S}", cfg, oracle=True)
    assert int(done.sum()) >= B  # maxsteps 3 over 5 steps: a reset inside the launches for every env


# ---- scripted moves.  Padded coordinates; actions 0: +x,
# 1: +y, 2: -x, 3: -y, 4: no-op.  Robots 0..3 start as the 2 x 2 cluster in the
# map's corner; the cell (4, 1) is a wall; x = 0 and y = 0 are the border row
# and column around the map (the only way to leave it).  Robot 3 never moves.
START = [(1, 1), (1, 2), (2, 1), (2, 2)]
SCRIPT = [
    # actions          cells after the step                fails  what the step is for
    ((2, 3, 0, 4), [(1, 1), (1, 2), (3, 1), (2, 2)], 2),  # 0 leaves the map; 1 blocked by a lower robot that stayed
    ((0, 3, 0, 4), [(2, 1), (1, 1), (3, 1), (2, 2)], 1),  # 1 enters the cell 0 vacated in this step; 2 hits the wall
    ((0, 4, 1, 3), [(2, 1), (1, 1), (3, 2), (2, 2)], 2),  # 0 blocked by 2, which has not moved yet; 3 blocked by 0
    ((0, 0, 1, 4), [(3, 1), (2, 1), (3, 3), (2, 2)], 0),  # 1 follows 0 into the vacated cell; nobody fails
    ((3, 3, 3, 3), [(3, 1), (2, 1), (3, 2), (2, 2)], 3),  # 0 and 1 leave the map; 3 blocked by 1
    ((1, 1, 2, 0), [(3, 1), (2, 1), (3, 2), (2, 2)], 4),  # everybody blocked
]


def test_scripted_moves_and_obs(torch_cuda, monkeypatch):
    """Six scripted steps in one fused launch: all three obs layers, the
    reward's bits and done against the oracle at every step, and the scenario
    itself checked on the oracle (cells after every step, failed moves per
    step from the penalties its updateRobotPos returns)."""
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    B, K = 2, len(SCRIPT)
    grid = np.ones((24, 22))
    grid[3, 0] = -1.0  # padded (4, 1)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[grid.copy() for _ in range(B)], auto_reset=True, seed=41)
    assert env.kernel_variant() == "env_kernel<64,2,u32,C2>", env.kernel_variant()
    pos = np.asarray([START] * B, dtype=np.int32)
    env.reset(positions=pos)
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    fails = [[] for _ in range(B)]  # per env: the penalties of the current step
    for b, r in enumerate(refs):
        def counted(x, y, i, _orig=r.updateRobotPos, _log=fails[b]):
            pen = _orig(x, y, i)
            _log.append(pen)
            return pen
        r.updateRobotPos = counted
    acts = np.asarray([[a] * B for a, _, _ in SCRIPT], dtype=np.uint8)  # [K][B][N]
    assert (acts == 4).any() and 255 not in acts
    n0 = env.env_launches()
    obs, rew, done = env.rollout(torch.from_numpy(acts).to(env.device))
    assert env.env_launches() - n0 == 1
    seen = set()
    for k, (_, cells, nfail) in enumerate(SCRIPT):
        for b in range(B):
            del fails[b][:]
            oo, rr, dd = refs[b].step(ref_action(acts[k, b]))
            got_fail = sum(1 for p in fails[b] if p != 0)
            assert got_fail == nfail, (k, b, fails[b])
            assert all(p in (0, -cfg["collision_penalty"]) for p in fails[b])
            assert list(zip(refs[b]._xinds, refs[b]._yinds)) == cells, (k, b)
            assert np.float64(rr).tobytes() == rew[k, b].cpu().numpy().tobytes(), (k, b, rr, float(rew[k, b]))
            assert bool(dd) == bool(done[k, b]) and not dd, (k, b)
            got, oo = obs[k, b].cpu().numpy(), np.asarray(oo)
            assert got.shape == oo.shape and got.shape[1] == 3
            for layer in range(3):
                np.testing.assert_array_equal(got[:, layer], oo[:, layer], err_msg=f"step {k} env {b} layer {layer}")
        seen.add(nfail)
    assert len(seen) >= 3, seen  # at least three different failed-move counts
    # robot 3 never moved: its bit is clear, so no robot layer shows it
    moved = env.get_state(_lib.FIELD_MOVED).cpu().numpy().astype(np.uint64)
    assert all(int(m) == 0b0111 for m in moved), moved
    last = obs[K - 1].cpu().numpy()
    assert last[:, 3, 0, 2, 2].tolist() == [0] * B and last[:, 0, 0, 2, 2].tolist() == [1] * B
    env.check()


def test_the_bench_row(torch_cuda, monkeypatch):
    """128 x 128 maps, B = 3, K = 4: one fused launch against four step calls,
    bitwise, and the final state -- on the row bench.py's default line times."""
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(1611)
    B, K = 3, 4
    envs = pair(cfg, [bern(rs, 128, 128, 0.1) for _ in range(B)], B, auto_reset=True, seed=43)
    assert envs[0].kernel_label() == "64,2,uint32_t,ShapeC2BV", envs[0].kernel_label()
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2>", envs[0].kernel_variant()
    fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 4, sentinel_p=0.0), 1, "diet bench row")


def _child_epw1():
    """MARLCOV_EPW=1: one env per workgroup (every lane of the wave is the
    env's; the obs roles of a one-slot wave)."""
    import torch
    cfg = c2_cfg()
    rs = np.random.RandomState(1612)
    B, K = 3, 6
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=44)
    assert envs[0].kernel_variant() == "env_kernel<64,1,u32,C2>", envs[0].kernel_variant()
    fused_vs_stepped(torch, envs, actions(rs, K, B, 4), 1, "diet epw 1", cfg, oracle=True)
    assert_same_state(envs[0], envs[1], "diet epw 1 end")


def test_one_env_per_workgroup(torch_cuda):
    """MARLCOV_EPW is read once per process: a child process, as
    test_gpu_fused_steps.test_in_a_child_process does."""
    env = dict(os.environ, MARLCOV_EPW="1", MARLCOV_VIS_TABLE="require")
    env.pop("MARLCOV_FUSE_STEPS", None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "epw1 ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    _child_epw1()
    print("epw1 ok")

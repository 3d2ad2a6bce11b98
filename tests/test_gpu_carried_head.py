"""GPU: the env head the fused step loop carries in registers (mc_env_step.h:
HeadK; EnvCfg::CARRY, the one-wave table kernels of the C2 shapes).  In steps
1.. of a fused launch the robots' cells, the env's counters, env_grid, numfree
and the moved mask come from the step before instead of memory, and the action
bytes of step k + 1 are loaded during step k; a slot's words count only after
a step that took the active path without a reset, and one stale slot makes
its whole wave load.  So the cases make slots go stale at different steps
(scripted sentinels, with auto-reset on and off), reset by maxsteps inside
the loop with an idle second slot and at every launch length that moves the
prefetch clamp and the step-0 hand-over, carry for a whole launch over
no-ops, blocked moves and moves off the map, write state between two calls,
and run the bench row and the one-env-per-workgroup rows.

Every case compares, at every step, the reward's bits, done and every obs
layer of the fused rollout with K step calls of a twin env and with the
oracle, and after the call the full device state (ep_pc and ep_len included)
with the twin's, the oracle's state and the oracle's episode records."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_fused_steps import DEFAULT_S, actions, assert_same_state, c2_cfg, launches, pair, set_knobs
from test_gpu_parity import bern
from test_gpu_step_diet import SCRIPT, START

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_ROW = "64,2,uint32_t,ShapeC2V"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def rollout_vs_stepped_vs_oracle(torch, envs, acts, cfg, auto_reset, tag, want_launches=None):
    """envs[0].rollout(acts) against len(acts) envs[1].step calls and against
    oracle envs built from the device state before the call: per step the
    reward's bits, done and every obs layer; after the call the full state and
    the episode records.  Returns the rollout's (obs, reward, done) and the
    state after it."""
    from marlcov import _lib
    fused, stepped = envs
    K, B = acts.shape[:2]
    st = device_state(fused)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    ep_pc = fused.get_state(_lib.FIELD_EP_PC).cpu().numpy().copy()
    ep_len = fused.get_state(_lib.FIELD_EP_LEN).cpu().numpy().copy()
    n0 = fused.env_launches()
    obs_r, rew_r, done_r = fused.rollout(torch.from_numpy(acts).to(fused.device))
    if want_launches is not None:
        assert fused.env_launches() - n0 == want_launches, (tag, fused.env_launches() - n0, want_launches)
    rew_h, done_h, obs_h = rew_r.cpu().numpy(), done_r.cpu().numpy(), obs_r.cpu().numpy()
    for k in range(K):
        o, r, d = stepped.step(torch.from_numpy(acts[k]).to(stepped.device))
        assert torch.equal(o, obs_r[k]), f"{tag}: obs of step {k}"
        assert rew_h[k].tobytes() == r.cpu().numpy().tobytes(), f"{tag}: reward of step {k}"
        assert torch.equal(d, done_r[k]), f"{tag}: done of step {k}"
        pos = None
        for b in range(B):
            oo, rr, dd = refs[b].step(ref_action(acts[k, b]))
            assert np.float64(rr).tobytes() == rew_h[k, b].tobytes(), (tag, k, b, float(rr), float(rew_h[k, b]))
            assert bool(dd) == bool(done_h[k, b]), (tag, k, b)
            if dd:
                ep_pc[b], ep_len[b] = refs[b].percent_covered(), refs[b]._currstep
                if auto_reset:  # the device drew the start cells: the stepped env's, after step k
                    if pos is None:
                        pos = stepped.get_state(_lib.FIELD_POS).cpu().numpy()
                    oo, _ = refs[b].reset(False, None, positions=[tuple(q) for q in pos[b]])
            oo = np.asarray(oo)
            assert obs_h[k, b].shape == oo.shape, (tag, k, b)
            for layer in range(oo.shape[1]):
                np.testing.assert_array_equal(obs_h[k, b][:, layer], oo[:, layer],
                                              err_msg=f"{tag}: step {k} env {b} obs layer {layer}")
    st = assert_same_state(fused, stepped, tag)
    for b in range(B):
        compare_env(st, b, refs[b], f"{tag} end env {b}")
    assert st["ep_pc"].tobytes() == ep_pc.astype(st["ep_pc"].dtype).tobytes(), (tag, st["ep_pc"], ep_pc)
    assert st["ep_len"].tobytes() == ep_len.astype(st["ep_len"].dtype).tobytes(), (tag, st["ep_len"], ep_len)
    for e in envs:
        e.check()
    return obs_r, rew_r, done_r, st


def stale_script(rs, K, B):
    """Case 1's actions: plain moves and a few no-ops, no random sentinel; env 0
    takes a sentinel at step 2 only and env 1 at step 4 only."""
    acts = actions(rs, K, B, 4, sentinel_p=0.0)
    assert 255 not in acts
    acts[2, 0, 0] = 255
    if B > 1:
        acts[4, 1, 0] = 255
    return acts


def stale_case(torch, B, auto_reset, tag):
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(1900 + B)
    K = 8
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=auto_reset, seed=51 + B)
    acts = stale_script(rs, K, B)
    _, _, done, st = rollout_vs_stepped_vs_oracle(torch, envs, acts, cfg, auto_reset, tag, 1)
    done = done.cpu().numpy().astype(bool)  # (checked against the twin and the oracle above)
    sent = acts[:, :, 0] == 255
    assert done[sent].all() and sent.sum() == min(B, 2)
    # the step counter: a reset env counts from its last reset on (a small map
    # can also be covered right after one); without auto-reset every step counts but a sentinel's
    for b in range(B):
        last = np.flatnonzero(done[:, b])
        want = (K - 1 - last[-1] if len(last) else K) if auto_reset else K - int(sent[:, b].sum())
        assert int(st["currstep"][b]) == want, (tag, b, st["currstep"], done[:, b])
    return envs


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("B", [2, 3])
def test_slots_go_stale_at_different_steps(torch_cuda, monkeypatch, B, auto_reset):
    """B = 2 and 3, K = 8 in one launch, sentinels scripted for env 0 at step 2
    and env 1 at step 4: one slot of the first wave takes the reset (auto-reset
    on) or the obs-only path (off) while the other could carry, so the wave
    loads for both in the next step, and carries again after it."""
    assert set_knobs(monkeypatch, "require", None) == DEFAULT_S
    envs = stale_case(torch_cuda, B, auto_reset, f"stale B={B} auto_reset={auto_reset}")
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()


@pytest.mark.parametrize("S", [2, 3, None])
def test_maxsteps_resets_inside_the_loop(torch_cuda, monkeypatch, S):
    """B = 1 (the wave's second slot idle in every step), maxsteps 3, K = 7 in
    launches of 2, 3 and 64 steps: resets in loop steps, in a launch's last
    step (where the prefetch re-reads its own row) and in step 0, whose head
    the loop takes over."""
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=3)
    rs = np.random.RandomState(1911)
    B, K = 1, 7
    envs = pair(cfg, [bern(rs, 24, 22, 0.12)], B, auto_reset=True, seed=57)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    acts = actions(rs, K, B, 4, sentinel_p=0.0)
    assert launches(K, s) == {2: 4, 3: 3, None: 1}[S]
    _, _, done, _ = rollout_vs_stepped_vs_oracle(torch_cuda, envs, acts, cfg, True, f"maxsteps 3 S={S}", launches(K, s))
    assert int(done.sum()) >= 2  # maxsteps 3 over 7 steps: at least two resets inside the launches


def test_long_carry_without_a_reset(torch_cuda, monkeypatch):
    """B = 2, K = 12 in one launch, maxsteps 1000: eleven carried steps in a
    row over the scripted moves of test_gpu_step_diet (no-ops, blocked moves,
    the wall, moves off the map), played twice, the second round from the
    cells the first one ended on."""
    from marlcov import _lib
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    B = 2
    grid = np.ones((24, 22))
    grid[3, 0] = -1.0  # padded (4, 1): the script's wall
    envs = pair(cfg, [grid.copy() for _ in range(B)], B, auto_reset=True, seed=58)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    for e in envs:
        e.reset(positions=np.asarray([START] * B, dtype=np.int32))
    acts = np.asarray([[a] * B for a, _, _ in SCRIPT] * 2, dtype=np.uint8)  # [K][B][N]
    K = len(acts)
    assert K == 12 and (acts == 4).any() and 255 not in acts
    _, _, done, st = rollout_vs_stepped_vs_oracle(torch_cuda, envs, acts, cfg, True, "long carry", 1)
    # the carried counters, as memory holds them after the call (assert_same_state
    # compared them with the stepped env's, compare_env with the oracle's)
    if not done.any():
        assert st["currstep"].tolist() == [K] * B
    assert all(int(m) & 0b0111 == 0b0111 for m in st["moved"]), st["moved"]  # robots 0..2 moved in the first round
    assert (st["free_cnt"] > 0).all() and (st["vis_cnt"] > 0).all()
    fused, stepped = envs
    for f in (_lib.FIELD_MOVED, _lib.FIELD_CURRSTEP, _lib.FIELD_FREE_COUNT, _lib.FIELD_VISITED_COUNT):
        assert fused.get_state(f).cpu().numpy().tobytes() == stepped.get_state(f).cpu().numpy().tobytes(), f


def test_state_written_between_two_calls(torch_cuda, monkeypatch):
    """Three fused steps, then env 0's robots are put on each other's cells by
    set_state (both twins), then three more: the second call's step 0 loads
    what was written, and nothing of the first call's head is left."""
    from marlcov import _lib
    torch = torch_cuda
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(1931)
    B = 2
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=59)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    rollout_vs_stepped_vs_oracle(torch, envs, actions(rs, 3, B, 4, sentinel_p=0.0), cfg, True, "before the write", 1)
    pos = envs[0].get_state(_lib.FIELD_POS).cpu().numpy()
    new = pos.copy()
    new[0] = np.roll(pos[0], 1, axis=0)  # env 0: robot i on robot i - 1's cell
    assert (new[0] != pos[0]).any() and (new[1] == pos[1]).all()
    for e in envs:
        e.set_state(_lib.FIELD_POS, torch.from_numpy(new))
    st = assert_same_state(envs[0], envs[1], "after the write")
    np.testing.assert_array_equal(st["pos"], new)
    rollout_vs_stepped_vs_oracle(torch, envs, actions(rs, 3, B, 4, sentinel_p=0.0), cfg, True, "after the write", 1)


def test_the_bench_row(torch_cuda, monkeypatch):
    """128 x 128 maps, B = 2, K = 6 in one launch: the row bench.py's default
    line times, five carried steps."""
    set_knobs(monkeypatch, "require", None)
    cfg = dict(c2_cfg(), maxsteps=1000)
    rs = np.random.RandomState(1941)
    B, K = 2, 6
    envs = pair(cfg, [bern(rs, 128, 128, 0.1) for _ in range(B)], B, auto_reset=True, seed=60)
    assert envs[0].kernel_label() == "64,2,uint32_t,ShapeC2BV", envs[0].kernel_label()
    rollout_vs_stepped_vs_oracle(torch_cuda, envs, actions(rs, K, B, 4, sentinel_p=0.0), cfg, True, "bench row", 1)


def _child_epw1():
    """MARLCOV_EPW=1: one env per workgroup, the carried head of a one-slot
    wave; case 1's script at B = 2 and B = 3, auto-reset on and off."""
    import torch
    for B in (2, 3):
        for auto_reset in (True, False):
            envs = stale_case(torch, B, auto_reset, f"epw 1 stale B={B} auto_reset={auto_reset}")
            assert envs[0].kernel_label() == "64,1,uint32_t,ShapeC2V", envs[0].kernel_label()


def test_one_env_per_workgroup(torch_cuda):
    """MARLCOV_EPW is read once per process: a child process, as
    test_gpu_step_diet.test_one_env_per_workgroup does."""
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

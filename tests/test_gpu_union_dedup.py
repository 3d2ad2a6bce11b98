"""GPU: the union dedup of the carried C2 table kernels' merge (mc_env_step.h:
under EnvCfg::CARRY it builds only the (item, lower agent) rounds that
ItemGeo leaves, with `b < a` a constant where every lane's agent is above b;
block origins from L.bx / L.by as before) on the authored walks of
tests/union_dedup_cases.py: all four robots in one tile, a pair whose block
origins differ by 1 .. 4 tiles in x, in y and in both (and by 3 and 1), each
of the six pairs as the only overlapping one, two robots that newly see the
same cells in one step, a block origin that shifts in mid-run.
tests/test_union_dedup_cases.py shows from the oracle alone that the `shared`
walks -- every one whose blocks overlap but dxy3 -- have a step whose reward
is wrong without the dedup.

Every case: 3 envs (the second wave's second slot is idle), env b playing the
script from step b on, through mc_step_many with MARLCOV_FUSE_STEPS unset (one
launch: step 0's copy, then the loop copy) and = 1; the row is the table
kernel; reward, done and every obs layer of every step equal the stepped
twin's and the oracle's, and after every step the twin's free / obstacle /
union maps, free_cnt and vis_cnt equal the oracle's; after the call the fused
env's whole state equals the twin's.

Mutants of the code, each built and run against this file and
tests/test_gpu_step_diet2_edges.py (profiles/r21/step_diet2/mutants.txt):
- a dedup round dropped (round (1, 1)): one_tile, pair12 and pair13 fail here,
  with and without fusing; there the 19 x 26, 17 x 17 and 22 x 23 edge maps
  and every pool case;
- `b <= a` for `b < a` in the rounds where it is tested: every case of both
  files fails (a robot dedups against itself);
- the dedup's range test narrowed to `bi < TW - 1`: dx1, dx2, dx3, dx3y1, dxy1,
  dxy2, dy2 and one_tile fail here (dx3 and dx3y1 have their common cells in
  the one tile row two blocks 3 tiles apart share); there three edge maps and
  the pool's resets and auto-reset sentinel (the same narrowing of `bj` was
  not built: dy3 and dx1y3 are its mirror images);
- the clip's row mask applied at TR - 2: none here (these maps are whole
  tiles); there every edge case but 24 x 25 (whose rows are whole tiles) and
  every pool case.
(The issue's fourth mutant, a record base not refreshed after a reset, has no
code to mutate: the carried base was measured and taken out.)"""
import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_carried_head import TABLE_ROW
from test_gpu_fused_steps import assert_same_state, c2_cfg, launches, pair, set_knobs
from union_dedup_cases import SCENARIOS, grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def walk_vs_oracle(torch, envs, acts, cfg, auto_reset, tag, want_launches, regrid=False):
    """envs[0].rollout(acts) against len(acts) envs[1].step calls and oracle
    envs built from the device state before the call: per step reward bits,
    done, every obs layer, and the twin's whole env state against the
    oracle's; after the call the fused env's state against the twin's.
    regrid: a reset draws the env's grid anew (reset_grid_mode "random"), so
    the oracle of an env that reset is rebuilt from the twin's state after the
    step; that step's obs is compared with the twin's only."""
    from marlcov import _lib
    fused, stepped = envs
    K, B = acts.shape[:2]
    st = device_state(fused)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    n0 = fused.env_launches()
    obs_r, rew_r, done_r = fused.rollout(torch.from_numpy(acts).to(fused.device))
    assert fused.env_launches() - n0 == want_launches, (tag, fused.env_launches() - n0, want_launches)
    rew_h, done_h, obs_h = rew_r.cpu().numpy(), done_r.cpu().numpy(), obs_r.cpu().numpy()
    for k in range(K):
        o, r, d = stepped.step(torch.from_numpy(acts[k]).to(stepped.device))
        assert torch.equal(o, obs_r[k]), f"{tag}: obs of step {k}"
        assert rew_h[k].tobytes() == r.cpu().numpy().tobytes(), f"{tag}: reward of step {k}"
        assert torch.equal(d, done_r[k]), f"{tag}: done of step {k}"
        sk = device_state(stepped)
        for b in range(B):
            oo, rr, dd = refs[b].step(ref_action(acts[k, b]))
            assert np.float64(rr).tobytes() == rew_h[k, b].tobytes(), (tag, k, b, float(rr), float(rew_h[k, b]))
            assert bool(dd) == bool(done_h[k, b]), (tag, k, b)
            if dd and auto_reset and regrid:
                refs[b] = oracle_from_device(sk, b, cfg)
                continue
            if dd and auto_reset:  # the device drew the start cells: the twin's, after step k
                oo, _ = refs[b].reset(False, None, positions=[tuple(q) for q in sk["pos"][b]])
            oo = np.asarray(oo)
            for layer in range(oo.shape[1]):
                np.testing.assert_array_equal(obs_h[k, b][:, layer], oo[:, layer],
                                              err_msg=f"{tag}: step {k} env {b} obs layer {layer}")
            compare_env(sk, b, refs[b], f"{tag} step {k} env {b}")
    st = assert_same_state(fused, stepped, tag)
    for e in envs:
        e.check()
    return done_h, st


@pytest.mark.parametrize("S", [None, 1])
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_authored_overlaps(torch_cuda, monkeypatch, name, S):
    s = set_knobs(monkeypatch, "require", S)
    cfg = dict(c2_cfg(), maxsteps=1000)
    start, script, _ = SCENARIOS[name]
    acts0 = np.asarray(script, dtype=np.uint8)
    B, K = 3, len(acts0)
    # env b starts b steps into the script (the cells differ, the moves still succeed or not as the oracle says)
    acts = np.stack([np.roll(acts0, -b, axis=0) for b in range(B)], axis=1)
    envs = pair(cfg, [grid() for _ in range(B)], B, auto_reset=False, seed=91)
    assert envs[0].kernel_label() == TABLE_ROW, envs[0].kernel_label()
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2>", envs[0].kernel_variant()
    for e in envs:
        e.reset(positions=np.asarray([start] * B, dtype=np.int32))
    walk_vs_oracle(torch_cuda, envs, acts, cfg, False, f"{name} S={S}", launches(K, s))

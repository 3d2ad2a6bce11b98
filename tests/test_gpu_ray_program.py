"""GPU: the sparse-beam march from host-built ray programs (csrc/
mc_internal.h build_ray_prog, mc_env_select.h EnvCfg::RAYPROG): the compiled C2
/ C2D instantiations read each ray's cell as the agent's packed cell plus a
precomputed 16-bit offset.  Every case steps against the oracle (oracle/
cpu_ref.py) and compares reward (tolerance 0), done, obs, positions, maps and
counters every step; the kernel instantiation is asserted through
mc_kernel_variant."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_parity import base_cfg, bern, full_obs
from test_gpu_shapes import run_against_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 128), (40, 33)]  # the bench instantiation (baked geometry) / runtime geometry


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def border_grids(rs, W, L, B):
    """Bernoulli grids whose corner cells, their neighbours and the middles
    of the four sides are free."""
    grids = []
    for _ in range(B):
        g = bern(rs, W, L, 0.1)
        for x in (0, 1, W - 2, W - 1):
            for y in (0, 1, L - 2, L - 1):
                g[x, y] = 1.0
        g[0, L // 2] = g[W - 1, L // 2] = g[W // 2, 0] = g[W // 2, L - 1] = 1.0
        grids.append(g)
    return grids


def border_positions(W, L):
    """[3, 4, 2] start cells (padded coordinates) next to every border and
    corner of a W x L grid."""
    return np.array([
        [(1, 1), (1, L), (W, 1), (W, L)],                                # the four corners
        [(1, L // 2 + 1), (W, L // 2 + 1), (W // 2 + 1, 1), (W // 2 + 1, L)],  # the middle of each side
        [(1, 2), (2, 1), (W, L - 1), (W - 1, L)],                        # next to two corners
    ], dtype=np.int32)


def reset_at(torch, env, cfg, pos, thetalist=None):
    """Reset every env at ``pos`` and compare the reset's own sensing with the
    oracle's reset at the same cells."""
    B = env.num_envs
    obs = env.reset(positions=pos)
    obs_h = full_obs(env, obs, cfg)
    st = device_state(env)
    refs = []
    for b in range(B):
        np.testing.assert_array_equal(st["pos"][b], pos[b])
        ref = oracle_from_device(st, b, cfg, thetalist=thetalist)
        o, _ = ref.reset(False, None, positions=[tuple(q) for q in pos[b]])
        np.testing.assert_array_equal(obs_h[b], o, err_msg=f"reset env {b} obs")
        compare_env(st, b, ref, f"reset env {b}")
        refs.append(ref)
    env.check()
    return refs


def steps_vs_oracle(torch, env, cfg, rs, refs, T, label):
    """T steps of random moves against the oracle envs ``refs`` (no done
    expected: the caller's maxsteps exceeds T)."""
    B, N = env.num_envs, env.num_agents
    for t in range(T):
        acts = rs.randint(0, 4, size=(B, N)).astype(np.uint8)
        obs, rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs_h, rew_h, done_h = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
        st = device_state(env)
        for b in range(B):
            o, r, d = refs[b].step(ref_action(acts[b]))
            tag = f"{label} t={t} env {b}"
            assert float(r) == rew_h[b], (tag, float(r), rew_h[b])
            assert bool(d) == bool(done_h[b]) and not d, tag
            np.testing.assert_array_equal(obs_h[b], o, err_msg=tag + " obs")
            compare_env(st, b, refs[b], tag)
    env.check()


@pytest.mark.parametrize("shape", SHAPES)
def test_c2_instantiations_from_border_cells(torch_cuda, shape):
    """Both C2 instantiations, B = 3 (one idle slot), robots injected next to
    every border and corner: the reset's sensing and 12 steps."""
    import marlcov
    torch = torch_cuda
    W, L = shape
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(W + L)
    env = marlcov.BatchCoverageEnv(cfg, 3, grids=border_grids(rs, W, L, 3), auto_reset=True, seed=5)
    assert "<64,2,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch, env, cfg, border_positions(W, L))
    steps_vs_oracle(torch, env, cfg, rs, refs, 12, f"c2 border {shape}")


@pytest.mark.parametrize("shape", SHAPES)
def test_c2_auto_reset_senses_through_the_program(torch_cuda, shape):
    """maxsteps 6 over 20 steps: every env resets inside the step kernel at
    least twice and reset_env's initial sensing runs from the ray program."""
    import marlcov
    torch = torch_cuda
    W, L = shape
    cfg = base_cfg(numrobot=4, maxsteps=6)
    rs = np.random.RandomState(7 * W + L)
    B = 3
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, W, L, 0.1) for _ in range(B)], auto_reset=True, seed=19)
    assert "<64,2,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    env.reset()
    resets = run_against_oracle(torch, env, cfg, rs, 20, list(range(B)), 19, f"c2 auto-reset {shape}")
    assert resets >= 2 * B


def test_beam_table_swaps_rebuild_the_program(torch_cuda):
    """Three beam table swaps on a 40 x 33 env: 21 angles rotated by 3 degrees
    (common patterns, K 8..10: the C2 kernel with another program), 9 beams
    (the generic kernel), the default 21 again."""
    import marlcov
    from marlcov.sensors import beam_angles
    torch = torch_cuda
    W, L = 40, 33
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(73)
    B = 3
    env = marlcov.BatchCoverageEnv(cfg, B, grids=border_grids(rs, W, L, B), auto_reset=True, seed=23)
    assert "<64,2,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    pos = border_positions(W, L)
    swaps = [(beam_angles(21) + np.deg2rad(3.0), "<64,2,u32,C2>"), (beam_angles(9), "<64,2,u32,generic>"),
             (beam_angles(21), "<64,2,u32,C2>")]
    for i, (th, variant) in enumerate(swaps):
        env.sensor.set_thetalist(th)
        assert variant in env.kernel_variant(), (i, env.kernel_variant())
        refs = reset_at(torch, env, cfg, pos, thetalist=th)
        steps_vs_oracle(torch, env, cfg, rs, refs, 6, f"swap {i}")


def test_full_beam_table_runs_the_generic_kernel(torch_cuda, monkeypatch):
    """MARLCOV_BEAM_TABLE=1: no program, so the generic kernel of the same
    geometry marches from the per-start table."""
    import marlcov
    torch = torch_cuda
    monkeypatch.setenv("MARLCOV_BEAM_TABLE", "1")
    W, L = 40, 33
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(41)
    env = marlcov.BatchCoverageEnv(cfg, 3, grids=border_grids(rs, W, L, 3), auto_reset=True, seed=29)
    assert "<64,2,u32,generic>" in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch, env, cfg, border_positions(W, L))
    steps_vs_oracle(torch, env, cfg, rs, refs, 8, "beam table")


def test_dijkstra_input_c2d(torch_cuda):
    """dijkstra_input = 1 on a 40 x 33 grid: the C2D instantiation."""
    import marlcov
    torch = torch_cuda
    W, L = 40, 33
    cfg = base_cfg(numrobot=4, dijkstra_input=1)
    rs = np.random.RandomState(43)
    env = marlcov.BatchCoverageEnv(cfg, 3, grids=border_grids(rs, W, L, 3), auto_reset=True, seed=31)
    assert "<64,2,u32,C2D>" in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch, env, cfg, border_positions(W, L))
    steps_vs_oracle(torch, env, cfg, rs, refs, 8, "c2d")


def _one_env_per_workgroup():
    """(child process, MARLCOV_EPW=1) <64,1,u32,C2>: 64 lanes per env, two
    rays per lane."""
    import marlcov
    import torch
    W, L = 40, 33
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(47)
    env = marlcov.BatchCoverageEnv(cfg, 3, grids=border_grids(rs, W, L, 3), auto_reset=True, seed=37)
    assert "<64,1,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    refs = reset_at(torch, env, cfg, border_positions(W, L))
    steps_vs_oracle(torch, env, cfg, rs, refs, 8, "epw1")
    print("epw1 ok")


def test_one_env_per_workgroup(torch_cuda):
    """MARLCOV_EPW=1 is read once per process, so the case runs in a child
    process of its own."""
    env = dict(os.environ, MARLCOV_EPW="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "epw1 ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    _one_env_per_workgroup()

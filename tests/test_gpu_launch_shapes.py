"""GPU parity of the env kernel's large launch shapes: workgroups of 8 and 16
waves (env_kernel<512 / 1024, 1, u32 / u64, generic>), which only configs with
many robots and a wide window select, and the square sensor beyond the one
shape the other suites run (<64, 2, u32>).

mc_create picks the shape (csrc/mc_env_select.h env_geometry = env_threads,
env_pack and the MARLCOV_NT rule, then select_env_row) from N, the window's
TW = (2 H + 17) // 8 tiles per side (H = max(ceil(range), egoradius)), the
beam count and the sensor; tests/native/env_select_check.cpp checks those
rules on the host for every config of the ORGANIC table below.  Rows are u32
for TW <= 4, else u64.  The LDS slot (csrc/mc_internal.h env_lds_bytes), with
rb = 4 (u32) or 8 and P = 8 TW (N | 1) (u32) or N (8 TW + 1) row-plane words:

    (3 lidar | 6 square) * N * TW^2 * 8  +  pad16(3 P rb)  +  16 * max(beams, 1)
      +  pad16(32 N)  +  64  +  pad16(N)  +  64 rb

e.g. 20 robots at lidar range 27 (TW = 8, 13 beams): 30,720 + 31,200 + 208 +
640 + 64 + 32 + 512 = 63,376 B, the largest accepted slot (21 robots: 66,512 B,
refused; tests/test_host_cpu.py test_create_window_limits).  Every test
asserts the exact kernel_variant() first, so a change of the selection rules
cannot quietly retire a shape from this file.
"""
import zlib

import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from oracle.cpu_ref import DecGridRLRef
import test_gpu_parity as parity
from test_gpu_parity import BATCH_CASES, base_cfg, bern, full_obs, tri
from test_gpu_shapes import run_against_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def lidar(n, beams, rng, **kw):
    return base_cfg(numrobot=n, sensor_config={"num_lasers": beams, "range": rng}, **kw)


def square(n, rng, **kw):
    return base_cfg(numrobot=n, sensor_type="square_sensor", sensor_config={"range": rng}, **kw)


# name: (config, grid maker, B, T, kernel variant)          items  lanes  LDS slot
ORGANIC = {
    # lidar range 27: TW = 8, u64 rows
    "wg512_u64_n12_r27": (lidar(12, 13, 27), lambda rs: bern(rs, 90, 70, 0.1), 3, 8,
                          "env_kernel<512,1,u64,generic>"),            # 768   512   38,336 B
    "wg512_u64_n16_r27_edge": (lidar(16, 13, 27), lambda rs: bern(rs, 90, 70, 0.1), 2, 8,
                               "env_kernel<512,1,u64,generic>"),       # 1,024: the last count at 512 lanes, 50,848 B
    "wg1024_u64_n17_r27": (lidar(17, 13, 27), lambda rs: bern(rs, 90, 70, 0.1), 2, 8,
                           "env_kernel<1024,1,u64,generic>"),          # 1,088: the first count at 1,024 lanes, 54,000 B
    "wg1024_u64_n20_r27_ldsmax": (lidar(20, 13, 27), lambda rs: bern(rs, 90, 70, 0.1), 2, 8,
                                  "env_kernel<1024,1,u64,generic>"),   # 1,280  1,024  63,376 B, the largest slot
    # range 19: TW = 6, a window side that is no power of two
    "wg1024_u64_n30_r19_tw6": (lidar(30, 9, 19), lambda rs: bern(rs, 70, 70, 0.1), 2, 8,
                               "env_kernel<1024,1,u64,generic>"),      # 1,080  1,024  62,912 B
    # TW = 4: u32 rows with the odd row stride N | 1
    "wg512_u32_n64_r10": (lidar(64, 7, 10, collision_penalty=1.5), lambda rs: bern(rs, 60, 60, 0.1), 2, 8,
                          "env_kernel<512,1,u32,generic>"),            # 1,024  512   52,080 B
    "wg256_u32_n32_r8": (lidar(32, 9, 8), lambda rs: bern(rs, 50, 50, 0.1), 3, 10,
                         "env_kernel<256,1,u32,generic>"),             # 512   256   26,480 B
    # the square sensor on 64-bit rows, alone in a workgroup, on many waves
    "square_r12_u64_packed": (square(2, 12), lambda rs: tri(rs, 40, 44), 4, 12,
                              "env_kernel<64,2,u64,generic>"),         # 50    64 (two envs per wave)
    "square_r9_u32_tw4": (square(3, 9), lambda rs: tri(rs, 40, 40), 4, 12,
                          "env_kernel<64,2,u32,generic>"),             # 48    64 (two envs per wave)
    "square_r12_n20_wg256": (square(20, 12), lambda rs: bern(rs, 60, 60, 0.1), 2, 8,
                             "env_kernel<256,1,u64,generic>"),         # 500   256   44,944 B
    "square_r27_n9_wg512": (square(9, 27, egoradius=3), lambda rs: bern(rs, 80, 70, 0.1), 2, 8,
                            "env_kernel<512,1,u64,generic>"),          # 576   512   42,592 B
    "square_r11_n40_wg512_u32": (square(40, 11), lambda rs: bern(rs, 60, 60, 0.1), 2, 8,
                                 "env_kernel<512,1,u32,generic>"),     # 640   512   48,128 B
}


def step_codes(rs, B, N, t):
    """Random moves with no-op codes; sentinel rows at random and, so that every
    case has one however few its envs and steps, in env t % B at t = 2 and 5."""
    acts = rs.randint(0, 4, size=(B, N)).astype(np.uint8)
    acts[rs.rand(B, N) < 0.08] = rs.choice([4, 7, 200])
    acts[rs.rand(B) < 0.05, 0] = 255
    if t in (2, 5):
        acts[t % B, 0] = 255
    return acts


@pytest.mark.parametrize("name", sorted(ORGANIC))
def test_launch_shape_matches_oracle(torch_cuda, name):
    """Each shape from the oracle's own reset, every step: reward (tolerance
    0), done, obs, adjacency, positions, maps, counters."""
    import marlcov
    torch = torch_cuda
    cfg, maker, B, T, variant = ORGANIC[name]
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    grids = [maker(rs) for _ in range(B)]
    N = cfg["numrobot"]
    refs, pos = [], []
    for b in range(B):
        np.random.seed(1000 + b)
        r = DecGridRLRef([grids[b]], cfg)
        refs.append(r)
        pos.append(np.stack([r._xinds, r._yinds], 1))
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=False, want_adjacency=True)
    assert env.kernel_variant() == variant, env.kernel_variant()
    obs, adj = env.reset(positions=np.stack(pos))
    st = device_state(env)
    obs_h = full_obs(env, obs, cfg)
    for b in range(B):
        compare_env(st, b, refs[b], f"{name} reset env {b}")
        np.testing.assert_array_equal(obs_h[b], refs[b].get_egocentric_observations(),
                                      err_msg=f"{name} reset obs {b}")
    sentinels = 0
    for t in range(T):
        acts = step_codes(rs, B, N, t)
        sentinels += int((acts[:, 0] == 255).sum())
        (obs, adj), rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs_h, rew_h, done_h, adj_h = (full_obs(env, obs, cfg), rew.cpu().numpy(),
                                       done.cpu().numpy(), adj.cpu().numpy())
        st = device_state(env)
        for b in range(B):
            o, r, d = refs[b].step(ref_action(acts[b]))
            tag = f"{name} t={t} env {b}"
            assert float(r) == rew_h[b], (tag, float(r), rew_h[b])
            assert bool(d) == bool(done_h[b]), tag
            np.testing.assert_array_equal(obs_h[b], o, err_msg=tag + " obs")
            np.testing.assert_array_equal(adj_h[b], refs[b]._adjacency_matrix, err_msg=tag + " adj")
            compare_env(st, b, refs[b], tag)
    assert sentinels >= 2
    env.check()


# ---------------------------------------------------------------------------
# features that otherwise run on one wave only, on 8 and 16 waves.  MARLCOV_NT
# (read at every mc_create) raises the lane count and leaves one env per
# workgroup; it is also the only way to <1024,1,u32,generic>: u32 rows mean
# TW <= 4, and 64 robots x 16 tiles = 1,024 items stop at 512 lanes.
# ---------------------------------------------------------------------------
MULTI_WAVE_CASES = ["map_sharing_comm", "dijkstra_lidar_n3", "minimap_dist_dijkstra", "lidar_single_tool",
                    "square_r2", "zero_cells", "dist_map_sharing", "crowded_n12"]


@pytest.mark.parametrize("nt", [512, 1024])
@pytest.mark.parametrize("name", MULTI_WAVE_CASES)
def test_features_on_multi_wave_workgroups(torch_cuda, monkeypatch, name, nt):
    """Map sharing and the comm graph, dijkstra_input, minimap layers,
    single_square_tool, the square sensor, zero cells, dist_reward with map
    sharing and the serial move rounds (crowded_n12: most waves hold no
    robot) with the env's work spread over 8 / 16 waves."""
    import marlcov
    monkeypatch.setenv("MARLCOV_NT", str(nt))
    cfg, maker, B, _ = BATCH_CASES[name]
    rs = np.random.RandomState(1)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[maker(rs) for _ in range(B)], auto_reset=False)
    v = env.kernel_variant()
    assert v.startswith(f"env_kernel<{nt},1,") and v.endswith("generic>"), v
    del env
    parity.test_batch_matches_oracle(torch_cuda, name)


# ---------------------------------------------------------------------------
# the non-stepping branch (sentinel rows, envs left out of a partial reset) and
# the reset branch on 8 and 16 waves
# ---------------------------------------------------------------------------
BRANCH_CASES = ["wg512_u32_n64_r10", "wg1024_u64_n20_r27_ldsmax"]


@pytest.mark.parametrize("name", BRANCH_CASES)
def test_wide_workgroup_sentinels_and_partial_resets(torch_cuda, name):
    """test_c4_shape_sentinels_and_partial_resets (tests/test_gpu_shapes.py) at
    8 and 16 waves per env: sentinel rows at 30 % without auto_reset (reward 0,
    done, no state change, obs of the current state), a partial reset with
    injected cells at t = 3 and one with device-drawn cells (checked against
    the host Philox stream) at t = 7, every env against the oracle every step."""
    import marlcov
    from marlcov import streams
    torch = torch_cuda
    cfg, maker, _, _, variant = ORGANIC[name]
    rs = np.random.RandomState(zlib.crc32(name.encode()) + 1)
    B, N, T = 3, cfg["numrobot"], 10
    sent_rows = rs.rand(T, B) < 0.3
    assert sent_rows.sum() >= B * T // 5 and not sent_rows.all(axis=0).any()
    grids = [maker(rs) for _ in range(B)]
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=False, seed=9)
    assert env.kernel_variant() == variant, env.kernel_variant()
    env.reset()
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    for t in range(T):
        if t in (3, 7):
            mask = rs.rand(B) < 0.5
            mask[t % B] = True          # at least one env in ...
            mask[(t + 1) % B] = False   # ... and one out
            inject = t == 3
            pos = None
            if inject:
                pos = st["pos"].copy()
                for b in np.flatnonzero(mask):
                    cells = np.argwhere(refs[b]._grid >= 0)
                    pos[b] = cells[rs.choice(len(cells), N, replace=False)]
            obs = env.reset(env_mask=mask.astype(np.uint8), positions=pos)
            obs_h = full_obs(env, obs, cfg)
            st = device_state(env)
            for b in range(B):
                tag = f"{name} partial reset t={t} env {b}"
                if mask[b]:
                    p = st["pos"][b]
                    if inject:
                        np.testing.assert_array_equal(p, pos[b], err_msg=tag)
                    else:
                        want = streams.start_cells(9, b, int(st["episode"][b]), refs[b]._grid, N)
                        np.testing.assert_array_equal(p, want, err_msg=tag + " start cells vs host Philox")
                    o, _ = refs[b].reset(False, None, positions=[tuple(q) for q in p])
                else:
                    o = refs[b].get_egocentric_observations()
                np.testing.assert_array_equal(obs_h[b], o, err_msg=tag + " obs")
                compare_env(st, b, refs[b], tag)
        acts = rs.randint(0, 4, size=(B, N)).astype(np.uint8)
        acts[rs.rand(B, N) < 0.06] = 9
        acts[sent_rows[t], 0] = 255
        obs, rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs_h, rew_h, done_h = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
        st = device_state(env)
        for b in range(B):
            o, r, d = refs[b].step(ref_action(acts[b]))
            tag = f"{name} sentinel t={t} env {b}"
            assert float(r) == rew_h[b], (tag, float(r), rew_h[b])
            assert bool(d) == bool(done_h[b]), tag
            np.testing.assert_array_equal(obs_h[b], o, err_msg=tag + " obs")
            compare_env(st, b, refs[b], tag)
    env.check()


@pytest.mark.parametrize("name", BRANCH_CASES)
def test_wide_workgroup_auto_reset(torch_cuda, name):
    """maxsteps 7 over 20 steps: every env resets inside the step kernel at
    least twice; each new episode equals the oracle's reset at the device-drawn
    cells, which equal the host Philox draw."""
    import marlcov
    torch = torch_cuda
    cfg, maker, _, _, variant = ORGANIC[name]
    cfg = dict(cfg, maxsteps=7)
    rs = np.random.RandomState(zlib.crc32(name.encode()) + 2)
    B, T = 2, 20
    grids = [maker(rs) for _ in range(B)]
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=True, seed=77, env_offset=1000)
    assert env.kernel_variant() == variant, env.kernel_variant()
    env.reset()
    resets = run_against_oracle(torch, env, cfg, rs, T, list(range(B)), 77, name)
    assert resets >= B

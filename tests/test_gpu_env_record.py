"""GPU: the per-env record (csrc/mc_internal.h EnvRec) behind the step's
scalars -- moved, done_thresh, free / visited counts, currstep, env_grid and
episode live in one 64-byte line per env; mc_get_state / mc_set_state still
speak contiguous [B] buffers.  Every path of the env kernel that reads or
writes the record runs against the oracle (bit-exact, reward tolerance 0) at
the smallest shapes that reach it."""
import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_parity import base_cfg, bern, full_obs
from test_gpu_shapes import run_against_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def test_state_round_trip_of_record_fields(torch_cuda):
    """set_state of one record field with distinct per-env values changes that
    field only: a wrong pitch, width or offset of the strided copies would
    land in a neighbouring field or env."""
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    B = 3
    rs = np.random.RandomState(1)
    env = marlcov.BatchCoverageEnv(base_cfg(numrobot=4), B, grids=[bern(rs, 20, 20, 0.1) for _ in range(B)],
                                   auto_reset=False, seed=2)
    env.reset()
    fields = {
        _lib.FIELD_MOVED: torch.tensor([0x0123456789ABCDE1, 0x7EDCBA9876543212, 0x0F0F0F0FF0F0F0F3], dtype=torch.int64),
        _lib.FIELD_DONE_THRESH: torch.tensor([0.125, 0.75, 1.0625], dtype=torch.float64),
        _lib.FIELD_FREE_COUNT: torch.tensor([101, 102, 103], dtype=torch.int32),
        _lib.FIELD_VISITED_COUNT: torch.tensor([0x01020304, 0x05060708, 0x090A0B0C], dtype=torch.int32),
        _lib.FIELD_CURRSTEP: torch.tensor([7, 8, 9], dtype=torch.int32),
        _lib.FIELD_ENV_GRID: torch.tensor([2, 0, 1], dtype=torch.int32),
        _lib.FIELD_EPISODE: torch.tensor([41, 42, 43], dtype=torch.int32),
    }
    now = {f: env.get_state(f).cpu() for f in fields}
    pos = env.get_state(_lib.FIELD_POS).cpu()
    for f, v in fields.items():
        assert not torch.equal(now[f], v), f  # the write below changes something
        env.set_state(f, v)
        now[f] = v
        for g, want in now.items():
            got = env.get_state(g).cpu()
            assert got.dtype == want.dtype and torch.equal(got, want), (f, g, got, want)
    assert torch.equal(env.get_state(_lib.FIELD_POS).cpu(), pos)
    env.check()


@pytest.mark.parametrize("shape", [(128, 128), (40, 33)])
def test_c2_shapes_odd_batch_auto_reset(torch_cuda, shape):
    """The C2 instantiations (128 x 128: the bench one, baked geometry; 40 x
    33: runtime geometry) with B = 3 -- the last workgroup's second slot is
    idle and clamps to env B - 1 -- and maxsteps 12 over 30 steps: two
    auto-resets per env write currstep, episode, the episode record and moved
    through the record."""
    import marlcov
    torch = torch_cuda
    cfg = base_cfg(numrobot=4, maxsteps=12)
    rs = np.random.RandomState(shape[0])
    B = 3
    grids = [bern(rs, shape[0], shape[1], 0.1) for _ in range(B)]
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=True, seed=31)
    assert "<64,2,u32,C2>" in env.kernel_variant(), env.kernel_variant()
    env.reset()
    resets = run_against_oracle(torch, env, cfg, rs, 30, list(range(B)), 31, f"c2 {shape}")
    assert resets >= 2 * B


def test_generic_kernel_done_incr(torch_cuda):
    """The generic kernel (3 agents, square sensor, 20 x 17 grids): a walled
    6 x 6 room that an episode covers, so done_thresh grows by done_incr at a
    covered episode's end and is written back through the record."""
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    cfg = base_cfg(numrobot=3, maxsteps=15, done_thresh=0.9, done_incr=0.25, sensor_type="square_sensor",
                   sensor_config={"range": 1})
    rs = np.random.RandomState(17)
    B = 5
    grids = []
    for b in range(B):
        g = -np.ones((20, 17))
        g[3 + b:9 + b, 2 + b:8 + b] = 1.0
        grids.append(g)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=True, seed=8)
    assert "generic" in env.kernel_variant(), env.kernel_variant()
    env.reset()
    grown = []

    def on_step(t):
        grown.append(env.get_state(_lib.FIELD_DONE_THRESH).cpu().numpy().copy())

    run_against_oracle(torch, env, cfg, rs, 30, list(range(B)), 8, "generic done_incr", on_step=on_step)
    # (run_against_oracle compared done_thresh with the oracle's every step:
    # where it grew, the oracle's episode covered the room too)
    assert (grown[-1] > 0.9).any(), grown[-1]


@pytest.mark.parametrize("dist", [0, 1])
def test_one_env_per_workgroup_rereads_counters(torch_cuda, dist):
    """16 agents (one env per workgroup): the kernel reads the counters again
    after the moves, from the record."""
    import marlcov
    torch = torch_cuda
    cfg = base_cfg(numrobot=16, dist_reward=dist)
    rs = np.random.RandomState(160 + dist)
    B = 2
    grids = [bern(rs, 64, 64, 0.1) for _ in range(B)]
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=True, seed=6)
    assert ",1," in env.kernel_variant(), env.kernel_variant()
    env.reset()
    run_against_oracle(torch, env, cfg, rs, 20, list(range(B)), 6, f"epw1 dist={dist}", dist_check=bool(dist))


def test_partial_reset_with_mask_and_injected_cells(torch_cuda):
    """mc_reset with env_mask = [1, 0, 1, 0] and injected start cells: the
    masked envs restart there (episode + 1, counters from the first sensing),
    the others keep their record."""
    import marlcov
    torch = torch_cuda
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(5)
    B, N = 4, 4
    grids = [bern(rs, 40, 33, 0.1) for _ in range(B)]
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=False, seed=12)
    env.reset()
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    for t in range(3):
        acts = rs.randint(0, 4, size=(B, N)).astype(np.uint8)
        env.step(torch.from_numpy(acts).to(env.device))
        for b in range(B):
            refs[b].step(ref_action(acts[b]))
    st = device_state(env)
    ep0 = st["episode"].copy()
    mask = np.array([1, 0, 1, 0], dtype=np.uint8)
    pos = st["pos"].copy()
    for b in np.flatnonzero(mask):
        cells = np.argwhere(refs[b]._grid >= 0)
        pos[b] = cells[rs.choice(len(cells), N, replace=False)]
    obs = env.reset(env_mask=mask, positions=pos)
    obs_h = full_obs(env, obs, cfg)
    st = device_state(env)
    for b in range(B):
        if mask[b]:
            np.testing.assert_array_equal(st["pos"][b], pos[b])
            o, _ = refs[b].reset(False, None, positions=[tuple(q) for q in pos[b]])
        else:
            o = refs[b].get_egocentric_observations()
        np.testing.assert_array_equal(obs_h[b], o, err_msg=f"env {b} obs")
        compare_env(st, b, refs[b], f"partial reset env {b}")
        assert int(st["episode"][b]) == int(ep0[b]) + int(mask[b]), b
    env.check()


@pytest.mark.parametrize("auto_reset", [False, True])
def test_sentinel_step(torch_cuda, auto_reset):
    """A sentinel row (agent 0's byte 255): reward 0, done, the episode record
    from the record's counters; without auto_reset no state change, with it
    a reset inside the launch."""
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    cfg = base_cfg(numrobot=4)
    rs = np.random.RandomState(9)
    B, N = 4, 4
    grids = [bern(rs, 40, 33, 0.1) for _ in range(B)]
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=auto_reset, seed=13)
    env.reset()
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    for t in range(4):
        acts = rs.randint(0, 4, size=(B, N)).astype(np.uint8)
        if t == 2:
            acts[[1, 2], 0] = 255
        obs, rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs_h, rew_h, done_h = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
        st = device_state(env)
        ep_pc = env.get_state(_lib.FIELD_EP_PC).cpu().numpy()
        ep_len = env.get_state(_lib.FIELD_EP_LEN).cpu().numpy()
        for b in range(B):
            o, r, d = refs[b].step(ref_action(acts[b]))
            tag = f"t={t} env {b}"
            assert float(r) == rew_h[b] and bool(d) == bool(done_h[b]), tag
            if d:
                assert acts[b, 0] == 255 and rew_h[b] == 0.0, tag
                assert ep_pc[b] == refs[b].percent_covered() and ep_len[b] == refs[b]._currstep, tag
                if auto_reset:
                    o, _ = refs[b].reset(False, None, positions=[tuple(q) for q in st["pos"][b]])
            np.testing.assert_array_equal(obs_h[b], o, err_msg=tag + " obs")
            compare_env(st, b, refs[b], tag)
    env.check()


def test_step_many_with_strides_matches_steps(torch_cuda):
    """mc_step_many, K = 3, non-zero output strides (BatchCoverageEnv.rollout)
    against three mc_step calls on a twin env: outputs and end state."""
    import marlcov
    torch = torch_cuda
    cfg = base_cfg(numrobot=4, maxsteps=2)
    rs = np.random.RandomState(3)
    B, N, K = 4, 4, 3
    grids = [bern(rs, 40, 33, 0.1) for _ in range(B)]
    envs = [marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=True, seed=14) for _ in range(2)]
    for e in envs:
        e.reset()
    acts = torch.from_numpy(rs.randint(0, 4, size=(K, B, N)).astype(np.uint8)).to(envs[0].device)
    obs_r, rew_r, done_r = envs[0].rollout(acts)
    for k in range(K):
        o, r, d = envs[1].step(acts[k])
        assert torch.equal(o, obs_r[k]) and torch.equal(r, rew_r[k]) and torch.equal(d, done_r[k]), k
    assert int(done_r[1].sum()) == B  # maxsteps 2: every env reset inside the rollout
    st0, st1 = device_state(envs[0]), device_state(envs[1])
    for k in st0:
        np.testing.assert_array_equal(st0[k], st1[k], err_msg=k)
    for e in envs:
        e.check()

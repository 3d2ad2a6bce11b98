"""GPU: ``BatchSuperGridEnv.rollout`` / ``mc_sg_step_many`` -- K SuperGridRL
steps in one call.  Without ``dist_reward`` the steps run up to
MARLCOV_FUSE_STEPS per step-kernel launch (sg_step_loop) and the distance
layer is computed once, after the last step; with it every step is launched as
``mc_sg_step`` launches it.  Either way the call must leave exactly what K
``step`` calls leave.

1. every kernel family against the oracle (oracle/super_ref.py): each step's
   reward and done, the full state after the last step, and the launch counts;
2. the distance layer after a fused chunk (the erosion kernel's region write
   is exact for one step only: the layer must be rewritten whole);
3. auto-reset inside a chunk, bit-equal to a stepped twin;
4. ``dist_reward = 1`` is stepped, not fused;
5. strides of 0 and a null quotient pointer; 6. K = 0 and K = 1;
7. refused calls enqueue nothing; 8. fork right after a fused rollout.
Everything is compared exactly (tolerance 0), as tests/test_gpu_super.py does.
The oracle run of a case is computed once and shared by its S variants."""
import ctypes
import functools
import zlib

import numpy as np
import pytest

from oracle.super_ref import SuperGridRLRef
from test_gpu_super import AUTO_RESET_CASES, bernoulli, compare, device_state, draw_positions, sg_cfg

pytestmark = pytest.mark.gpu

KNOBS = ("MARLCOV_SG_ROWS", "MARLCOV_SG_GPW", "MARLCOV_SG_GENERIC", "MARLCOV_SG_SWEEP", "MARLCOV_SG_FULL_DIST",
         "MARLCOV_FUSE_STEPS")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def set_knobs(monkeypatch, knobs, fuse=None):
    """The handle reads its knobs at create: clear them all, then set the case's."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    if fuse is not None:
        monkeypatch.setenv("MARLCOV_FUSE_STEPS", str(fuse))


def make_env(cfg, B, shape, p, grid_seed, **kw):
    """B envs on their own Bernoulli grids, reset at drawn start cells."""
    import marlcov
    rs = np.random.RandomState(grid_seed)
    grids = [bernoulli(rs, shape[0], shape[1], p) for _ in range(B)]
    pos = np.stack([draw_positions(rs, g, cfg["numrobot"]) for g in grids])
    kw.setdefault("auto_reset", False)
    env = marlcov.BatchSuperGridEnv(cfg, B, grids=grids, device="cuda", **kw)
    env.reset(positions=pos)
    return env, grids, pos


def random_actions(rs, K, B, N, p_sentinel):
    digits = rs.randint(0, 4, size=(K, B, N)).astype(np.uint8)
    quot = rs.choice([0, 0, 0, 1, 2, 3], size=(K, B)).astype(np.int32)
    sentinel = rs.rand(K, B) < p_sentinel
    codes = digits.copy()
    codes[sentinel, 0] = 255
    return digits, quot, sentinel, codes


def assert_same_state(a, b, tag):
    sa, sb = device_state(a), device_state(b)
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{tag}: {k}")


def episode_fields(env):
    from marlcov import _lib
    return {f: env.get_state(f).cpu().numpy() for f in (_lib.SG_FIELD_EPISODE, _lib.SG_FIELD_EP_PC, _lib.SG_FIELD_EP_LEN)}


# ---------------------------------------------------------------------------
# 1. against the oracle, every kernel family, no auto-reset
# name: (config, grid shape, p(obstacle), B, K, knobs, kernels)
# ---------------------------------------------------------------------------
_LANES = {"MARLCOV_SG_ROWS": "0"}
ORACLE_CASES = {
    "rows_n4_r2": (sg_cfg(numrobot=4, senseradius=2), (40, 52), 0.15, 19, 40, {},
                   "sg_step_rows<2,4> rl=4 dpp | sg_erode"),
    "lanes_n4_r2": (sg_cfg(numrobot=4, senseradius=2), (40, 52), 0.15, 19, 40, _LANES,
                    "sg_step_kernel<2,4> | sg_erode"),
    "generic_n1_r0": (sg_cfg(numrobot=1, senseradius=0), (20, 20), 0.2, 7, 40, {},
                      "sg_step_kernel<-1,4> | sg_erode"),
    "scan_n6_r1": (sg_cfg(numrobot=6, senseradius=1, use_scanning=1), (33, 33), 0.2, 11, 40, {},
                   "sg_step_rows<1,2> rl=4 | sg_erode"),
    "global_150x300": (sg_cfg(numrobot=4, senseradius=2), (150, 300), 0.1, 3, 12, {},
                       "sg_step_rows<2,4> rl=4 dpp | sg_dist<global> nt=256"),
}
# (case, MARLCOV_FUSE_STEPS or None = unset: the default, 64)
ORACLE_RUNS = [(n, s) for n in sorted(ORACLE_CASES) if n != "global_150x300" for s in (16, None, 1)] + \
    [("global_150x300", None)]


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The case's inputs and what the oracle makes of them: per-step reward and
    done, and the oracle envs after the last step.  Read-only for its users.
    lanes_n4_r2 is rows_n4_r2 on another kernel: one oracle run serves both."""
    cfg, shape, p, B, K, _, _ = ORACLE_CASES[name]
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    N = cfg["numrobot"]
    grids = [bernoulli(rs, shape[0], shape[1], p) for _ in range(B)]
    pos = np.stack([draw_positions(rs, g, N) for g in grids])
    digits, quot, sentinel, codes = random_actions(rs, K, B, N, 0.05)
    refs, rew, done = [], np.zeros((K, B)), np.zeros((K, B), dtype=bool)
    for b in range(B):
        np.random.seed(b)
        r = SuperGridRLRef([grids[b]], cfg)
        r.reset(False, None, positions=pos[b])
        for k in range(K):
            if sentinel[k, b]:
                _, rr, rd = r.step(None)
            else:
                a = int(sum(int(d) * 4 ** i for i, d in enumerate(digits[k, b]))) + int(quot[k, b]) * 4 ** N
                _, rr, rd = r.step(a)
            rew[k, b], done[k, b] = float(rr), bool(rd)
        refs.append(r)
    return dict(grids=grids, pos=pos, codes=codes, quot=quot, rew=rew, done=done, refs=refs)


def oracle_key(name):
    return "rows_n4_r2" if name == "lanes_n4_r2" else name


@pytest.mark.parametrize("name,fuse", ORACLE_RUNS, ids=[f"{n}-S{s}" for n, s in ORACLE_RUNS])
def test_rollout_matches_oracle(torch_cuda, monkeypatch, name, fuse):
    import marlcov
    torch = torch_cuda
    cfg, shape, p, B, K, knobs, variant = ORACLE_CASES[name]
    set_knobs(monkeypatch, knobs, fuse)
    o = oracle_run(oracle_key(name))
    env = marlcov.BatchSuperGridEnv(cfg, B, grids=o["grids"], device="cuda", auto_reset=False)
    assert env.kernel_variant() == variant, (name, env.kernel_variant())
    env.reset(positions=o["pos"])
    s0, d0 = env.launches()
    (planes, dist), rew, dn = env.rollout(torch.from_numpy(o["codes"]).cuda(), quot=torch.from_numpy(o["quot"]))
    env.check()
    s1, d1 = env.launches()
    S = 64 if fuse is None else fuse
    assert (s1 - s0, d1 - d0) == (-(-K // S), 1), (name, fuse, s1 - s0, d1 - d0)
    assert planes is env.planes and dist is env.dist
    assert tuple(rew.shape) == (K, B) and rew.dtype == torch.float64
    assert tuple(dn.shape) == (K, B) and dn.dtype == torch.uint8
    np.testing.assert_array_equal(rew.cpu().numpy(), o["rew"], err_msg=f"{name} reward")
    np.testing.assert_array_equal(dn.cpu().numpy().astype(bool), o["done"], err_msg=f"{name} done")
    np.testing.assert_array_equal(env.reward.cpu().numpy(), o["rew"][-1])
    np.testing.assert_array_equal(env.done.cpu().numpy().astype(bool), o["done"][-1])
    st = device_state(env)
    for b in range(B):
        compare(st, b, o["refs"][b], f"{name} S={fuse} after {K} steps env {b}")


# ---------------------------------------------------------------------------
# 2. the distance layer after a chunk.  On the oracle (checked on the CPU in
# tests/test_super_rollout_host_cpu.py): max(d) is 2 before and after the 20
# steps, 61 cells of the layer change, and 43 of them lie outside the 9 x 9
# region (side 2 (r + M_old + 1) + 1) around the final cell (6, 25) -- the only
# cells a transform that keeps its one-step region write would store.
# ---------------------------------------------------------------------------
def test_rollout_rewrites_whole_distance_layer(torch_cuda, monkeypatch):
    import marlcov
    torch = torch_cuda
    set_knobs(monkeypatch, {})
    cfg = sg_cfg(numrobot=1, senseradius=1)
    B = 5
    grid = np.ones((12, 48))
    pos = np.tile(np.array([[[6, 2]]], dtype=np.int32), (B, 1, 1))
    env = marlcov.BatchSuperGridEnv(cfg, B, grids=[grid] * B, device="cuda", auto_reset=False)
    assert env.kernel_variant() == "sg_step_rows<1,4> rl=16 | sg_erode", env.kernel_variant()
    env.reset(positions=pos)
    np.random.seed(0)
    ref = SuperGridRLRef([grid], cfg)
    ref.reset(False, None, positions=pos[0])
    east = torch.full((B, 1), 2, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        env.step(east)
        ref.step(2)
    rr = np.zeros(20)
    for k in range(20):
        _, r, _ = ref.step(2)
        rr[k] = float(r)
    _, rew, _ = env.rollout(east.expand(20, B, 1).contiguous())
    env.check()
    assert (ref._xinds[0], ref._yinds[0]) == (6, 25)
    np.testing.assert_array_equal(rew.cpu().numpy(), np.tile(rr[:, None], (1, B)))
    st = device_state(env)
    for b in range(B):
        compare(st, b, ref, f"dist layer after a chunk env {b}")


# ---------------------------------------------------------------------------
# 3. auto-reset inside a chunk, against a stepped twin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AUTO_RESET_CASES))
def test_rollout_auto_reset_equals_stepped_twin(torch_cuda, monkeypatch, name):
    torch = torch_cuda
    knobs, variant = AUTO_RESET_CASES[name]
    set_knobs(monkeypatch, knobs, 16)
    rows = name == "rows_2_per_wave"
    cfg = sg_cfg(numrobot=6, senseradius=2, free_penalty=0.15) if rows else \
        sg_cfg(numrobot=4, senseradius=1, free_penalty=0.15)
    B, K, cut, N = (10 if rows else 73), 40, 9, cfg["numrobot"]
    seed = zlib.crc32(name.encode())
    fused, _, _ = make_env(cfg, B, (17, 15), 0.12, seed, auto_reset=True, maxsteps=cut, seed=11)
    twin, _, _ = make_env(cfg, B, (17, 15), 0.12, seed, auto_reset=True, maxsteps=cut, seed=11)
    assert fused.kernel_variant() == variant == twin.kernel_variant(), fused.kernel_variant()
    _, quot, _, codes = random_actions(np.random.RandomState(seed + 1), K, B, N, 0.03)
    acts, q = torch.from_numpy(codes).cuda(), torch.from_numpy(quot).cuda()
    s0, d0 = fused.launches()
    _, rew, dn = fused.rollout(acts, quot=q)
    fused.check()
    s1, d1 = fused.launches()
    assert (s1 - s0, d1 - d0) == (3, 1)
    rew_t, dn_t = np.zeros((K, B)), np.zeros((K, B), dtype=np.uint8)
    for k in range(K):
        _, r, d = twin.step(acts[k], quot=q[k])
        rew_t[k], dn_t[k] = r.cpu().numpy(), d.cpu().numpy()
    twin.check()
    np.testing.assert_array_equal(rew.cpu().numpy(), rew_t)
    np.testing.assert_array_equal(dn.cpu().numpy(), dn_t)
    assert int(dn_t.sum()) >= B  # every env passed the cut inside a chunk
    assert_same_state(fused, twin, name)
    ef, et = episode_fields(fused), episode_fields(twin)
    for f in ef:
        np.testing.assert_array_equal(ef[f], et[f], err_msg=f"{name}: field {f}")


# ---------------------------------------------------------------------------
# 4. dist_reward = 1 is stepped, not fused
# ---------------------------------------------------------------------------
def test_rollout_dist_reward_is_stepped(torch_cuda, monkeypatch):
    import marlcov
    torch = torch_cuda
    set_knobs(monkeypatch, {})
    cfg = sg_cfg(numrobot=4, senseradius=2, dist_reward=1)
    B, K, N = 6, 12, 4
    rs = np.random.RandomState(404)
    grids = [bernoulli(rs, 40, 52, 0.15) for _ in range(B)]
    pos = np.stack([draw_positions(rs, g, N) for g in grids])
    digits, quot, sentinel, codes = random_actions(rs, K, B, N, 0.05)
    env = marlcov.BatchSuperGridEnv(cfg, B, grids=grids, device="cuda", auto_reset=False)
    assert env.kernel_variant() == "sg_step_rows<2,4> rl=4 dpp | sg_erode", env.kernel_variant()
    env.reset(positions=pos)
    s0, d0 = env.launches()
    _, rew, dn = env.rollout(torch.from_numpy(codes).cuda(), quot=torch.from_numpy(quot))
    env.check()
    s1, d1 = env.launches()
    assert (s1 - s0, d1 - d0) == (K, K)
    rew, dn = rew.cpu().numpy(), dn.cpu().numpy()
    st = device_state(env)
    for b in range(B):
        np.random.seed(b)
        r = SuperGridRLRef([grids[b]], cfg)
        r.reset(False, None, positions=pos[b])
        for k in range(K):
            if sentinel[k, b]:
                _, rr, rd = r.step(None)
            else:
                _, rr, rd = r.step(int(sum(int(d) * 4 ** i for i, d in enumerate(digits[k, b]))) + int(quot[k, b]) * 4 ** N)
            assert float(rr) == rew[k, b] and bool(rd) == bool(dn[k, b]), (k, b, float(rr), rew[k, b])
        compare(st, b, r, f"dist_reward rollout env {b}")


# ---------------------------------------------------------------------------
# 5.-8. the call's contract, on one small shape: twins with the same seed
# ---------------------------------------------------------------------------
SMALL = (sg_cfg(numrobot=4, senseradius=2, free_penalty=0.15), 10, (17, 15), 0.12)


def small_twins(monkeypatch, fuse=16, **kw):
    set_knobs(monkeypatch, {}, fuse)
    cfg, B, shape, p = SMALL
    a, _, _ = make_env(cfg, B, shape, p, 808, **kw)
    b, _, _ = make_env(cfg, B, shape, p, 808, **kw)
    assert a.kernel_variant() == "sg_step_rows<2,4> rl=4 dpp | sg_erode", a.kernel_variant()
    return a, b, B, cfg["numrobot"]


def stream_of(env):
    return ctypes.c_void_p(env._torch.cuda.current_stream(env.device).cuda_stream)


def test_step_many_zero_strides_and_null_quot(torch_cuda, monkeypatch):
    torch = torch_cuda
    env, twin, B, N = small_twins(monkeypatch)
    K = 20
    _, quot, _, codes = random_actions(np.random.RandomState(5), K, B, N, 0.05)
    acts, q = torch.from_numpy(codes).cuda(), torch.from_numpy(quot).cuda()
    # every output stride 0: the buffers hold the last step's values
    rew = torch.zeros(B, dtype=torch.float64, device="cuda")
    dn = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rc = env.lib.mc_sg_step_many(env._h, acts.data_ptr(), B * N, q.data_ptr(), B * 4, K, rew.data_ptr(), 0,
                                 dn.data_ptr(), 0, stream_of(env))
    assert rc == 0, env.lib.mc_last_error()
    _, rew_t, dn_t = twin.rollout(acts, quot=q)
    np.testing.assert_array_equal(rew.cpu().numpy(), rew_t[-1].cpu().numpy())
    np.testing.assert_array_equal(dn.cpu().numpy(), dn_t[-1].cpu().numpy())
    assert_same_state(env, twin, "output strides 0")
    # actions_stride 0 and no quotients: one action row K times == K steps with it
    row = torch.from_numpy(codes[0]).cuda()
    row[:, 0] = row[:, 0] % 4  # no sentinel row: every step moves
    rew_k = torch.zeros((K, B), dtype=torch.float64, device="cuda")
    dn_k = torch.zeros((K, B), dtype=torch.uint8, device="cuda")
    rc = env.lib.mc_sg_step_many(env._h, row.data_ptr(), 0, None, 0, K, rew_k.data_ptr(), B * 8, dn_k.data_ptr(), B,
                                 stream_of(env))
    assert rc == 0, env.lib.mc_last_error()
    for k in range(K):
        _, r, d = twin.step(row)
        np.testing.assert_array_equal(rew_k[k].cpu().numpy(), r.cpu().numpy(), err_msg=f"step {k}")
        np.testing.assert_array_equal(dn_k[k].cpu().numpy(), d.cpu().numpy(), err_msg=f"step {k}")
    assert_same_state(env, twin, "actions_stride 0")
    # step_many_raw is that call with every output stride 0
    assert env.step_many_raw(row.data_ptr(), 0, 3, rew.data_ptr(), dn.data_ptr(), stream_of(env)) == 0
    for _ in range(3):
        _, r, d = twin.step(row)
    np.testing.assert_array_equal(rew.cpu().numpy(), r.cpu().numpy())
    assert_same_state(env, twin, "step_many_raw")
    env.check()


def test_step_many_zero_and_one_step(torch_cuda, monkeypatch):
    torch = torch_cuda
    env, twin, B, N = small_twins(monkeypatch)
    _, quot, _, codes = random_actions(np.random.RandomState(6), 1, B, N, 0.0)
    acts, q = torch.from_numpy(codes).cuda(), torch.from_numpy(quot).cuda()
    rew = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    dn = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    before = env.launches()
    rc = env.lib.mc_sg_step_many(env._h, acts.data_ptr(), B * N, q.data_ptr(), B * 4, 0, rew.data_ptr(), B * 8,
                                 dn.data_ptr(), B, stream_of(env))
    assert rc == 0 and env.launches() == before
    _, r0, d0 = env.rollout(acts[:0])
    assert tuple(r0.shape) == (0, B) and tuple(d0.shape) == (0, B) and env.launches() == before
    assert (rew == 7.0).all() and (dn == 9).all()
    assert_same_state(env, twin, "K = 0")
    _, r1, d1 = env.rollout(acts, quot=q)
    assert env.launches() == (before[0] + 1, before[1] + 1)
    _, r, d = twin.step(acts[0], quot=q[0])
    np.testing.assert_array_equal(r1[0].cpu().numpy(), r.cpu().numpy())
    np.testing.assert_array_equal(d1[0].cpu().numpy(), d.cpu().numpy())
    assert_same_state(env, twin, "K = 1")
    env.check()


def test_step_many_refused_calls_enqueue_nothing(torch_cuda, monkeypatch):
    torch = torch_cuda
    env, twin, B, N = small_twins(monkeypatch)
    K = 4
    _, quot, _, codes = random_actions(np.random.RandomState(7), K, B, N, 0.0)
    acts, q = torch.from_numpy(codes).cuda(), torch.from_numpy(quot).cuda()
    rew = torch.zeros((K, B), dtype=torch.float64, device="cuda")
    dn = torch.zeros((K, B), dtype=torch.uint8, device="cuda")
    good = dict(a=acts.data_ptr(), a_s=B * N, q=q.data_ptr(), q_s=B * 4, k=K, r=rew.data_ptr(), r_s=B * 8,
                d=dn.data_ptr(), d_s=B)
    bad = {"reward_stride 12": dict(r_s=12), "quot_stride 6": dict(q_s=6), "num_steps -1": dict(k=-1),
           "null reward": dict(r=None), "stride overflow": dict(a_s=2 ** 62)}
    before = env.launches()
    for what, change in bad.items():
        c = dict(good, **change)
        rc = env.lib.mc_sg_step_many(env._h, c["a"], c["a_s"], c["q"], c["q_s"], c["k"], c["r"], c["r_s"], c["d"],
                                     c["d_s"], stream_of(env))
        assert rc == -1, (what, rc)  # MC_EINVAL
        assert "mc_sg_step_many" in env.lib.mc_last_error().decode(), what
        assert env.launches() == before, what
    assert env.lib.mc_sg_launches(env._h, 2) == -1
    assert_same_state(env, twin, "refused calls")
    env.check()


def test_fork_after_fused_rollout(torch_cuda, monkeypatch):
    torch = torch_cuda
    env, _, B, N = small_twins(monkeypatch)
    K = 20
    _, quot, _, codes = random_actions(np.random.RandomState(8), K + 1, B, N, 0.0)
    acts, q = torch.from_numpy(codes).cuda(), torch.from_numpy(quot).cuda()
    env.rollout(acts[:K], quot=q[:K])
    sib = env.sibling(B)
    sib.fork(torch.arange(B, dtype=torch.int32, device="cuda"), source=env)
    assert_same_state(env, sib, "forked")
    _, r_e, d_e = env.step(acts[K], quot=q[K])
    _, r_s, d_s = sib.step(acts[K], quot=q[K])
    np.testing.assert_array_equal(r_e.cpu().numpy(), r_s.cpu().numpy())
    np.testing.assert_array_equal(d_e.cpu().numpy(), d_s.cpu().numpy())
    assert_same_state(env, sib, "one step after the fork")
    env.check()
    sib.check()

"""GPU: mc_step_many's fused launches (mc_env_step.h: io.num_steps steps
inside one env-kernel launch; mc_capi.hip / mc_fuse.h: ceil(K / S) launches,
S = MARLCOV_FUSE_STEPS read at mc_create).  Every case builds two identical
envs, drives one by ``rollout`` (fused) and the other by K ``step`` calls, and
asks for bitwise equal obs, reward, done and adjacency at every step and a
bitwise equal device state at the end; it asserts kernel_variant() and the
mc_env_launches delta, so the fused path cannot be retired quietly.  Maps are
small on purpose (20-26 cells a side): every line a step re-reads stays
cache-resident, which is where a stale read would show.  About 8 % of the
action rows are sentinels and maxsteps is 7-9, so resets fall inside launches
and on chunk boundaries."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_launch_shapes import lidar, square
from test_gpu_parity import base_cfg, bern, tri

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_S = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def launches(K, S):
    return -(-K // S)


def actions(rs, K, B, N, sentinel_p=0.08):
    acts = rs.randint(0, 4, size=(K, B, N)).astype(np.uint8)
    acts[rs.rand(K, B, N) < 0.05] = 4  # a no-op code
    acts[rs.rand(K, B) < sentinel_p, 0] = 255
    return acts


def full_state(env):
    from marlcov import _lib
    st = device_state(env)
    st["ep_pc"] = env.get_state(_lib.FIELD_EP_PC).cpu().numpy()
    st["ep_len"] = env.get_state(_lib.FIELD_EP_LEN).cpu().numpy()
    return st


def assert_same_state(e0, e1, tag):
    s0, s1 = full_state(e0), full_state(e1)
    assert sorted(s0) == sorted(s1)
    for k in s0:
        assert s0[k].tobytes() == s1[k].tobytes(), f"{tag}: state field {k} differs"
    return s0


def pair(cfg, grids, B, **kw):
    import marlcov
    envs = [marlcov.BatchCoverageEnv(cfg, B, grids=grids, **kw) for _ in range(2)]
    for e in envs:
        e.reset()
    return envs


def fused_vs_stepped(torch, envs, acts, want_launches, tag, cfg=None, oracle=False):
    """envs[0].rollout(acts) against len(acts) envs[1].step calls; with
    ``oracle`` every step also against oracle envs (auto-reset configs)."""
    from marlcov import _lib
    fused, stepped = envs
    K, B = acts.shape[:2]
    refs = None
    if oracle:
        st = device_state(fused)
        refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    n0, n1 = fused.env_launches(), stepped.env_launches()
    out = fused.rollout(torch.from_numpy(acts).to(fused.device))
    assert fused.env_launches() - n0 == want_launches, (tag, fused.env_launches() - n0, want_launches)
    adj_r = None
    if fused.adj is not None:
        (obs_r, adj_r), rew_r, done_r = out
    else:
        obs_r, rew_r, done_r = out
    for k in range(K):
        res = stepped.step(torch.from_numpy(acts[k]).to(stepped.device))
        if adj_r is not None:
            (o, a), r, d = res
            assert torch.equal(a, adj_r[k]), f"{tag}: adjacency of step {k}"
        else:
            o, r, d = res
        assert torch.equal(o, obs_r[k]), f"{tag}: obs of step {k}"
        assert rew_r[k].cpu().numpy().tobytes() == r.cpu().numpy().tobytes(), f"{tag}: reward of step {k}"
        assert torch.equal(d, done_r[k]), f"{tag}: done of step {k}"
        if refs is not None:
            for b in range(B):
                oo, rr, dd = refs[b].step(ref_action(acts[k, b]))
                assert float(rr) == float(rew_r[k, b]) and bool(dd) == bool(done_r[k, b]), (tag, k, b)
                if dd:
                    p = stepped.get_state(_lib.FIELD_POS).cpu().numpy()[b]  # the stepped env, after step k
                    oo, _ = refs[b].reset(False, None, positions=[tuple(q) for q in p])
                np.testing.assert_array_equal(obs_r[k, b].cpu().numpy(), oo, err_msg=f"{tag} k={k} b={b}")
    assert stepped.env_launches() - n1 == K, tag
    st = assert_same_state(fused, stepped, tag)
    if refs is not None:
        for b in range(B):
            compare_env(st, b, refs[b], f"{tag} end env {b}")
    for e in envs:
        e.check()
    return done_r


def c2_cfg(**kw):
    return base_cfg(numrobot=4, maxsteps=8, **kw)  # 21 beams, R = 10, egoradius 2: the C2 shape


def set_knobs(monkeypatch, vis=None, S=None):
    if vis is not None:
        monkeypatch.setenv("MARLCOV_VIS_TABLE", vis)
    if S is None:
        monkeypatch.delenv("MARLCOV_FUSE_STEPS", raising=False)
    else:
        monkeypatch.setenv("MARLCOV_FUSE_STEPS", str(S))
    return DEFAULT_S if S is None else max(1, S)


@pytest.mark.parametrize("S", [16, None, 1])
@pytest.mark.parametrize("vis", ["require", "0"])
def test_c2_auto_reset_odd_batch(torch_cuda, monkeypatch, vis, S):
    """The C2 shape, B = 5 (the last wave has an idle slot), K = 40, auto-reset,
    with S = 16 (3 launches), the default S (1) and S = 1 (40); every step also
    against the oracle."""
    s = set_knobs(monkeypatch, vis, S)
    cfg = c2_cfg()
    rs = np.random.RandomState(1201)
    B, K = 5, 40
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=11)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2>", envs[0].kernel_variant()
    done = fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 4), launches(K, s), f"c2 {vis} S={S}", cfg, oracle=True)
    assert int(done.sum()) >= 3 * B  # maxsteps 8 over 40 steps: resets inside launches


@pytest.mark.parametrize("vis", ["require", "0"])
def test_c2_without_auto_reset(torch_cuda, monkeypatch, vis):
    """auto_reset off: the sentinel and obs-only path in steps k > 0 of a
    launch, and an env that reported done keeps stepping as the stepped env does."""
    set_knobs(monkeypatch, vis, 16)
    cfg = c2_cfg()
    rs = np.random.RandomState(1202)
    B, K = 5, 40
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=False, seed=12)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2>", envs[0].kernel_variant()
    acts = actions(rs, K, B, 4)
    assert (acts[1:, :, 0] == 255).sum() >= 5
    done = fused_vs_stepped(torch_cuda, envs, acts, 3, f"c2 no auto-reset {vis}")
    assert int(done.sum()) > int((acts[:, :, 0] == 255).sum())  # maxsteps dones besides the sentinels'


def test_generic_three_robots_u32(torch_cuda, monkeypatch):
    """3 robots, 9 beams: the generic two-envs-per-wave kernel on 32-bit rows."""
    set_knobs(monkeypatch, None, 16)
    cfg = lidar(3, 9, 4, maxsteps=9)
    rs = np.random.RandomState(1203)
    B, K = 5, 40
    envs = pair(cfg, [bern(rs, 20, 20, 0.15) for _ in range(B)], B, auto_reset=True, seed=13)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,generic>", envs[0].kernel_variant()
    fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 3), 3, "generic n3", cfg, oracle=True)


def test_square_sensor_u64(torch_cuda, monkeypatch):
    """The square sensor on 64-bit rows, two envs per wave."""
    set_knobs(monkeypatch, None, 16)
    cfg = square(2, 12, maxsteps=7)
    rs = np.random.RandomState(1204)
    B, K = 5, 40
    envs = pair(cfg, [tri(rs, 24, 26) for _ in range(B)], B, auto_reset=True, seed=14)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u64,generic>", envs[0].kernel_variant()
    fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 2), 3, "square u64")


def test_multi_wave_generic(torch_cuda, monkeypatch):
    """Four waves per env: the barrier and the fences between a launch's steps."""
    set_knobs(monkeypatch, None, 4)
    cfg = lidar(32, 9, 8, maxsteps=7)
    rs = np.random.RandomState(1205)
    B, K = 3, 10
    envs = pair(cfg, [bern(rs, 50, 50, 0.1) for _ in range(B)], B, auto_reset=True, seed=15)
    assert envs[0].kernel_variant() == "env_kernel<256,1,u32,generic>", envs[0].kernel_variant()
    fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 32), 3, "wg256 generic")


def test_multi_wave_c4_shape(torch_cuda, monkeypatch):
    """The C4 shape (8 robots, 360 beams, R = 20, fan march) on a 64 x 64 grid."""
    set_knobs(monkeypatch, None, 4)
    cfg = base_cfg(numrobot=8, maxsteps=7, allow_even_beams=True, sensor_config={"num_lasers": 360, "range": 20})
    rs = np.random.RandomState(1206)
    B, K = 2, 6
    envs = pair(cfg, [bern(rs, 62, 62, 0.1) for _ in range(B)], B, auto_reset=True, seed=16)
    v = envs[0].kernel_variant()
    assert v.startswith("env_kernel<256,1,u64,C4>") and "+fan(" in v, v
    fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 8, sentinel_p=0.2), 2, "c4 shape")


def test_comm_graph_per_step_adjacency(torch_cuda, monkeypatch):
    """Every step of a launch writes its own adjacency at adj + k * stride."""
    set_knobs(monkeypatch, None, 16)
    cfg = c2_cfg(comm_radius=5, allow_comm=1)
    rs = np.random.RandomState(1207)
    B, K = 5, 40
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=17, want_adjacency=True)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2>", envs[0].kernel_variant()
    assert envs[0].adj is not None
    fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 4), 3, "comm graph")


def test_all_strides_zero(torch_cuda, monkeypatch):
    """The benchmark's form of the call: every output stride 0, K = 24 in one
    launch.  The buffers then hold step K - 1's outputs."""
    set_knobs(monkeypatch, None, None)
    torch = torch_cuda
    cfg = c2_cfg()
    rs = np.random.RandomState(1208)
    B, K = 5, 24
    fused, stepped = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=18)
    assert fused.kernel_variant() == "env_kernel<64,2,u32,C2>", fused.kernel_variant()
    acts = actions(rs, K, B, 4)
    a = torch.from_numpy(acts).to(fused.device)
    n0 = fused.env_launches()
    rc = fused.step_many_raw(a.data_ptr(), B * 4, K, fused.reward.data_ptr(), fused.done.data_ptr(),
                             fused.obs.data_ptr(), fused._stream())
    assert rc == 0, fused.lib.mc_last_error()
    assert fused.env_launches() - n0 == 1
    for k in range(K):
        o, r, d = stepped.step(a[k])
    assert torch.equal(fused.obs, o) and torch.equal(fused.done, d)
    assert fused.reward.cpu().numpy().tobytes() == r.cpu().numpy().tobytes()
    assert_same_state(fused, stepped, "strides 0")
    fused.check()


def test_ineligible_config_launches_per_step(torch_cuda, monkeypatch):
    """dijkstra_input: a second kernel follows every step's env kernel, so
    mc_step_many keeps one env-kernel launch per step."""
    set_knobs(monkeypatch, None, 16)
    cfg = c2_cfg(dijkstra_input=1)
    rs = np.random.RandomState(1209)
    B, K = 5, 12
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=19)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,C2D>", envs[0].kernel_variant()
    fused_vs_stepped(torch_cuda, envs, actions(rs, K, B, 4), K, "c2d")


def test_fork_after_a_fused_rollout(torch_cuda, monkeypatch):
    """Memory holds the whole state at launch end: a fork after a fused
    rollout, then 2 more fused steps."""
    set_knobs(monkeypatch, None, 16)
    torch = torch_cuda
    cfg = c2_cfg()
    rs = np.random.RandomState(1210)
    B = 5
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=20)
    fused_vs_stepped(torch, envs, actions(rs, 10, B, 4), 1, "before the fork")
    src = np.asarray([-1, 0, 0, -1, 3], dtype=np.int32)  # (no source is also overwritten)
    for e in envs:
        e.fork(src)
        e.check()
    assert_same_state(envs[0], envs[1], "after the fork")
    fused_vs_stepped(torch, envs, actions(rs, 2, B, 4), 1, "after the fork")


# ---- cases whose switches are read once per process: a child process each
def _child_generic():
    """MARLCOV_SPECIALIZE=0: the C2 config on the generic <64,2,u32> kernel."""
    import torch
    cfg = c2_cfg()
    rs = np.random.RandomState(1211)
    B, K = 5, 40
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=21)
    assert envs[0].kernel_variant() == "env_kernel<64,2,u32,generic>", envs[0].kernel_variant()
    fused_vs_stepped(torch, envs, actions(rs, K, B, 4), 3, "specialize 0", cfg, oracle=True)


def _child_epw1():
    """MARLCOV_EPW=1: one env per workgroup, the kernel arguments re-read at
    phase boundaries (the step's buffer offsets applied again each time)."""
    import torch
    cfg = c2_cfg()
    rs = np.random.RandomState(1212)
    B, K = 5, 40
    envs = pair(cfg, [bern(rs, 24, 22, 0.12) for _ in range(B)], B, auto_reset=True, seed=22)
    assert envs[0].kernel_variant() == "env_kernel<64,1,u32,C2>", envs[0].kernel_variant()
    fused_vs_stepped(torch, envs, actions(rs, K, B, 4), 3, "epw 1", cfg, oracle=True)


CHILDREN = {"generic": (_child_generic, {"MARLCOV_SPECIALIZE": "0"}),
            "epw1": (_child_epw1, {"MARLCOV_EPW": "1"})}


@pytest.mark.parametrize("name", sorted(CHILDREN))
def test_in_a_child_process(torch_cuda, name):
    env = dict(os.environ, MARLCOV_FUSE_STEPS="16", **CHILDREN[name][1])
    env.pop("MARLCOV_VIS_TABLE", None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), name], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{name} ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    CHILDREN[sys.argv[1]][0]()
    print(f"{sys.argv[1]} ok")

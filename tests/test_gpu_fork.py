"""GPU: fork and restore env state on the device (mc_copy_envs /
mc_sg_copy_envs, csrc/mc_fork.hip) -- ``BatchCoverageEnv.fork`` / ``sibling``
and the SuperGridRL twins.  The oracle side of a fork is ``copy.deepcopy`` of
the source env's oracle; everything is compared bit for bit (reward tolerance
0), and the envs step on against the oracle after the fork so that a field
the copy missed shows up as a diverging step."""
import copy

import numpy as np
import pytest

import test_gpu_super as sgt
from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_parity import base_cfg, bern, check_dist_mw, full_obs

pytestmark = pytest.mark.gpu

B = 8
SRC = [-1, 0, 0, 3, -1, 3, 6, 0]  # env 3 and 6 name themselves; 0 and 3 have several children


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


# ---------------------------------------------------------------------------
# DecGridRL
# ---------------------------------------------------------------------------
FORK_CASES = {
    # padded 40 x 72: 2 x 3 tile blocks with edge tiles
    "lidar_n3_38x70": (base_cfg(numrobot=3), (38, 70)),
    "n1_18x25": (base_cfg(numrobot=1), (18, 25)),
    "square_r2_n4_sharing_adj": (base_cfg(numrobot=4, sensor_type="square_sensor", sensor_config={"range": 2},
                                          map_sharing=1, comm_radius=3, allow_comm=1), (30, 30)),
    "dist_n2_64x64": (base_cfg(numrobot=2, dist_reward=1), (64, 64)),
    "dijkstra_n2": (base_cfg(numrobot=2, dijkstra_input=1, sensor_config={"num_lasers": 9, "range": 4}), (24, 28)),
    "minimap_rad3": (base_cfg(numrobot=2, mini_map_rad=3), (24, 24)),
}
DIST_CFG = FORK_CASES["dist_n2_64x64"][0]


def rand_actions(rs, n, noop=0.1):
    a = rs.randint(0, 4, size=(B, n)).astype(np.uint8)
    a[rs.rand(B, n) < noop] = rs.choice([4, 7, 200])
    return a


def do_step(torch, env, acts):
    """step -> host (obs with float layers, reward, done, adjacency or None)"""
    out, rew, done = env.step(torch.from_numpy(acts).to(env.device))
    obs, adj = out if env.adj is not None else (out, None)
    return (full_obs(env, obs, env.config), rew.cpu().numpy(), done.cpu().numpy(),
            None if adj is None else adj.cpu().numpy())


def step_against(torch, env, refs, cfg, rs, steps, tag, envs=None):
    n = cfg["numrobot"]
    envs = range(env.num_envs) if envs is None else envs
    for t in range(steps):
        acts = rand_actions(rs, n)
        obs, rew, done, adj = do_step(torch, env, acts)
        st = device_state(env)
        for b in envs:
            o, r, d = refs[b].step(ref_action(acts[b]))
            tg = f"{tag} t={t} env {b}"
            assert float(r) == rew[b], (tg, float(r), rew[b])
            assert bool(d) == bool(done[b]), tg
            np.testing.assert_array_equal(obs[b], o, err_msg=tg + " obs")
            if adj is not None:
                np.testing.assert_array_equal(adj[b], refs[b]._adjacency_matrix, err_msg=tg + " adj")
            compare_env(st, b, refs[b], tg)
        if cfg.get("dist_reward"):
            check_dist_mw(env, {b: refs[b] for b in envs}, f"{tag} t={t}")


def make_env(cfg, shape, seed, **kw):
    import marlcov
    rs = np.random.RandomState(seed)
    grids = [bern(rs, shape[0], shape[1], 0.12) for _ in range(B)]
    kw.setdefault("auto_reset", False)
    return marlcov.BatchCoverageEnv(cfg, B, grids=grids, seed=seed, **kw), rs


@pytest.mark.parametrize("name", sorted(FORK_CASES))
def test_fork_within_handle(torch_cuda, name):
    torch = torch_cuda
    cfg, shape = FORK_CASES[name]
    n = cfg["numrobot"]
    env, rs = make_env(cfg, shape, 11)
    env.reset()
    for _ in range(5):
        env.step(torch.from_numpy(rand_actions(rs, n, noop=0.2)).to(env.device))
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    env.fork(np.asarray(SRC, dtype=np.int32))
    env.check()
    clones = [refs[b] if s < 0 else copy.deepcopy(refs[s]) for b, s in enumerate(SRC)]
    st = device_state(env)
    for b in range(B):
        compare_env(st, b, clones[b], f"{name} fork env {b} <- {SRC[b]}")
    # a reset of no env returns the current-state observations.  The float
    # dist layer is the exception: a partial reset rewrites it only for maps
    # whose max(d) is unknown, so that layer is compared from
    # the next step on
    out = env.reset(env_mask=np.zeros(B, dtype=np.uint8))
    obs = full_obs(env, out[0] if env.adj is not None else out, cfg)
    for b in range(B):
        want = clones[b].get_egocentric_observations()
        if cfg.get("dist_reward") and not cfg.get("dijkstra_input"):
            obs[b][:, 3] = want[:, 3]
        np.testing.assert_array_equal(obs[b], want, err_msg=f"{name} current-state obs env {b}")
    step_against(torch, env, clones, cfg, rs, 8, name)
    env.check()


def test_fork_keeps_derived_state(torch_cuda):
    """dist_reward: a forked batch does the work its source does -- the same
    maps listed, served by the top-cell cache and fully transformed at every
    later step (MC_FIELD_DIST_TOTALS deltas), and the same outputs."""
    from marlcov import _lib
    torch = torch_cuda
    a, rs = make_env(DIST_CFG, (64, 64), 5)
    a.reset()
    bh = a.sibling(B)
    assert bh.num_envs == B and bh._cfg.auto_reset == 0
    for _ in range(10):
        a.step(torch.from_numpy(rand_actions(rs, 2)).to(a.device))
    bh.fork(torch.arange(B, dtype=torch.int32), source=a)
    tot = [e.get_state(_lib.FIELD_DIST_TOTALS).cpu().numpy() for e in (a, bh)]
    for t in range(10):
        acts = rand_actions(rs, 2)
        ra = do_step(torch, a, acts)
        rb = do_step(torch, bh, acts)
        for x, y, what in zip(ra[:3], rb[:3], ("obs", "reward", "done")):
            np.testing.assert_array_equal(x, y, err_msg=f"t={t} {what}")
        np.testing.assert_array_equal(a.dist_obs.cpu().numpy(), bh.dist_obs.cpu().numpy())
        now = [e.get_state(_lib.FIELD_DIST_TOTALS).cpu().numpy() for e in (a, bh)]
        np.testing.assert_array_equal(now[0] - tot[0], now[1] - tot[1], err_msg=f"t={t} dist totals")
        tot = now
    a.check()
    bh.check()


@pytest.mark.parametrize("dist", [0, 1])
def test_snapshot_restore_replay(torch_cuda, dist):
    from marlcov import _lib
    torch = torch_cuda
    cfg = base_cfg(numrobot=3, maxsteps=4, dist_reward=dist, sensor_config={"num_lasers": 11, "range": 4})
    env, rs = make_env(cfg, (24, 24), 21, auto_reset=True)
    env.reset()
    for _ in range(3):
        env.step(torch.from_numpy(rand_actions(rs, 3)).to(env.device))
    snap = env.sibling(3)
    slot2 = device_state(snap)
    saved = [2, 5]
    st0 = device_state(env)
    oracles = {b: oracle_from_device(st0, b, cfg) for b in saved}
    snap.fork(np.array([2, 5, -1], dtype=np.int32), source=env)
    acts = [rand_actions(rs, 3) for _ in range(6)]

    def play():
        rec = []
        for a in acts:
            obs, rew, done, _ = do_step(torch, env, a)
            st = device_state(env)
            rec.append((obs[saved], rew[saved], done[saved], st["pos"][saved], st["free"][saved],
                        st["episode"][saved], env.get_state(_lib.FIELD_EP_PC).cpu().numpy()[saved],
                        env.get_state(_lib.FIELD_EP_LEN).cpu().numpy()[saved]))
        return rec

    first = play()
    assert any(r[2].any() for r in first)  # maxsteps 4: the window crosses an auto-reset
    back = np.full(B, -1, dtype=np.int32)
    back[2], back[5] = 0, 1
    env.fork(back, source=snap)
    st = device_state(env)
    for b in saved:
        compare_env(st, b, oracles[b], f"restored env {b}")
        assert st["episode"][b] == st0["episode"][b] and st["env_grid"][b] == st0["env_grid"][b]
    for x, y in zip(first, play()):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    now = device_state(snap)
    for k in ("pos", "free", "obst", "vis", "currstep", "episode", "moved"):
        np.testing.assert_array_equal(now[k][2], slot2[k][2], err_msg=f"untouched sibling slot: {k}")
    env.check()
    snap.check()


def test_fork_in_a_captured_graph(torch_cuda):
    """The call allocates nothing, synchronises nothing and reads nothing
    back: it can be captured, and every replay forks the source's state of
    that moment."""
    torch = torch_cuda
    cfg = base_cfg(numrobot=3)
    env, rs = make_env(cfg, (20, 20), 9)
    env.reset()
    sib = env.sibling(B)
    idx = torch.arange(B, dtype=torch.int32, device=env.device)
    sib.fork(idx, source=env)  # once outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sib.fork(idx, source=env)
    for _ in range(2):
        for _ in range(3):
            env.step(torch.from_numpy(rand_actions(rs, 3)).to(env.device))
        g.replay()
        torch.cuda.synchronize()
        a, b = device_state(env), device_state(sib)
        for k in ("pos", "moved", "free", "obst", "vis", "free_cnt", "vis_cnt", "currstep", "episode"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    sib.check()


def test_fork_errors(torch_cuda):
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    cfg = base_cfg(numrobot=3)
    env, rs = make_env(cfg, (20, 20), 3)
    env.reset()
    for _ in range(4):
        env.step(torch.from_numpy(rand_actions(rs, 3)).to(env.device))
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    # env 1 names env 0, which the same call overwrites (a chain); B and -2 are
    # out of range; env 0 <- 2 and env 6 <- 5 are valid
    src = np.array([2, 0, -1, B, -2, -1, 5, -1], dtype=np.int32)
    env.fork(src)
    with pytest.raises(_lib.MarlcovError, match="0x20"):
        env.check()
    env.check()  # reported once, then clear
    clones = list(refs)
    clones[0], clones[6] = copy.deepcopy(refs[2]), copy.deepcopy(refs[5])
    st = device_state(env)
    for b in range(B):
        compare_env(st, b, clones[b], f"after bad fork env {b}")
    # incompatible handles: nothing is enqueued, the message names the field
    rs2 = np.random.RandomState(1)
    other_n = marlcov.BatchCoverageEnv(base_cfg(numrobot=2), B, grids=[bern(rs2, 20, 20, 0.1)], auto_reset=False)
    other_w = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs2, 22, 20, 0.1)], auto_reset=False)
    for other, field in ((other_n, "num_agents"), (other_w, "width")):
        with pytest.raises(_lib.MarlcovError, match=rf"\(-1\).*{field}"):
            env.fork(np.arange(B, dtype=np.int32), source=other)
    with pytest.raises(ValueError):
        env.fork(np.zeros(B - 1, dtype=np.int32))
    with pytest.raises(ValueError):
        env.fork(np.zeros(B, dtype=np.int32), source=object())
    step_against(torch, env, clones, cfg, rs, 3, "after errors")
    env.check()


# ---------------------------------------------------------------------------
# SuperGridRL
# ---------------------------------------------------------------------------
SG_CASES = {
    # planes (P + 2) * W * L = 315 B per env, bitboards of 5 words
    "scan_n1_5x21": (sgt.sg_cfg(numrobot=1, use_scanning=1), (5, 21)),
    # two words per bitboard row
    "n3_r2_dist_9x70": (sgt.sg_cfg(numrobot=3, senseradius=2, dist_reward=1), (9, 70)),
}


def sg_make(cfg, shape, seed, **kw):
    import marlcov
    rs = np.random.RandomState(seed)
    grids = [sgt.bernoulli(rs, shape[0], shape[1], 0.1) for _ in range(B)]
    pos = np.stack([sgt.draw_positions(rs, g, cfg["numrobot"]) for g in grids])
    kw.setdefault("auto_reset", False)
    env = marlcov.BatchSuperGridEnv(cfg, B, grids=grids, device="cuda", seed=seed, **kw)
    env.reset(positions=pos)
    return env, rs


def sg_actions(rs, nenv, n):
    return rs.randint(0, 4, size=(nenv, n)).astype(np.uint8), rs.randint(0, 4, size=nenv).astype(np.int32)


def sg_step(torch, env, digits, quot):
    (_, _), rew, dn = env.step(torch.from_numpy(digits).cuda(), quot=torch.from_numpy(quot))
    env.check()
    return rew.cpu().numpy(), dn.cpu().numpy()


def sg_step_against(torch, env, refs, cfg, rs, steps, tag, cut=0):
    n = cfg["numrobot"]
    for t in range(steps):
        digits, quot = sg_actions(rs, env.num_envs, n)
        rew, dn = sg_step(torch, env, digits, quot)
        st = sgt.device_state(env)
        for b, ref in refs.items():
            a = int(sum(int(d) * 4 ** i for i, d in enumerate(digits[b]))) + int(quot[b]) * 4 ** n
            _, rr, rd = ref.step(a)
            tg = f"{tag} step {t} env {b}"
            assert float(rr) == rew[b], (tg, float(rr), rew[b])
            assert bool(rd) == bool(dn[b]), tg
            sgt.compare(st, b, ref, tg)


def sg_warm(torch, env, cfg, rs, steps=5):
    """a few steps with per-env quotients, then every env's oracle rebuilt
    from the device (a_prev included)"""
    for t in range(steps):
        digits, quot = sg_actions(rs, env.num_envs, cfg["numrobot"])
        if t == steps - 1:  # neighbouring envs end with different a_prev
            quot = (np.arange(env.num_envs) % 4).astype(np.int32)
        sg_step(torch, env, digits, quot)
    st = sgt.device_state(env)
    return st, {b: sgt.oracle_from_device(st, b, cfg) for b in range(env.num_envs)}


@pytest.mark.parametrize("name", sorted(SG_CASES))
def test_sg_fork_within_handle(torch_cuda, name):
    torch = torch_cuda
    cfg, shape = SG_CASES[name]
    env, rs = sg_make(cfg, shape, 13)
    st0, refs = sg_warm(torch, env, cfg, rs)
    # the first step after the fork proves a_prev travelled: some child had another one
    assert any(s >= 0 and s != b and st0["a_prev"][b] != st0["a_prev"][s] for b, s in enumerate(SRC))
    env.fork(torch.tensor(SRC, dtype=torch.int32))
    env.check()
    planes, dist = env.planes.cpu().numpy(), env.dist.cpu().numpy()
    clones = {}
    for b, s in enumerate(SRC):
        s = b if s < 0 else s
        np.testing.assert_array_equal(planes[b], st0["planes"][s], err_msg=f"{name} planes {b} <- {s}")
        np.testing.assert_array_equal(dist[b], st0["dist"][s], err_msg=f"{name} dist {b} <- {s}")
        clones[b] = copy.deepcopy(refs[s])
    st = sgt.device_state(env)
    for b in range(B):
        sgt.compare(st, b, clones[b], f"{name} fork env {b}")
    sg_step_against(torch, env, clones, cfg, rs, 8, name)


@pytest.mark.parametrize("name", sorted(SG_CASES))
def test_sg_fork_from_sibling(torch_cuda, name):
    torch = torch_cuda
    cfg, shape = SG_CASES[name]
    env, rs = sg_make(cfg, shape, 17)
    st0, refs = sg_warm(torch, env, cfg, rs)
    sib = env.sibling(4)
    own = sgt.device_state(sib)
    src = [1, 7, -1, 3]
    sib.fork(np.asarray(src, dtype=np.int32), source=env)
    sib.check()
    planes, dist = sib.planes.cpu().numpy(), sib.dist.cpu().numpy()
    clones = {}
    for b, s in enumerate(src):
        if s < 0:  # the sibling's own env, as its reset left it
            np.testing.assert_array_equal(planes[b], own["planes"][b])
            clones[b] = sgt.oracle_from_device(own, b, cfg)
            continue
        np.testing.assert_array_equal(planes[b], st0["planes"][s], err_msg=f"{name} planes {b} <- {s}")
        np.testing.assert_array_equal(dist[b], st0["dist"][s], err_msg=f"{name} dist {b} <- {s}")
        clones[b] = copy.deepcopy(refs[s])
    st = sgt.device_state(sib)
    for b in range(4):
        sgt.compare(st, b, clones[b], f"{name} sibling env {b}")
    sg_step_against(torch, sib, clones, cfg, rs, 8, name + " sibling")
    # the source went on untouched
    sg_step_against(torch, env, refs, cfg, rs, 2, name + " source")


@pytest.mark.parametrize("name", sorted(SG_CASES))
def test_sg_snapshot_restore_replay(torch_cuda, name):
    from marlcov import _lib
    torch = torch_cuda
    cfg, shape = SG_CASES[name]
    env, rs = sg_make(cfg, shape, 19, auto_reset=True, maxsteps=4)
    st0, refs = sg_warm(torch, env, cfg, rs, steps=3)
    snap = env.sibling(3)
    slot2 = sgt.device_state(snap)
    saved = [2, 5]
    snap.fork(np.array([2, 5, -1], dtype=np.int32), source=env)
    acts = [sg_actions(rs, B, cfg["numrobot"]) for _ in range(6)]

    def play():
        rec = []
        for digits, quot in acts:
            rew, dn = sg_step(torch, env, digits, quot)
            st = sgt.device_state(env)
            rec.append((rew[saved], dn[saved]) + tuple(st[k][saved] for k in sorted(st) if k not in ("neg", "gpos"))
                       + (env.get_state(_lib.SG_FIELD_EPISODE).cpu().numpy()[saved],
                          env.get_state(_lib.SG_FIELD_EP_PC).cpu().numpy()[saved],
                          env.get_state(_lib.SG_FIELD_EP_LEN).cpu().numpy()[saved]))
        return rec

    first = play()
    assert any(r[1].any() for r in first)  # the window crosses an auto-reset
    back = np.full(B, -1, dtype=np.int32)
    back[2], back[5] = 0, 1
    env.fork(back, source=snap)
    st = sgt.device_state(env)
    for b in saved:
        sgt.compare(st, b, refs[b], f"{name} restored env {b}")
    for x, y in zip(first, play()):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    now = sgt.device_state(snap)
    for k in now:
        np.testing.assert_array_equal(now[k][2], slot2[k][2], err_msg=f"untouched sibling slot: {k}")
    snap.check()


def test_sg_fork_errors(torch_cuda):
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    cfg, shape = SG_CASES["n3_r2_dist_9x70"]
    env, rs = sg_make(cfg, shape, 23)
    st0, refs = sg_warm(torch, env, cfg, rs)
    src = np.array([2, 0, -1, B, -2, -1, 5, -1], dtype=np.int32)
    env.fork(src)
    with pytest.raises(_lib.MarlcovError, match="0x20"):
        env.check()
    env.check()
    clones = dict(refs)
    clones[0], clones[6] = copy.deepcopy(refs[2]), copy.deepcopy(refs[5])
    st = sgt.device_state(env)
    for b in range(B):
        sgt.compare(st, b, clones[b], f"after bad fork env {b}")
    rs2 = np.random.RandomState(2)
    other_n = marlcov.BatchSuperGridEnv(sgt.sg_cfg(numrobot=2, senseradius=2, dist_reward=1), B,
                                        grids=[sgt.bernoulli(rs2, 9, 70, 0.1)], auto_reset=False)
    other_l = marlcov.BatchSuperGridEnv(cfg, B, grids=[sgt.bernoulli(rs2, 9, 64, 0.1)], auto_reset=False)
    other_s = marlcov.BatchSuperGridEnv(dict(cfg, use_scanning=1), B,
                                        grids=[sgt.bernoulli(rs2, 9, 70, 0.1) for _ in range(B)], auto_reset=False)
    for other, field in ((other_n, "num_agents"), (other_l, "length"), (other_s, "use_scanning")):
        with pytest.raises(_lib.MarlcovError, match=rf"\(-1\).*{field}"):
            env.fork(np.arange(B, dtype=np.int32), source=other)
    with pytest.raises(ValueError):
        env.fork(np.zeros((B, 1), dtype=np.int32))
    sg_step_against(torch, env, clones, cfg, rs, 3, "after errors")

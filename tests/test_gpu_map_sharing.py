"""Map sharing (share_kernel, csrc/mc_grid_kernels.hip) against
DecGridRLRef.shareMaps past the shapes the other files reach: maps of more
than 64 tiles (several share workgroups per env, dead lanes in the last),
non-trivial comm graphs up to 64 robots, and sharing together with
auto-reset, a masked reset, mc_step_many, dist_reward and dijkstra_input.
Every comparison is exact: obs, reward, done, adjacency (the one reset
returns too) and, through compare_env, every agent's maps, the counters and
the positions, every step."""
import zlib

import numpy as np
import pytest

import map_sharing_cases as msc
from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from oracle.cpu_ref import DecGridRLRef
from test_gpu_parity import check_dist_mw, full_obs

pytestmark = pytest.mark.gpu

NOOP = 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def device_tiles(env):
    """Map words per agent map, from the FIELD_FREE state the device returns."""
    from marlcov import _lib
    return int(np.prod(env.get_state(_lib.FIELD_FREE).shape[2:]))


def make_env(cfg, grids, B, **kw):
    import marlcov
    kw.setdefault("auto_reset", False)
    return marlcov.BatchCoverageEnv(cfg, B, grids=grids, want_adjacency=True, **kw)


def authored(cfg, grid, cells, B):
    """B oracle envs and one device env, all reset at ``cells``; the reset's
    obs, adjacency and state are compared.  Returns (env, refs, device state)."""
    refs = []
    for b in range(B):
        np.random.seed(b)
        r = DecGridRLRef([grid], cfg)
        r.reset(False, None, positions=cells)
        refs.append(r)
    env = make_env(cfg, [grid] * B, B)
    obs, adj = env.reset(positions=np.broadcast_to(np.asarray(cells, np.int32), (B, len(cells), 2)).copy())
    st = device_state(env)
    obs_h, adj_h = full_obs(env, obs, cfg), adj.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(obs_h[b], refs[b].get_egocentric_observations(), err_msg=f"reset obs {b}")
        np.testing.assert_array_equal(adj_h[b], refs[b]._adjacency_matrix, err_msg=f"reset adj {b}")
        compare_env(st, b, refs[b], f"reset env {b}")
    return env, refs, st


def step_and_compare(torch, env, cfg, refs, acts, tag):
    """One env.step against the oracles; returns the device state after it."""
    (obs, adj), rew, done = env.step(torch.from_numpy(acts).to(env.device))
    obs_h, rew_h, done_h, adj_h = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy(), adj.cpu().numpy()
    st = device_state(env)
    for b, ref in enumerate(refs):
        o, r, d = ref.step(ref_action(acts[b]))
        t = f"{tag} env {b}"
        assert float(r) == rew_h[b], (t, float(r), rew_h[b])
        assert bool(d) == bool(done_h[b]), t
        np.testing.assert_array_equal(obs_h[b], o, err_msg=t + " obs")
        np.testing.assert_array_equal(adj_h[b], ref._adjacency_matrix, err_msg=t + " adj")
        compare_env(st, b, ref, t)
    return st


def random_actions(rs, B, N, sentinel=0.05):
    acts = rs.randint(0, 4, size=(B, N)).astype(np.uint8)
    acts[rs.rand(B, N) < 0.08] = rs.choice([4, 7, 200])
    acts[rs.rand(B) < sentinel, 0] = 255
    return acts


def known(st, b):
    return (st["free"][b] | st["obst"][b]).astype(bool)


# ---------------------------------------------------------------------------
# 1. chains: knowledge travels exactly one hop per step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,R", msc.CHAINS, ids=[f"n{n}_r{r}" for n, r in msc.CHAINS])
def test_chain_one_hop_per_step(torch_cuda, N, R):
    torch = torch_cuda
    cfg, grid, cells = msc.chain(N, R)
    B = 3
    env, refs, st0 = authored(cfg, grid, cells, B)
    assert device_tiles(env) == msc.tiles(env.width, env.length) == 96  # two share blocks, 32 dead lanes
    chain_adj = msc.chain_adjacency(N)
    k0 = known(st0, 0)
    rs = np.random.RandomState(zlib.crc32(f"chain{N}_{R}".encode()))
    # step 0: no-ops, env 1 a sentinel row -- its maps and free_cnt must not change
    acts = np.full((B, N), NOOP, np.uint8)
    acts[1, 0] = 255
    st1 = step_and_compare(torch, env, cfg, refs, acts, "noop 0")
    for key in ("free", "obst"):
        np.testing.assert_array_equal(st1[key][1], st0[key][1], err_msg=f"sentinel changed {key}")
    assert int(st1["free_cnt"][1]) == int(st0["free_cnt"][1])
    one = msc.share_one_hop(k0, chain_adj)
    for b in (0, 2):
        np.testing.assert_array_equal(known(st1, b), one, err_msg=f"one hop env {b}")
    # step 1: no-ops everywhere; env 1 lags the others by exactly one share
    acts = np.full((B, N), NOOP, np.uint8)
    st2 = step_and_compare(torch, env, cfg, refs, acts, "noop 1")
    for key in ("free", "obst"):
        np.testing.assert_array_equal(st2[key][1], st1[key][0], err_msg=f"lag {key}")
    assert int(st2["free_cnt"][1]) == int(st1["free_cnt"][0])
    two = msc.share_one_hop(one, chain_adj)
    for b in (0, 2):
        np.testing.assert_array_equal(known(st2, b), two, err_msg=f"two hops env {b}")
    assert (two != one).any()
    for t in range(10):
        step_and_compare(torch, env, cfg, refs, random_actions(rs, B, N), f"chain n{N} t={t}")
    env.check()


# ---------------------------------------------------------------------------
# 2. the radius boundary: d == R shares, d == R + 1 does not; radius 0 and a
#    complete graph
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 7])
def test_radius_boundary(torch_cuda, R):
    torch = torch_cuda
    cfg, grid, cells = msc.boundary(R)
    B = 2
    env, refs, st0 = authored(cfg, grid, cells, B)
    assert device_tiles(env) == 96
    np.testing.assert_array_equal(env.adj.cpu().numpy()[0], msc.boundary_adjacency())
    st1 = step_and_compare(torch, env, cfg, refs, np.full((B, 3), NOOP, np.uint8), f"boundary R={R}")
    for b in range(B):
        k0, k1 = known(st0, b), known(st1, b)
        np.testing.assert_array_equal(k1[2], k0[2])
        np.testing.assert_array_equal(k1[0], k0[0] | k0[1])
        np.testing.assert_array_equal(k1[1], k0[0] | k0[1])
        assert (k1[0] != k0[0]).any()
    rs = np.random.RandomState(R)
    for t in range(6):
        step_and_compare(torch, env, cfg, refs, random_actions(rs, B, 3), f"boundary R={R} t={t}")
    env.check()


@pytest.mark.parametrize("radius", [0, 72], ids=["radius0", "complete"])
def test_radius_extremes(torch_cuda, radius):
    """comm_radius = 0 with map_sharing on shares nothing; a radius of at
    least both sides of the map makes every agent's maps equal after one
    step."""
    torch = torch_cuda
    N, B = 6, 2
    cells = [(2, 2), (3, 2), (3, 3), (40, 20), (70, 40), (2, 40)]  # neighbours at distance 1 and far corners
    cfg = msc.sharing_cfg(numrobot=N, comm_radius=radius, sensor_config={"num_lasers": 9, "range": 2})
    env, refs, st0 = authored(cfg, msc.chain_grid(), cells, B)
    assert device_tiles(env) == 96
    st1 = step_and_compare(torch, env, cfg, refs, np.full((B, N), NOOP, np.uint8), f"radius {radius}")
    for b in range(B):
        if radius == 0:
            for key in ("free", "obst"):
                np.testing.assert_array_equal(st1[key][b], st0[key][b], err_msg=key)
            assert int(st1["free_cnt"][b]) == int(st0["free_cnt"][b])
        else:
            for key in ("free", "obst"):
                union = st0[key][b].max(axis=0)
                for i in range(N):
                    np.testing.assert_array_equal(st1[key][b][i], union, err_msg=f"{key} agent {i}")
            assert int(st1["free_cnt"][b]) == N * int(st0["free"][b].max(axis=0).sum())
    rs = np.random.RandomState(radius)
    for t in range(6):
        step_and_compare(torch, env, cfg, refs, random_actions(rs, B, N), f"radius {radius} t={t}")
    env.check()


# ---------------------------------------------------------------------------
# 3. random walks against the oracle (the loop of test_batch_matches_oracle,
#    with the adjacency of the reset compared too)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(msc.WALK_CASES))
def test_walk_matches_oracle(torch_cuda, name):
    torch = torch_cuda
    cfg, maker, B, T = msc.WALK_CASES[name]
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    grids = [maker(rs) for _ in range(B)]
    N = cfg["numrobot"]
    refs, pos = [], []
    for b in range(B):
        np.random.seed(1000 + b)
        r = DecGridRLRef([grids[b]], cfg)
        refs.append(r)
        pos.append(np.stack([r._xinds, r._yinds], 1))
    env = make_env(cfg, grids, B)
    assert device_tiles(env) == msc.tiles(env.width, env.length) == msc.WALK_TILES[name]
    obs, adj = env.reset(positions=np.stack(pos))
    st = device_state(env)
    obs_h, adj_h = full_obs(env, obs, cfg), adj.cpu().numpy()
    linked = 0
    for b in range(B):
        compare_env(st, b, refs[b], f"{name} reset env {b}")
        np.testing.assert_array_equal(obs_h[b], refs[b].get_egocentric_observations(),
                                      err_msg=f"{name} reset obs {b}")
        np.testing.assert_array_equal(adj_h[b], refs[b]._adjacency_matrix, err_msg=f"{name} reset adj {b}")
        linked += int(refs[b]._adjacency_matrix.sum()) - N
    for t in range(T):
        step_and_compare(torch, env, cfg, refs, random_actions(rs, B, N), f"{name} t={t}")
        linked += sum(int(r._adjacency_matrix.sum()) - N for r in refs)
        if cfg.get("dist_reward"):
            check_dist_mw(env, refs, f"{name} t={t}")
    assert linked > 0, "the comm graph was the identity all along"
    env.check()


# ---------------------------------------------------------------------------
# 4. auto-reset: the step after a reset shares over the new positions' graph
#    and the fresh maps
# ---------------------------------------------------------------------------
def test_sharing_with_auto_reset(torch_cuda):
    torch = torch_cuda
    from marlcov import _lib
    N, B = 5, 16
    cfg = msc.sharing_cfg(numrobot=N, comm_radius=6, maxsteps=6, sensor_config={"num_lasers": 11, "range": 4})
    rs = np.random.RandomState(7)
    grids = [msc.bern(rs, 36, 70, 0.2) for _ in range(B)]
    env = make_env(cfg, grids, B, auto_reset=True, seed=123)
    assert device_tiles(env) == 96
    obs, adj = env.reset()
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    adj_h = adj.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(adj_h[b], refs[b]._adjacency_matrix, err_msg=f"reset adj {b}")
        compare_env(st, b, refs[b], f"reset env {b}")
    resets = np.zeros(B, int)
    for t in range(20):
        acts = rs.randint(0, 4, size=(B, N)).astype(np.uint8)
        acts[rs.rand(B) < 0.08, 0] = 255  # a sentinel's done resets the env too
        (obs, adj), rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs_h, rew_h, done_h, adj_h = (full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy(),
                                       adj.cpu().numpy())
        st = device_state(env)
        ep_pc = env.get_state(_lib.FIELD_EP_PC).cpu().numpy()
        ep_len = env.get_state(_lib.FIELD_EP_LEN).cpu().numpy()
        for b in range(B):
            o, r, d = refs[b].step(ref_action(acts[b]))
            assert float(r) == rew_h[b] and bool(d) == bool(done_h[b]), (t, b, float(r), rew_h[b])
            if d:
                assert ep_pc[b] == refs[b].percent_covered() and ep_len[b] == refs[b]._currstep, (t, b)
                resets[b] += 1
                p = st["pos"][b]
                assert len({tuple(q) for q in p}) == N
                o, _ = refs[b].reset(False, None, positions=[tuple(q) for q in p])
                assert int(st["currstep"][b]) == 0
            np.testing.assert_array_equal(obs_h[b], o, err_msg=f"t={t} env {b}")
            np.testing.assert_array_equal(adj_h[b], refs[b]._adjacency_matrix, err_msg=f"t={t} env {b} adj")
            compare_env(st, b, refs[b], f"t={t} env {b}")
    assert resets.min() >= 1  # maxsteps=6 over 20 steps: every env reset at least once
    env.check()


# ---------------------------------------------------------------------------
# 5. a masked partial reset: the untouched envs keep sharing undisturbed
# ---------------------------------------------------------------------------
def test_sharing_with_masked_reset(torch_cuda):
    torch = torch_cuda
    N, B = 5, 6
    cfg = msc.sharing_cfg(numrobot=N, comm_radius=6, sensor_config={"num_lasers": 11, "range": 4})
    rs = np.random.RandomState(17)
    grids = [msc.bern(rs, 36, 70, 0.15) for _ in range(B)]
    refs, pos = [], []
    for b in range(B):
        np.random.seed(300 + b)
        r = DecGridRLRef([grids[b]], cfg)
        refs.append(r)
        pos.append(np.stack([r._xinds, r._yinds], 1))
    env = make_env(cfg, grids, B)
    assert device_tiles(env) == 96
    env.reset(positions=np.stack(pos))
    for t in range(6):  # steps 0..5
        step_and_compare(torch, env, cfg, refs, random_actions(rs, B, N, sentinel=0.0), f"before t={t}")
    st = device_state(env)
    mask = np.zeros(B, np.uint8)
    mask[[1, 4]] = 1
    cells = st["pos"].copy()
    # a tight cluster (the fresh graph is not the identity) across the edge of
    # the second share block's tiles (x >= 32, y >= 32 on this 38 x 72 map)
    for b in (1, 4):
        free = np.argwhere(refs[b]._grid[30:37, 40:47] >= 0) + (30, 40)
        cells[b] = free[rs.choice(len(free), N, replace=False)]
    obs, adj = env.reset(env_mask=mask, positions=cells)
    obs_h, adj_h = full_obs(env, obs, cfg), adj.cpu().numpy()
    st = device_state(env)
    for b in range(B):
        if mask[b]:
            o, _ = refs[b].reset(False, None, positions=[tuple(q) for q in cells[b]])
            assert refs[b]._adjacency_matrix.sum() > N
            np.testing.assert_array_equal(adj_h[b], refs[b]._adjacency_matrix, err_msg=f"masked reset adj {b}")
        else:
            o = refs[b].get_egocentric_observations()
        np.testing.assert_array_equal(obs_h[b], o, err_msg=f"masked reset obs {b}")
        compare_env(st, b, refs[b], f"masked reset env {b}")
    for t in range(10):
        step_and_compare(torch, env, cfg, refs, random_actions(rs, B, N), f"after t={t}")
    env.check()


# ---------------------------------------------------------------------------
# 6. mc_step_many: the per-step path reads step k's action row for the
#    share's sentinel test
# ---------------------------------------------------------------------------
def test_sharing_step_many(torch_cuda):
    torch = torch_cuda
    N, B, K = 5, 4, 9
    cfg = msc.sharing_cfg(numrobot=N, comm_radius=6, sensor_config={"num_lasers": 11, "range": 4})
    rs = np.random.RandomState(29)
    grids = [msc.bern(rs, 36, 70, 0.15) for _ in range(B)]
    refs, pos = [], []
    for b in range(B):  # start in and around the second share block's tiles (x >= 32, y >= 32)
        np.random.seed(400 + b)
        r = DecGridRLRef([grids[b]], cfg)
        free = np.argwhere(r._grid[26:37, 34:56] >= 0) + (26, 34)
        cells = free[rs.choice(len(free), N, replace=False)]
        r.reset(False, None, positions=[tuple(q) for q in cells])
        refs.append(r)
        pos.append(cells)
    many, stepped = make_env(cfg, grids, B), make_env(cfg, grids, B)
    assert device_tiles(many) == 96
    for e in (many, stepped):
        e.reset(positions=np.stack(pos))
    acts = np.stack([random_actions(rs, B, N, sentinel=0.0) for _ in range(K)])
    for k, b in ((0, 2), (1, 0), (3, 3), (4, 1), (4, 2), (7, 0)):  # sentinel rows: other envs at other k
        acts[k, b, 0] = 255
    n0 = many.env_launches()
    (obs_r, adj_r), rew_r, done_r = many.rollout(torch.from_numpy(acts).to(many.device))
    assert many.env_launches() - n0 == K  # one env-kernel launch per step: not fused
    obs_r, adj_r, rew_r, done_r = obs_r.cpu().numpy(), adj_r.cpu().numpy(), rew_r.cpu().numpy(), done_r.cpu().numpy()
    for k in range(K):
        (o, a), r, d = stepped.step(torch.from_numpy(acts[k]).to(stepped.device))
        tag = f"k={k}"
        np.testing.assert_array_equal(obs_r[k], o.cpu().numpy(), err_msg=tag + " obs twin")
        np.testing.assert_array_equal(adj_r[k], a.cpu().numpy(), err_msg=tag + " adj twin")
        np.testing.assert_array_equal(rew_r[k], r.cpu().numpy(), err_msg=tag + " reward twin")
        np.testing.assert_array_equal(done_r[k], d.cpu().numpy(), err_msg=tag + " done twin")
        for b in range(B):
            oo, rr, dd = refs[b].step(ref_action(acts[k, b]))
            t = f"{tag} env {b}"
            assert float(rr) == rew_r[k, b] and bool(dd) == bool(done_r[k, b]), (t, float(rr), rew_r[k, b])
            np.testing.assert_array_equal(obs_r[k, b].astype(np.float64), oo, err_msg=t + " obs")
            np.testing.assert_array_equal(adj_r[k, b], refs[b]._adjacency_matrix, err_msg=t + " adj")
    st_m, st_s = device_state(many), device_state(stepped)
    for key in st_m:
        np.testing.assert_array_equal(st_m[key], st_s[key], err_msg=key)
    for b in range(B):
        compare_env(st_m, b, refs[b], f"end env {b}")
    for e in (many, stepped):
        e.check()

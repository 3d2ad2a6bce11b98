"""GPU: mc_frontier_actions (BatchCoverageEnv.frontier / frontier_actions,
marlcov.episodes.frontier_policy) against the oracle's dijkstra_path_map
through tests/frontier_ref.py: action, distance and goal of every agent
bit-exact, on every kernel choice, and the call changes nothing of the env."""
import ctypes

import numpy as np
import pytest

from frontier_ref import ACT_STAY, action_from_layer, expected_all
from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from oracle.cpu_ref import DecGridRLRef

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def base_cfg(**kw):
    c = dict(numrobot=1, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0,
             terminal_reward=30, dist_reward=0, train_maxsteps=1000, test_maxsteps=1000,
             egoradius=2, mini_map_rad=0, comm_radius=0, allow_comm=0, map_sharing=0,
             single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
             sensor_config={"num_lasers": 21, "range": 10})
    c.update(kw)
    return c


def bern(rs, w, l, p):
    return rs.choice([1.0, -1.0], size=(w, l), p=[1 - p, p])


def check_frontier(env, refs, tag):
    """env.frontier() of the current state against the oracle envs."""
    act, dist, goal = (t.cpu().numpy() for t in env.frontier())
    assert act.dtype == np.uint8 and dist.dtype == np.int32 and goal.dtype == np.int32
    for b, ref in enumerate(refs):
        ea, ed, eg = expected_all(ref)
        np.testing.assert_array_equal(act[b], ea, err_msg=f"{tag} env {b} actions (dist {ed})")
        np.testing.assert_array_equal(dist[b], ed, err_msg=f"{tag} env {b} dist")
        np.testing.assert_array_equal(goal[b], eg, err_msg=f"{tag} env {b} goal")
    return act, dist, goal


# ---------------------------------------------------------------------------
# 1. a random walk: the call before every step, the state after it
# ---------------------------------------------------------------------------
WALK_SENSORS = {
    "lidar": dict(sensor_config={"num_lasers": 9, "range": 3}),
    "square": dict(sensor_type="square_sensor", sensor_config={"range": 1}, single_square_tool=1, egoradius=1),
}


@pytest.mark.parametrize("sensor", sorted(WALK_SENSORS))
def test_random_walk_matches_oracle(torch_cuda, monkeypatch, sensor):
    import marlcov
    torch = torch_cuda
    for v in ("MARLCOV_DJ_FULL", "MARLCOV_DJ_BIG", "MARLCOV_DJ_BIG_GRID"):
        monkeypatch.delenv(v, raising=False)
    cfg = base_cfg(numrobot=3, **WALK_SENSORS[sensor])
    rs = np.random.RandomState(17)
    B, N = 6, 3
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, 30, 26, 0.15) for _ in range(B)], auto_reset=False)
    obs = env.reset()
    assert obs.shape[2] == 3
    assert env.frontier_variant() == ""
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    moves = 0
    for t in range(25):
        act, _, _ = check_frontier(env, refs, f"walk {sensor} t={t}")
        moves += int((act != ACT_STAY).sum())
        acts = rs.randint(0, 5, size=(B, N)).astype(np.uint8)
        obs, rew, done = env.step(torch.from_numpy(acts).to(env.device))
        assert obs.shape[2] == 3
        rew_h, done_h = rew.cpu().numpy(), done.cpu().numpy()
        st = device_state(env)
        for b in range(B):
            _, r, d = refs[b].step(ref_action(acts[b]))
            tag = f"walk {sensor} t={t} env {b}"
            assert float(r) == rew_h[b] and bool(d) == bool(done_h[b]), tag
            compare_env(st, b, refs[b], tag)  # the call changed nothing
    assert env.frontier_variant() == "window+lds"
    assert moves > B * N * 25 // 2
    # the actions alone, into a tensor of the caller's
    out = torch.full((B, N), 9, dtype=torch.uint8, device=env.device)
    assert env.frontier_actions(out=out) is out
    assert torch.equal(out, env.frontier()[0])
    with pytest.raises(ValueError):
        env.frontier_actions(out=torch.zeros((B, N), dtype=torch.int32, device=env.device))
    with pytest.raises(ValueError):
        env.frontier(goal=torch.zeros((B, N), dtype=torch.int32, device=env.device))
    env.check()


# ---------------------------------------------------------------------------
# 2. far targets and edge cases on every kernel choice
# ---------------------------------------------------------------------------
FAR_MODES = {
    "window+lds": {},
    "lds": {"MARLCOV_DJ_FULL": "1"},
    "window+hbm": {"MARLCOV_DJ_BIG": "1", "MARLCOV_DJ_BIG_GRID": "2"},
    "hbm": {"MARLCOV_DJ_FULL": "1", "MARLCOV_DJ_BIG": "1", "MARLCOV_DJ_BIG_GRID": "2"},
}
FAR_DEPTHS = [1, 6, 22, 23, 24, 25, 26, 31, 45, 200]


def set_far_mode(monkeypatch, variant):
    for v in ("MARLCOV_DJ_FULL", "MARLCOV_DJ_BIG", "MARLCOV_DJ_BIG_GRID", "MARLCOV_DJ_DEPTH"):
        monkeypatch.delenv(v, raising=False)
    for k, v in FAR_MODES[variant].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("variant", list(FAR_MODES))
def test_far_targets_and_edge_cases(torch_cuda, monkeypatch, variant):
    """The explored L1 diamond around each robot has a depth on both sides of
    the window kernel's 24 layers; depth 200 explores the whole map (the pad
    ring walled off by the observed border: empty path).  One agent stands on
    an unexplored cell, two robots one cell from the border ring."""
    import marlcov
    from marlcov import _lib
    from marlcov.tiles import cells_to_tiles
    torch = torch_cuda
    set_far_mode(monkeypatch, variant)
    cfg = base_cfg(numrobot=3, sensor_config={"num_lasers": 9, "range": 3})
    rs = np.random.RandomState(11)
    B, N = 8, 3
    grid = bern(rs, 72, 60, 0.08)
    grid[0, 0] = grid[-1, -1] = 1.0  # padded cells (1, 1) and (W - 2, L - 2)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[grid], auto_reset=False)
    W, L = env.width, env.length
    free_cells = np.argwhere(grid > 0) + 1  # padded coordinates
    pos = np.stack([free_cells[rs.choice(len(free_cells), N, replace=False)] for _ in range(B)]).astype(np.int32)
    pos[2, 0] = (1, 1)
    pos[3, 2] = (W - 2, L - 2)
    assert all(len({tuple(q) for q in pos[b]}) == N for b in range(B))
    env.reset(positions=pos)
    st = device_state(env)
    np.testing.assert_array_equal(st["pos"], pos)
    X, Y = np.meshgrid(np.arange(W), np.arange(L), indexing="ij")
    free = np.zeros((B, N, W, L), np.uint8)
    obst = np.zeros((B, N, W, L), np.uint8)
    neg = st["neg"][0][:W, :L]
    want_depth = {}
    for b in range(B):
        for i in range(N):
            D = FAR_DEPTHS[(b + 4 * i) % len(FAR_DEPTHS)]
            want_depth[D] = (b, i)
            x, y = pos[b, i]
            near = (np.abs(X - x) + np.abs(Y - y)) < D
            free[b, i] = near & (neg == 0)
            obst[b, i] = near & (neg == 1)
    assert sorted(want_depth) == sorted(FAR_DEPTHS)
    free[1, 1, pos[1, 1, 0], pos[1, 1, 1]] = 0  # this agent's own cell is unexplored (its diamond: 25)
    vis = free.max(axis=1)

    def put(field, a):
        env.set_state(field, torch.from_numpy(np.ascontiguousarray(a)))

    put(_lib.FIELD_FREE, cells_to_tiles(free, blocks=True).view(np.int64))
    put(_lib.FIELD_OBST, cells_to_tiles(obst, blocks=True).view(np.int64))
    put(_lib.FIELD_VISITED, cells_to_tiles(vis, blocks=True).view(np.int64))
    put(_lib.FIELD_FREE_COUNT, free.reshape(B, -1).sum(1).astype(np.int32))
    put(_lib.FIELD_VISITED_COUNT, vis.reshape(B, -1).sum(1).astype(np.int32))
    st = device_state(env)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    act, dist, goal = check_frontier(env, refs, f"far {variant}")
    assert env.frontier_variant() == variant
    # the cases this test is about are all there
    assert dist[1, 1] == 0 and act[1, 1] == ACT_STAY and tuple(goal[1, 1]) == tuple(pos[1, 1])
    for b, i in ((5, 1), (1, 2)):  # depth 200: fully explored and walled off
        assert FAR_DEPTHS[(b + 4 * i) % len(FAR_DEPTHS)] == 200
        assert dist[b, i] == -1 and act[b, i] == ACT_STAY and tuple(goal[b, i]) == tuple(pos[b, i])
    assert dist.max() > 24 and 0 < dist[dist > 0].min() <= 24  # both sides of the window's depth
    # a second call (the list protocol left its count words ready) gives the same
    again = env.frontier()
    assert all(np.array_equal(a.cpu().numpy(), b_) for a, b_ in zip(again, (act, dist, goal)))
    st2 = device_state(env)
    for b in range(B):
        compare_env(st2, b, refs[b], f"far {variant} env {b}")
    env.check()


# ---------------------------------------------------------------------------
# 3. a dijkstra_input handle: its own layer, list and launch count stay
# ---------------------------------------------------------------------------
def test_dijkstra_input_handle_keeps_its_layer_and_list(torch_cuda, monkeypatch):
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    set_far_mode(monkeypatch, "window+lds")
    cfg = base_cfg(numrobot=3, dijkstra_input=1, sensor_config={"num_lasers": 9, "range": 3})
    rs = np.random.RandomState(23)
    B, N = 6, 3
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, 30, 26, 0.15) for _ in range(B)], auto_reset=False)
    env.reset()
    moves = 0
    for t in range(5):
        acts = rs.randint(0, 5, size=(B, N)).astype(np.uint8)
        obs, _, _ = env.step(torch.from_numpy(acts).to(env.device))
        obs_before = obs.clone()
        listed_before = env.get_state(_lib.FIELD_DJ_LISTED).clone()
        launches = env.env_launches()
        got = env.frontier_actions().cpu().numpy()
        assert env.env_launches() == launches
        assert torch.equal(env.get_state(_lib.FIELD_DJ_LISTED), listed_before)
        assert torch.equal(env.obs, obs_before)
        layer = obs_before.cpu().numpy()[:, :, 3]
        want = np.array([[action_from_layer(layer[b, i]) for i in range(N)] for b in range(B)], np.uint8)
        np.testing.assert_array_equal(got, want, err_msg=f"t={t}")
        moves += int((want != ACT_STAY).sum())
    assert moves > 0
    assert env.frontier_variant() == env.dijkstra_variant() == "window+lds"
    env.check()


# ---------------------------------------------------------------------------
# 4. closed loop: the greedy follower against an oracle driven by the helper
# ---------------------------------------------------------------------------
def test_closed_loop_follows_the_oracle(torch_cuda, monkeypatch):
    """N = 1: rewards, dones and percent_covered of every device step equal an
    oracle driven by the helper's action.  On the CPU that oracle covered maps
    1..3 at 100 % in 132, 145 and 154 steps; map 0 has one free cell no path
    reaches, so its follower covers 99.7 % and then stays put (dist -1) until
    maxsteps = 400 ends the episode: the floor below is what that run met."""
    import marlcov
    set_far_mode(monkeypatch, "window+lds")
    cfg = base_cfg(numrobot=1, maxsteps=400, sensor_config={"num_lasers": 9, "range": 3})
    rs = np.random.RandomState(5)
    B = 4
    grids = [bern(rs, 22, 18, 0.15) for _ in range(B)]
    refs, pos = [], []
    for b in range(B):
        np.random.seed(b)
        r = DecGridRLRef([grids[b]], cfg)
        refs.append(r)
        pos.append(np.stack([r._xinds, r._yinds], 1))
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=False)
    env.reset(positions=np.stack(pos))
    finished = np.zeros(B, bool)
    steps = 0
    while not finished.all():
        assert steps < 400
        want = np.stack([expected_all(r)[0] for r in refs])
        a = env.frontier_actions()
        np.testing.assert_array_equal(a.cpu().numpy(), want, err_msg=f"t={steps}")
        _, rew, done = env.step(a)
        rew_h, done_h, pc = rew.cpu().numpy(), done.cpu().numpy(), env.percent_covered().cpu().numpy()
        for b in range(B):
            _, r, d = refs[b].step(ref_action(want[b]))
            assert float(r) == rew_h[b] and bool(d) == bool(done_h[b]), (steps, b)
            assert refs[b].percent_covered() == pc[b], (steps, b)
            finished[b] |= bool(d)
        steps += 1
    assert steps == 400 and all(r.percent_covered() >= 0.99 for r in refs)
    assert [r.percent_covered() >= 1.0 for r in refs] == [False, True, True, True]
    env.check()


# ---------------------------------------------------------------------------
# 5. the episode driver with frontier_policy
# ---------------------------------------------------------------------------
def test_frontier_policy_drives_generate_episodes(torch_cuda, monkeypatch):
    import marlcov
    from marlcov.episodes import episode_config, frontier_policy, generate_episodes
    set_far_mode(monkeypatch, "window+lds")
    c = episode_config(base_cfg(numrobot=3, done_thresh=0.35, done_incr=0.1, test_maxsteps=14,
                                sensor_config={"num_lasers": 11, "range": 4}), testing=True)
    rs = np.random.RandomState(31)
    B, E = 8, 2
    env = marlcov.BatchCoverageEnv(c, B, grids=[bern(rs, 16, 16, 0.15) for _ in range(B)], auto_reset=True, seed=9)
    env.reset()
    st = device_state(env)
    refs = [oracle_from_device(st, b, c) for b in range(B)]
    seen = {"steps": 0, "moves": 0}

    def on_step(t, actions, reward, done):
        acts = actions.cpu().numpy()
        rew, dn = reward.cpu().numpy(), done.cpu().numpy()
        s = device_state(env)
        for b in range(B):
            # refs[b] still holds the pre-step state: the policy's action is its frontier move
            np.testing.assert_array_equal(acts[b], expected_all(refs[b])[0], err_msg=f"t={t} env {b}")
            _, r, d = refs[b].step(ref_action(acts[b]))
            assert float(r) == rew[b] and bool(d) == bool(dn[b]), (t, b)
            if d:
                refs[b].reset(False, None, positions=[tuple(q) for q in s["pos"][b]])
        seen["steps"] += 1
        seen["moves"] += int((acts != ACT_STAY).sum())

    out = generate_episodes(env, frontier_policy(env), E, max_steps=400, on_step=on_step)
    assert out["length"].shape == (B, E)
    assert (out["length"] <= c["maxsteps"]).all() and (out["length"] > 0).all()
    assert seen["steps"] == out["steps"] and seen["moves"] > 0
    with pytest.raises(ValueError, match="BatchSuperGridEnv"):
        scfg = dict(numrobot=2, train_maxsteps=10, test_maxsteps=10, collision_penalty=5, senseradius=1,
                    free_penalty=0.2, done_thresh=1, done_incr=0, terminal_reward=30, dist_reward=0, use_scanning=0)
        frontier_policy(marlcov.BatchSuperGridEnv(scfg, 2, grids=[bern(rs, 8, 8, 0.1)], auto_reset=True))


# ---------------------------------------------------------------------------
# 6. errors and the allocation's size
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["window+lds", "window+hbm"])
def test_errors_and_state_bytes(torch_cuda, monkeypatch, variant):
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    set_far_mode(monkeypatch, variant)
    cfg = base_cfg(numrobot=3, sensor_config={"num_lasers": 9, "range": 3})
    rs = np.random.RandomState(2)
    B, N = 4, 3
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, 30, 26, 0.15)], auto_reset=False)
    env.reset()
    lib, h = env.lib, env._h
    out = torch.zeros((B, N), dtype=torch.uint8, device=env.device)
    assert lib.mc_frontier_variant(h) == b""
    assert lib.mc_frontier_actions(h, out.data_ptr(), None, None, env._stream()) == _lib.MC_ESTATE
    assert b"mc_frontier_setup" in lib.mc_last_error()
    assert lib.mc_frontier_actions(h, None, None, None, env._stream()) == _lib.MC_EINVAL
    assert b"dev_actions" in lib.mc_last_error()

    def state_bytes():
        lay = _lib.McLayout()
        _lib.check(lib.mc_query(h, ctypes.byref(lay)), "mc_query")
        return lay.state_bytes

    before = state_bytes()
    assert lib.mc_frontier_setup(h) == _lib.MC_OK
    grew = (B * N + 3) * 4  # count, done, last count and the items
    if variant.endswith("hbm"):
        rx, rw = env.width + 2 * env.pad, -(-(env.length + 2 * env.pad) // 64)
        grew += 2 * 7 * rx * rw * 8  # MARLCOV_DJ_BIG_GRID = 2 slots of seven planes
    assert state_bytes() == before + grew
    assert lib.mc_frontier_setup(h) == _lib.MC_OK  # idempotent
    assert state_bytes() == before + grew
    assert lib.mc_frontier_variant(h) == variant.encode()
    assert lib.mc_frontier_actions(h, None, None, None, env._stream()) == _lib.MC_EINVAL
    assert lib.mc_frontier_actions(h, out.data_ptr(), None, None, env._stream()) == _lib.MC_OK
    env.check()
    assert int(out.max()) <= ACT_STAY

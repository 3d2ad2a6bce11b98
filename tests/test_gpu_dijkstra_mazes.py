"""GPU: the BFS path kernels of csrc/mc_dijkstra.hip on the authored mazes of
dijkstra_maze_cases.py -- detours behind a wall, corridors that wind for
thousands of layers, forks whose ends tie, rings and wide corridors whose walks
back tie, sealed chambers, wall-ring targets, corridors on the bitboards' word
boundaries -- against the oracle's dijkstra_path_map, bit-exact, on all four
kernel choices (window+lds, lds, window+hbm, hbm) and through both sinks: the
move, distance and goal of mc_frontier_actions, and dijkstra_input's obs layer
at the largest crop (31 x 31) and at 5 x 5.  What each case is there for is
asserted on the oracle alone in test_dijkstra_maze_cases_cpu.py."""
import numpy as np
import pytest

import dijkstra_maze_cases as mz
from frontier_ref import ACT_STAY, expected_all, planning_map
from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_frontier import FAR_MODES, set_far_mode
from test_gpu_parity import full_obs

pytestmark = pytest.mark.gpu

WINDOW_MODES = ("window+lds", "window+hbm")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def authored_env(torch, cases, cfg):
    """A BatchCoverageEnv holding the cases, env b on grid b: reset onto the authored start
    cells, then the authored planes and counters put in place of what the reset sensed."""
    import marlcov
    from marlcov import _lib
    from marlcov.tiles import cells_to_tiles
    B = len(cases)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[c.grid for c in cases], auto_reset=False,
                                   env_grid=np.arange(B, dtype=np.int32))
    want = mz.batch_state(cases)
    assert (env.width, env.length) == cases[0].shape and env.num_agents == want["pos"].shape[1]
    env.reset(positions=want["pos"])

    def put(f, a):
        env.set_state(f, torch.from_numpy(np.ascontiguousarray(a)))

    put(_lib.FIELD_FREE, cells_to_tiles(want["free"], blocks=True).view(np.int64))
    put(_lib.FIELD_OBST, cells_to_tiles(want["obst"], blocks=True).view(np.int64))
    put(_lib.FIELD_VISITED, cells_to_tiles(want["vis"], blocks=True).view(np.int64))
    put(_lib.FIELD_FREE_COUNT, want["free_cnt"])
    put(_lib.FIELD_VISITED_COUNT, want["vis_cnt"])
    st = device_state(env)
    np.testing.assert_array_equal(st["env_grid"], np.arange(B))
    np.testing.assert_array_equal(st["pos"], want["pos"])
    np.testing.assert_array_equal(st["free"], want["free"])
    np.testing.assert_array_equal(st["obst"], want["obst"])
    for b, c in enumerate(cases):
        np.testing.assert_array_equal(st["neg"][b][:env.width, :env.length], ~c.canvas.free)
    return env, st


# ---------------------------------------------------------------------------
# 1. the move sink: mc_frontier_actions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam", mz.FAMILIES)
@pytest.mark.parametrize("variant", list(FAR_MODES))
def test_move_sink(torch_cuda, monkeypatch, variant, fam):
    """Action, distance and goal of every agent equal frontier_ref.expected_all of the oracle
    rebuilt from the device's state (and what the case declares); a second call gives the
    same; the call changes nothing of the env."""
    set_far_mode(monkeypatch, variant)
    ego = 2
    cases = mz.family(fam, ego)
    B, N = len(cases), len(cases[0].agents)
    cfg = mz.square_cfg(N, ego)
    env, st = authored_env(torch_cuda, cases, cfg)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    act, dist, goal = (t.cpu().numpy() for t in env.frontier())
    assert env.frontier_variant() == variant
    for b, (case, ref) in enumerate(zip(cases, refs)):
        ea, ed, eg = expected_all(ref)
        tag = f"{variant} {case.name}"
        np.testing.assert_array_equal(dist[b], ed, err_msg=tag + " dist")
        np.testing.assert_array_equal(goal[b], eg, err_msg=tag + f" goal (dist {ed})")
        np.testing.assert_array_equal(act[b], ea, err_msg=tag + f" actions (dist {ed})")
        for i, a in enumerate(case.agents):  # the oracle met the declaration: so does the device
            assert dist[b, i] == a.d, (tag, i)
            assert tuple(goal[b, i]) == tuple(a.end if a.d >= 0 else a.start), (tag, i)
            if a.d <= 0:
                assert act[b, i] == ACT_STAY, (tag, i)
    again = env.frontier()
    assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(again, (act, dist, goal)))
    st2 = device_state(env)
    for b in range(B):
        compare_env(st2, b, refs[b], f"{variant} {cases[b].name}")
    env.check()


# ---------------------------------------------------------------------------
# 2. the crop sink: dijkstra_input's obs layer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam", mz.FAMILIES)
@pytest.mark.parametrize("ego", mz.EGOS, ids=["ego15", "ego2"])
@pytest.mark.parametrize("variant", list(FAR_MODES))
def test_crop_sink(torch_cuda, monkeypatch, variant, ego, fam):
    """Four steps against the oracle, the first of no-ops and three of random moves: obs of
    every layer, reward (exact), done and compare_env each step, and MC_FIELD_DJ_LISTED equal
    to the number of items window_lists predicts on the oracle's maps after the step (every
    item where the full-map kernel takes them all)."""
    from marlcov import _lib
    torch = torch_cuda
    set_far_mode(monkeypatch, variant)
    cases = mz.family(fam, ego)
    B, N = len(cases), len(cases[0].agents)
    cfg = mz.square_cfg(N, ego, dijkstra_input=1)
    env, st = authored_env(torch, cases, cfg)
    assert env.dijkstra_variant() == variant
    E = env.obs_shape[-1]
    assert E == 2 * ego + 1 and (ego != mz.EGO_MAX or E == 31)
    refs = [oracle_from_device(st, b, cfg) for b in range(B)]
    rs = np.random.RandomState(len(fam) + ego)
    counts = []
    for t in range(4):
        acts = (np.full((B, N), 4) if t == 0 else rs.randint(0, 4, size=(B, N))).astype(np.uint8)
        obs, rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs_h, rew_h, done_h = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
        listed = int(env.get_state(_lib.FIELD_DJ_LISTED).item())
        st = device_state(env)
        want = 0
        for b in range(B):
            o, r, d = refs[b].step(ref_action(acts[b]))
            tag = f"{variant} ego {ego} {cases[b].name} t={t}"
            assert float(r) == rew_h[b], (tag, float(r), rew_h[b])
            assert bool(d) == bool(done_h[b]), tag
            np.testing.assert_array_equal(obs_h[b], o, err_msg=tag + " obs")
            compare_env(st, b, refs[b], tag)
            want += sum(mz.window_lists(*planning_map(refs[b], i)) for i in range(N))
        counts.append(want)
        assert listed == (want if variant in WINDOW_MODES else B * N), (variant, fam, ego, t, listed, want)
    print(f"listed {fam} ego {ego} {variant}: predicted {counts} of {B * N} items")
    env.check()


# ---------------------------------------------------------------------------
# 3. closed loop: the greedy follower through a serpentine and a spiral
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("variant", ["window+lds", "hbm"])
def test_closed_loop_on_mazes(torch_cuda, monkeypatch, variant, n):
    """The device stepped by its own frontier_actions() beside oracles driven by
    frontier_ref.expected_all: equal actions, rewards, dones and percent_covered every step,
    and 100 % coverage after the steps the reference loop takes on the CPU (LOOP_STEPS,
    asserted there as well)."""
    import marlcov
    set_far_mode(monkeypatch, variant)
    kinds = ("serpentine", "spiral")
    cfg = mz.loop_cfg(n)
    B = len(kinds)
    refs = [mz.loop_oracle(k, n) for k in kinds]
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[mz.loop_grid(k) for k in kinds], auto_reset=False,
                                   env_grid=np.arange(B, dtype=np.int32))
    env.reset(positions=np.array([mz.LOOP_STARTS[n]] * B, dtype=np.int32))
    st = device_state(env)
    for b in range(B):
        compare_env(st, b, refs[b], f"{kinds[b]} reset")
    finished = [None] * B
    steps = 0
    while None in finished:
        assert steps < 1000
        want = np.stack([expected_all(r)[0] for r in refs])
        a = env.frontier_actions()
        np.testing.assert_array_equal(a.cpu().numpy(), want, err_msg=f"t={steps}")
        _, rew, done = env.step(a)
        rew_h, done_h, pc = rew.cpu().numpy(), done.cpu().numpy(), env.percent_covered().cpu().numpy()
        steps += 1
        for b in range(B):
            _, r, d = refs[b].step(ref_action(want[b]))
            assert float(r) == rew_h[b] and bool(d) == bool(done_h[b]), (steps, b)
            assert refs[b].percent_covered() == pc[b], (steps, b)
            if d and finished[b] is None:
                finished[b] = steps
                assert pc[b] >= 1.0
    assert env.frontier_variant() == variant
    assert finished == [mz.LOOP_STEPS[(k, n)] for k in kinds]
    st = device_state(env)
    for b in range(B):
        compare_env(st, b, refs[b], f"{kinds[b]} end")
    env.check()

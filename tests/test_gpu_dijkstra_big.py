"""dijkstra_input with the full-map BFS planes in HBM (csrc/mc_dijkstra.hip
dijkstra_big_kernel): maps whose bitboards exceed one workgroup's LDS, and
small maps forced onto the kernel (MARLCOV_DJ_BIG=1) where the oracle is
cheap.  Every test steps against the oracle (dijkstra.py:112-187 through
dec_grid_rl.py:354-358): obs of every layer, reward (exact), done, positions,
maps and counters each step.

The depth of a search is set by injecting maps explored within L1 distance D
of each robot: the nearest unexplored cell is then D steps away (or farther,
behind obstacles), the BFS runs D layers deep, and the window kernel lists
every item with D > 24 for the full-map kernel.  On these maps the geodesic
distance is the L1 distance give or take a cell; that "farther" -- targets a
few cells away behind a wall, corridors that wind for thousands of layers,
tied ends and tied walks back -- is what test_gpu_dijkstra_mazes.py tests, on
the authored mazes of dijkstra_maze_cases.py.
"""
import os

import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from golden_util import GOLDEN_DIR
from oracle.cpu_ref import DecGridRLRef
from test_gpu_parity import base_cfg, bern, full_obs
from test_gpu_shapes import run_against_oracle

pytestmark = pytest.mark.gpu

MAPS = os.path.join(GOLDEN_DIR, "maps")
DJ_ENV = ("MARLCOV_DJ_BIG", "MARLCOV_DJ_FULL", "MARLCOV_DJ_BIG_GRID", "MARLCOV_DJ_FULL_GRID", "MARLCOV_DJ_DEPTH")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def big_map():
    """bg2_1073x1073/AR0011SR.png as the reference's gridload makes it:
    float64, 0 -> -1, 255 -> 1 (gridmaker.py:89-91)."""
    import marlcov
    _, test = marlcov.gridload({"grid_dir": MAPS, "numgrids": 1000}, sort=True)
    grids = [g for g in test if g.shape == (1073, 1073)]
    assert len(grids) == 1
    return grids[0]


def set_dj_env(monkeypatch, **kw):
    """Only the given MARLCOV_DJ_* variables (read at mc_create)."""
    for k in DJ_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("MARLCOV_DJ_" + k, str(v))


def inject_diamonds(torch, env, depth_of):
    """Every agent's maps become "explored within L1 distance D of the
    robot", D = depth_of(b, i): free / obstacle maps, the visited union and
    the two counters, as the env itself would have left them."""
    from marlcov import _lib
    from marlcov.tiles import cells_to_tiles
    B, N, W, L = env.num_envs, env.num_agents, env.width, env.length
    pos = env.get_state(_lib.FIELD_POS).cpu().numpy()
    eg = env.get_state(_lib.FIELD_ENV_GRID).cpu().numpy()
    st = device_state(env, envs=[int(np.flatnonzero(eg == g)[0]) for g in sorted(set(eg.tolist()))])
    X, Y = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(L, dtype=np.int32), indexing="ij")
    free = np.zeros((B, N, W, L), np.uint8)
    obst = np.zeros((B, N, W, L), np.uint8)
    for b in range(B):
        neg = st["neg"][int(eg[b])][:W, :L]
        for i in range(N):
            x, y = pos[b, i]
            near = (np.abs(X - x) + np.abs(Y - y)) < depth_of(b, i)
            free[b, i] = near & (neg == 0)
            obst[b, i] = near & (neg == 1)
    vis = free.max(axis=1)

    def put(field, a):
        env.set_state(field, torch.from_numpy(np.ascontiguousarray(a)))

    put(_lib.FIELD_FREE, cells_to_tiles(free, blocks=True).view(np.int64))
    put(_lib.FIELD_OBST, cells_to_tiles(obst, blocks=True).view(np.int64))
    put(_lib.FIELD_VISITED, cells_to_tiles(vis, blocks=True).view(np.int64))
    put(_lib.FIELD_FREE_COUNT, free.reshape(B, -1).sum(1).astype(np.int32))
    put(_lib.FIELD_VISITED_COUNT, vis.reshape(B, -1).sum(1).astype(np.int32))


def step_against_oracle(torch, env, cfg, rs, T, envs, label):
    """T random steps; the envs in ``envs`` against oracle envs rebuilt from
    the device state: obs, reward, done and compare_env every step.  Returns
    the largest MC_FIELD_DJ_LISTED seen."""
    from marlcov import _lib
    B, N = env.num_envs, env.num_agents
    st = device_state(env, envs)
    refs = {b: oracle_from_device(st, b, cfg) for b in envs}
    listed = 0
    for t in range(T):
        acts = rs.randint(0, 4, size=(B, N)).astype(np.uint8)
        obs, rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs_h, rew_h, done_h = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
        listed = max(listed, int(env.get_state(_lib.FIELD_DJ_LISTED).item()))
        st = device_state(env, envs)
        for b in envs:
            o, r, d = refs[b].step(ref_action(acts[b]))
            tag = f"{label} t={t} env {b}"
            assert float(r) == rew_h[b], (tag, float(r), rew_h[b])
            assert bool(d) == bool(done_h[b]), tag
            np.testing.assert_array_equal(obs_h[b], o, err_msg=tag + " obs")
            compare_env(st, b, refs[b], tag)
    env.check()
    return listed


FAR_DEPTHS = [1, 6, 22, 23, 24, 25, 26, 31, 45, 80, 300]


def far_targets(torch, monkeypatch, label, **dj):
    """The configuration of test_gpu_parity.test_dijkstra_far_targets."""
    import marlcov
    set_dj_env(monkeypatch, **dj)
    cfg = base_cfg(numrobot=3, dijkstra_input=1, sensor_config={"num_lasers": 9, "range": 3})
    rs = np.random.RandomState(11)
    B = 10
    grids = [bern(rs, 110, 96, 0.08) for _ in range(B)]
    env = marlcov.BatchCoverageEnv(cfg, B, grids=grids, auto_reset=False)
    env.reset()
    inject_diamonds(torch, env, lambda b, i: FAR_DEPTHS[(b + 4 * i) % len(FAR_DEPTHS)])
    return env, step_against_oracle(torch, env, cfg, rs, 4, list(range(B)), label)


@pytest.mark.parametrize("full", [False, True], ids=["window", "full_map"])
def test_forced_hbm_far_targets(torch_cuda, monkeypatch, full):
    """The HBM kernel forced onto a 110x96 map, nearest unexplored cell 1..300
    steps away: as the full-map kernel behind the window kernel, and
    (MARLCOV_DJ_FULL=1) on every item."""
    dj = {"BIG": 1, "FULL": 1} if full else {"BIG": 1}
    env, listed = far_targets(torch_cuda, monkeypatch, "hbm far", **dj)
    assert env.dijkstra_variant() == ("hbm" if full else "window+hbm")
    if not full:
        assert listed > 0  # some paths were farther than the window holds


def test_forced_hbm_slot_reuse(torch_cuda, monkeypatch):
    """Thirty items over two scratch slots and four steps, deep searches (80,
    300) followed by shallow ones (1, 6) on the same slot: a plane word left
    by an earlier item or step must never be read."""
    env, _ = far_targets(torch_cuda, monkeypatch, "hbm slots", BIG=1, FULL=1, BIG_GRID=2)
    assert env.dijkstra_variant() == "hbm"


EDGE_DEPTHS = [1, 24, 25, 40, 70, 1000]  # 1000: past the map's diameter (fully explored)
# (unpadded grid, extended columns RY = length + 2 + 2 * egoradius, words per row, reset seed)
EDGE_SHAPES = {
    "ry_multiple_of_64": ((20, 186), 192, 3, 1),
    "partial_last_word": ((20, 190), 196, 4, 1),
    "one_word_rows_clipped": ((200, 10), 16, 1, 1),
}


@pytest.mark.parametrize("name", sorted(EDGE_SHAPES))
def test_forced_hbm_plane_edges(torch_cuda, monkeypatch, name):
    """Plane geometry: RY an exact multiple of 64, a partial last word, one
    word per row with the band clipped by the rows; robots within 2 cells of
    the map border (padded coordinates, whose index 0 and last index are the
    wall ring: the robot stands one or two free cells from the wall); one
    fully explored map per case (empty path, or the pad ring)."""
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    (w, l), ry, rw, seed = EDGE_SHAPES[name]
    set_dj_env(monkeypatch, BIG=1, FULL=1)
    cfg = base_cfg(numrobot=2, dijkstra_input=1, egoradius=2, sensor_config={"num_lasers": 9, "range": 3})
    rs = np.random.RandomState(l)
    B, N = 4, 2
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, w, l, 0.08) for _ in range(B)], auto_reset=False,
                                   seed=seed)
    assert env.dijkstra_variant() == "hbm"
    assert env.length + 2 * cfg["egoradius"] == ry and (ry + 63) // 64 == rw
    if name == "ry_multiple_of_64":
        assert ry % 64 == 0
    env.reset()
    pos = env.get_state(_lib.FIELD_POS).cpu().numpy()
    edge = np.minimum(np.minimum(pos[..., 0], env.width - 1 - pos[..., 0]),
                      np.minimum(pos[..., 1], env.length - 1 - pos[..., 1]))
    assert (edge <= 2).any(), "no robot within 2 cells of the border: pick another seed"
    diam = env.width + env.length
    depths = [d for d in EDGE_DEPTHS if d == 1000 or d < diam]
    assert depths[-1] == 1000 and depths[-1] > diam
    inject_diamonds(torch, env, lambda b, i: depths[(b * N + i) % len(depths)])
    step_against_oracle(torch, env, cfg, rs, 3, list(range(B)), name)


LARGE_DEPTHS = [1, 24, 25, 80, 120, 300]


def test_large_grid_runs_and_matches_oracle(torch_cuda, monkeypatch):
    """A 448x384 grid (about 178 KB of planes: more than one workgroup's LDS)
    with no environment variable set: mc_create selects the HBM kernel behind
    the window kernel instead of rejecting the env.

    Without the HBM kernel this test fails in the constructor with
    MarlcovError ("dijkstra_input: ... B of LDS bitboards ... exceed")."""
    import marlcov
    torch = torch_cuda
    set_dj_env(monkeypatch)
    cfg = base_cfg(numrobot=3, dijkstra_input=1, sensor_config={"num_lasers": 9, "range": 3})
    rs = np.random.RandomState(448)
    B, N = 2, 3
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, 448, 384, 0.08) for _ in range(B)], auto_reset=False)
    assert env.dijkstra_variant() == "window+hbm"
    env.reset()
    inject_diamonds(torch, env, lambda b, i: LARGE_DEPTHS[b * N + i])
    listed = step_against_oracle(torch, env, cfg, rs, 2, list(range(B)), "448x384")
    assert listed > 0


BG2_SEED = 4  # reset seed of the bg2 test: few envs with a robot at row / column >= 1000, at least one


@pytest.mark.parametrize("full", [False, True], ids=["window", "full_map"])
def test_bg2_1073_dijkstra(torch_cuda, monkeypatch, full):
    """dijkstra_input on the reference's 1073x1073 map (about 1 MB of planes
    per item), 16 envs x 4 agents at the C2 sensor: the envs with a robot at
    row or column >= 1000 (the far end of the planes) and one other env
    against the oracle, searches 30 and 120 layers deep."""
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    set_dj_env(monkeypatch, **({"FULL": 1} if full else {}))
    cfg = base_cfg(numrobot=4, dijkstra_input=1)
    B, N = 16, 4
    g = big_map()
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[g], auto_reset=False, seed=BG2_SEED)
    assert env.dijkstra_variant() == ("hbm" if full else "window+hbm")
    env.reset()
    pos = env.get_state(_lib.FIELD_POS).cpu().numpy()
    far = np.flatnonzero((pos >= 1000).any(axis=(1, 2)))
    assert far.size > 0, "no robot at row or column >= 1000: pick another seed"
    other = [b for b in range(B) if b not in set(far.tolist())][:1]
    envs = sorted(far.tolist() + other)
    inject_diamonds(torch, env, lambda b, i: [30, 120][(b + i) % 2])
    listed = step_against_oracle(torch, env, cfg, np.random.RandomState(1073), 2, envs, "bg2 dj")
    if not full:
        assert listed > 0
        # plain steps from a fresh reset: the nearest unexplored cell is close,
        # the list stays empty and the HBM kernel runs over zero items
        env.reset()
        run_against_oracle(torch, env, cfg, np.random.RandomState(7), 6, envs[:2], BG2_SEED, "bg2 dj plain",
                           sentinel_p=0.0)
        assert int(env.get_state(_lib.FIELD_DJ_LISTED).item()) == 0


def test_facade_large_grid(torch_cuda, monkeypatch):
    """marlcov.DecGridRL with dijkstra_input on one 448x384 grid: constructs
    (no size limit) and equals the oracle's DecGridRLRef through a reset and
    3 steps under the same NumPy seed."""
    import marlcov
    set_dj_env(monkeypatch)
    cfg = base_cfg(numrobot=2, dijkstra_input=1, sensor_config={"num_lasers": 9, "range": 4})
    rs = np.random.RandomState(6)
    train = [bern(rs, 448, 384, 0.08)]
    np.random.seed(3)
    env = marlcov.DecGridRL(train, cfg)
    np.random.seed(3)
    ref = DecGridRLRef(train, cfg)
    np.random.seed(21)
    o, g = env.reset(False, None)
    np.random.seed(21)
    ro, rg = ref.reset(False, None)
    np.testing.assert_array_equal(g, rg)
    assert np.shape(o) == np.shape(ro)
    np.testing.assert_array_equal(o, ro)
    for t in range(3):
        a = int(rs.randint(0, 16))
        o, r, d = env.step(a)
        ro, rr, rd = ref.step(a)
        assert float(r) == float(rr) and bool(d) == bool(rd), t
        assert np.shape(o) == np.shape(ro)
        np.testing.assert_array_equal(o, ro, err_msg=f"t {t}")


def test_dijkstra_variant_small_map(torch_cuda, monkeypatch):
    """Nothing changes for maps that fit LDS: a 40x40 env reports the LDS
    kernels, and no dijkstra kernels without the layer."""
    import marlcov
    g = [np.ones((40, 40))]
    set_dj_env(monkeypatch)
    assert marlcov.BatchCoverageEnv(base_cfg(dijkstra_input=1), 2, grids=g).dijkstra_variant() == "window+lds"
    assert marlcov.BatchCoverageEnv(base_cfg(), 2, grids=g).dijkstra_variant() == ""
    set_dj_env(monkeypatch, FULL=1)
    assert marlcov.BatchCoverageEnv(base_cfg(dijkstra_input=1), 2, grids=g).dijkstra_variant() == "lds"

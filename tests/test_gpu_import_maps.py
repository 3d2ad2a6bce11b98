"""GPU: mc_import_maps (csrc/mc_import.hip) -- ``BatchCoverageEnv.set_global_state``:
dense uint8 planes (robots, free0.., obst0..) set the tiled maps, the union
map, the two counters and the positions of chosen envs on the device.

References, all independent of the import: planes authored on the host and
numpy counts of them; ``get_state`` tiles decoded with
``marlcov.tiles.tiles_to_cells``; the CPU oracle filled from the authored
arrays and stepped beside the env (``gpu_util.compare_env``); a twin env.
Every comparison is bit for bit.

Shapes as in test_gpu_export_maps.py: unpadded 35 x 43 pads to 37 x 45 (2 x 2
tile blocks, planes of 1,665 bytes: every plane and slot starts at another
alignment, edge tiles partly outside the grid), unpadded 32 x 46 pads to 34 x
48.  6 envs, 3 agents, two grids (env e on grid e % 2), square sensor of
radius 2."""
import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_export_maps import B, N, SEED, SHAPES, make_small, run_steps, small_cfg, small_grids
from test_gpu_parity import full_obs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def per_env_fields():
    from marlcov import _lib
    return {"POS": _lib.FIELD_POS, "MOVED": _lib.FIELD_MOVED, "FREE": _lib.FIELD_FREE, "OBST": _lib.FIELD_OBST,
            "VISITED": _lib.FIELD_VISITED, "FREE_COUNT": _lib.FIELD_FREE_COUNT,
            "VISITED_COUNT": _lib.FIELD_VISITED_COUNT, "CURRSTEP": _lib.FIELD_CURRSTEP,
            "DONE_THRESH": _lib.FIELD_DONE_THRESH, "ENV_GRID": _lib.FIELD_ENV_GRID, "EPISODE": _lib.FIELD_EPISODE}


def fields(env):
    """host copies of every per-env state field, by name"""
    return {name: env.get_state(f).cpu().numpy().copy() for name, f in per_env_fields().items()}


def assert_fields_equal(got, want, envs, tag, skip=()):
    for name in want:
        if name not in skip:
            np.testing.assert_array_equal(got[name][list(envs)], want[name][list(envs)], err_msg=f"{tag} {name}")


def padded_grids(shape):
    """the padded grids of make_small's pool (a ring of -1 around each)"""
    return [np.pad(g, 1, constant_values=-1.0) for g in small_grids(shape)]


def author(shape, rs, envs):
    """Planes made on the host for the envs `envs` of a make_small env: per
    agent a random half of the cells with grid >= 0 free, a random half of
    the cells with grid < 0 obstacles (bytes 1 and 255), robots on distinct
    cells with grid > 0.  Returns (robots [K, W, L], free [K, N, W, L], obst
    [K, N, W, L], pos [K, N, 2]), uint8 / int."""
    gp = padded_grids(shape)
    W, L = gp[0].shape
    K = len(envs)
    robots = np.zeros((K, W, L), dtype=np.uint8)
    free = np.zeros((K, N, W, L), dtype=np.uint8)
    obst = np.zeros((K, N, W, L), dtype=np.uint8)
    pos = np.zeros((K, N, 2), dtype=np.int64)
    for k, e in enumerate(envs):
        g = gp[e % 2]
        for a in range(N):
            free[k, a] = (g >= 0) & (rs.rand(W, L) < 0.5)
            obst[k, a] = ((g < 0) & (rs.rand(W, L) < 0.5)) * rs.choice([1, 255], size=(W, L))
        cells = np.argwhere(g > 0)
        pos[k] = cells[rs.choice(len(cells), size=N, replace=False)]
        for a in range(N):
            robots[k, pos[k, a, 0], pos[k, a, 1]] = a + 1
    return robots, free, obst, pos


def stack_planes(robots, free, obst):
    return np.concatenate([robots[:, None], free, obst], axis=1)


def authored_state(env, envs, free, obst, pos):
    """gpu_util.device_state of `env` with the maps and positions of `envs`
    replaced by the authored arrays: what oracle_from_device fills an oracle
    from (the grid pool, MOVED, CURRSTEP and DONE_THRESH are the env's own)."""
    st = device_state(env)
    for k, e in enumerate(envs):
        st["pos"][e] = pos[k]
        st["free"][e] = free[k] != 0
        st["obst"][e] = obst[k] != 0
        st["vis"][e] = (free[k] != 0).any(axis=0)
    return st


def step_beside_oracle(env, refs, cfg, steps, first, tag, dist_layer=False):
    """`steps` random_actions steps of env and oracles: obs, reward, done and
    (compare_env) the state of every env at every step"""
    for t in range(first, first + steps):
        acts = env.random_actions(SEED, t)
        obs, rew, done = env.step(acts)
        acts = acts.cpu().numpy()
        obs, rew, done = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
        st = device_state(env)
        for b, ref in refs.items():
            o, r, d = ref.step(ref_action(acts[b]))
            tg = f"{tag} t={t} env {b}"
            assert float(r) == rew[b], (tg, float(r), rew[b])
            assert bool(d) == bool(done[b]), tg
            np.testing.assert_array_equal(obs[b], o, err_msg=tg + " obs")
            if dist_layer:
                assert np.asarray(o)[:, 3].any(), tg + ": the oracle's dist layer is empty"
            compare_env(st, b, ref, tg)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_authored_planes_against_the_oracle(torch_cuda, shape):
    from marlcov import _lib
    from marlcov.tiles import tiles_to_cells
    env = make_small(SHAPES[shape])
    W, L = env.width, env.length
    rs = np.random.RandomState(SEED + 1)
    envs = list(range(B))
    robots, free, obst, pos = author(SHAPES[shape], rs, envs)
    planes = stack_planes(robots, free, obst)
    # non-vacuity: every plane has zero and nonzero cells; the union differs from each agent's map
    assert all(planes[k, p].any() and not planes[k, p].all() for k in range(B) for p in range(1 + 2 * N))
    union = (free != 0).any(axis=1)
    assert all(not np.array_equal(union[k], free[k, a] != 0) for k in range(B) for a in range(N))
    assert set(np.unique(obst).tolist()) == {0, 1, 255}
    before = fields(env)
    env.set_global_state(planes)  # a host array, all envs in order
    env.check()
    got = fields(env)

    def cells(name):
        return tiles_to_cells(got[name], W, L)

    np.testing.assert_array_equal(cells("FREE"), free != 0)
    np.testing.assert_array_equal(cells("OBST"), obst != 0)
    np.testing.assert_array_equal(cells("VISITED"), union)
    np.testing.assert_array_equal(got["POS"], pos)
    np.testing.assert_array_equal(got["FREE_COUNT"], np.count_nonzero(free, axis=(1, 2, 3)))
    np.testing.assert_array_equal(got["VISITED_COUNT"], np.count_nonzero(union, axis=(1, 2)))
    assert_fields_equal(got, before, envs, "untouched", skip=("POS", "FREE", "OBST", "VISITED", "FREE_COUNT",
                                                              "VISITED_COUNT"))
    # the tiles hold nothing beyond the grid (edge tiles, padding tiles of the last blocks)
    full = tiles_to_cells(got["FREE"], 32 * got["FREE"].shape[-4], 32 * got["FREE"].shape[-3])
    assert full[..., :W, :L].sum() == full.sum()
    # the oracle, filled from the authored arrays, steps beside the env
    cfg = small_cfg()
    st = authored_state(env, envs, free, obst, pos)
    refs = {b: oracle_from_device(st, b, cfg) for b in envs}
    step_beside_oracle(env, refs, cfg, 8, 0, shape)
    env.check()
    env.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_round_trip_through_a_sibling(torch_cuda, shape):
    from marlcov import _lib
    a = make_small(SHAPES[shape])
    run_steps(a, 12)
    sib = a.sibling(B)
    planes = a.global_state(_lib.MAP_IMPORTABLE)
    assert planes[:, 1:].any() and planes[:, 0].max() == N
    sib.set_global_state(planes, _lib.MAP_IMPORTABLE)
    for f in (_lib.FIELD_MOVED, _lib.FIELD_CURRSTEP, _lib.FIELD_DONE_THRESH):
        sib.set_state(f, a.get_state(f))
    sib.check()
    assert_fields_equal(fields(sib), fields(a), range(B), "round trip")
    # the import of an env's own export is the identity on its state
    a.set_global_state(a.global_state(("free", "robots"), envs=[3, 0]), ("free", "robots"), envs=[3, 0])
    assert_fields_equal(fields(a), fields(sib), range(B), "identity")
    ra, rb = run_steps(a, 8, first=12), run_steps(sib, 8, first=12)
    for t, (x, y) in enumerate(zip(ra, rb)):
        for u, v, what in zip(x, y, ("obs", "reward", "done")):
            np.testing.assert_array_equal(u, v, err_msg=f"step {12 + t} {what}")
    assert_fields_equal(fields(sib), fields(a), range(B), "after 8 steps")
    a.check(), sib.check()
    a.close(), sib.close()


def test_map_narrower_than_a_tile(torch_cuda):
    """unpadded 20 x 3 pads to 22 x 5: rows of 5 bytes, one column of tiles (the
    kernel's instantiation that reads runs of Lp bytes)"""
    import marlcov
    from marlcov import _lib
    from marlcov.tiles import tiles_to_cells
    cfg = small_cfg(numrobot=2, egoradius=1, sensor_config={"range": 1})
    a = marlcov.BatchCoverageEnv(cfg, 3, grids=[np.ones((20, 3))], seed=SEED, auto_reset=False)
    a.reset()
    for t in range(9):
        a.step(a.random_actions(SEED, t))
    sib = a.sibling(3)
    planes = a.global_state(_lib.MAP_IMPORTABLE)
    assert tuple(planes.shape) == (3, 5, 22, 5)
    sib.set_global_state(planes, _lib.MAP_IMPORTABLE)
    for f in (_lib.FIELD_MOVED, _lib.FIELD_CURRSTEP, _lib.FIELD_DONE_THRESH):
        sib.set_state(f, a.get_state(f))
    sib.check()
    assert_fields_equal(fields(sib), fields(a), range(3), "narrow round trip")
    # and against the planes themselves, on the host
    got = fields(sib)
    host = planes.cpu().numpy()
    np.testing.assert_array_equal(tiles_to_cells(got["FREE"], 22, 5), host[:, 1:3] != 0)
    np.testing.assert_array_equal(tiles_to_cells(got["OBST"], 22, 5), host[:, 3:5] != 0)
    assert host[:, 1:3].any() and host[:, 3:5].any() and not host[:, 1:3].all()
    a.close(), sib.close()


def test_subset_and_order(torch_cuda):
    from marlcov import _lib
    torch = torch_cuda
    src, dst = make_small(SHAPES["37x45"]), make_small(SHAPES["37x45"])
    run_steps(src, 12)
    run_steps(dst, 5, first=40)
    want, before = fields(src), fields(dst)
    maps = ("POS", "FREE", "OBST", "VISITED", "FREE_COUNT", "VISITED_COUNT")
    assert all(not np.array_equal(want[n][[4, 1]], before[n][[4, 1]]) for n in maps)
    planes = src.global_state(_lib.MAP_IMPORTABLE, envs=[4, 1])
    dst.set_global_state(planes, _lib.MAP_IMPORTABLE, envs=[4, 1])
    dst.check()
    got = fields(dst)
    assert_fields_equal(got, before, [0, 2, 3, 5], "other envs")
    for name in maps:
        np.testing.assert_array_equal(got[name][[4, 1]], want[name][[4, 1]], err_msg=name)
    assert_fields_equal(got, before, [4, 1], "kept", skip=maps)
    # the same from a device index, the slots the other way round
    again = make_small(SHAPES["37x45"])
    run_steps(again, 5, first=40)
    again.set_global_state(planes.flip(0), ("robots", "free", "obst"), envs=torch.tensor([1, 4], device=again.device))
    again.check()
    assert_fields_equal(fields(again), got, range(B), "device index")
    # ROBOTS alone moves only POS
    mid = fields(dst)
    dst.set_global_state(src.global_state("robots", envs=[2]), "robots", envs=[2])
    dst.check()
    got = fields(dst)
    np.testing.assert_array_equal(got["POS"][2], want["POS"][2])
    assert not np.array_equal(mid["POS"][2], want["POS"][2])
    assert_fields_equal(got, mid, range(B), "robots alone", skip=("POS",))
    assert_fields_equal(got, mid, [0, 1, 3, 4, 5], "robots alone POS")
    # FREE alone rewrites FREE, VISITED and the counts, and leaves OBST and POS
    mid = got
    dst.set_global_state(src.global_state("free", envs=[3]), "free", envs=[3])
    dst.check()
    got = fields(dst)
    derived = ("FREE", "VISITED", "FREE_COUNT", "VISITED_COUNT")
    for name in derived:
        np.testing.assert_array_equal(got[name][3], want[name][3], err_msg=name)
        assert not np.array_equal(mid[name][3], want[name][3]), name
    assert_fields_equal(got, mid, range(B), "free alone", skip=derived)
    assert_fields_equal(got, mid, [0, 1, 2, 4, 5], "free alone, other envs")
    for e in (src, dst, again):
        e.close()


def test_bad_slots_leave_their_envs_and_are_reported(torch_cuda):
    from marlcov import _lib
    torch = torch_cuda
    shape = SHAPES["37x45"]
    env = make_small(shape)
    run_steps(env, 4)
    before = fields(env)
    rs = np.random.RandomState(SEED + 2)
    slots = [0, B, 1, 2, 3, 4, 5]  # slot 1: an index out of range
    robots, free, obst, pos = author(shape, rs, [e % B for e in slots])
    robots[2][robots[2] == 2] = 0  # env 1: robot 2 is missing
    robots[3][tuple(np.argwhere((padded_grids(shape)[0] > 0) & (robots[3] == 0))[0])] = 1  # env 2: robot 1 twice
    robots[4][robots[4] == 3] = N + 1  # env 3: a number above N
    robots[5][robots[5] == 1] = 0  # env 4: robot 1 on an obstacle of the grid
    blocked = np.argwhere(padded_grids(shape)[0][1:-1, 1:-1] < 0)[0] + 1
    robots[5][tuple(blocked)] = 1
    idx = torch.tensor(slots, dtype=torch.int32, device=env.device)
    env.set_global_state(stack_planes(robots, free, obst), envs=idx)
    with pytest.raises(_lib.MarlcovError, match=r"0x80.*128=import_maps.*bit 128"):
        env.check()
    env.check()  # reported once, then clean
    got = fields(env)
    assert_fields_equal(got, before, [1, 2, 3, 4], "bad slots")
    for k, e in ((0, 0), (6, 5)):
        np.testing.assert_array_equal(got["POS"][e], pos[k])
        np.testing.assert_array_equal(got["FREE_COUNT"][e], np.count_nonzero(free[k]))
        assert not np.array_equal(got["FREE"][e], before["FREE"][e])
    env.step(env.random_actions(SEED, 4))
    env.check()
    env.close()


def test_argument_errors_name_the_argument(torch_cuda):
    from marlcov import _lib
    torch = torch_cuda
    env = make_small(SHAPES["34x48"])
    W, L = env.width, env.length
    free = torch.zeros((B, N, W, L), dtype=torch.uint8, device=env.device)
    with pytest.raises(_lib.MarlcovError, match=r"layers 0x24 has bit 4 \(MC_MAP_VISITED\)"):
        env.set_global_state(free, _lib.MAP_FREE | _lib.MAP_VISITED)
    with pytest.raises(_lib.MarlcovError, match=r"layers 0x21 has bit 1 \(MC_MAP_GRID_NEG\)"):
        env.set_global_state(free, ("free", "grid_neg"))
    with pytest.raises(_lib.MarlcovError, match="layers 0x0"):
        env.set_global_state(free, 0)
    with pytest.raises(ValueError, match="planes must have shape"):
        env.set_global_state(free[:, :2], "free")
    with pytest.raises(_lib.MarlcovError, match=r"in_bytes"):
        _lib.check(env.lib.mc_import_maps(env._h, _lib.MAP_FREE, None, B, free.data_ptr(), free.numel() - 1,
                                          env._stream()), "mc_import_maps")
    with pytest.raises(_lib.MarlcovError, match=r"count 5 with dev_envs NULL"):
        _lib.check(env.lib.mc_import_maps(env._h, _lib.MAP_FREE, None, B - 1, free.data_ptr(),
                                          (B - 1) * N * W * L, env._stream()), "mc_import_maps")
    with pytest.raises(_lib.MarlcovError, match=r"null dev_in"):
        _lib.check(env.lib.mc_import_maps(env._h, _lib.MAP_FREE, None, B, None, free.numel(), env._stream()),
                   "mc_import_maps")
    with pytest.raises(ValueError, match="envs names an env twice"):
        env.set_global_state(free[:3], "free", envs=[2, 0, 2])
    before = fields(env)
    env.set_global_state(free[:0], "free", envs=[])  # a no-op
    assert_fields_equal(fields(env), before, range(B), "after the refused calls")
    env.step(env.random_actions(SEED, 0))
    env.check()
    env.close()


def test_dist_reward_caches_of_imported_envs(torch_cuda):
    import marlcov
    from marlcov import _lib
    shape = SHAPES["37x45"]
    cfg = small_cfg(dist_reward=1)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=small_grids(shape), seed=SEED, auto_reset=False,
                                   env_grid=[e % 2 for e in range(B)])
    env.reset()
    for t in range(6):
        env.step(env.random_actions(SEED, t))
    assert (env.get_state(_lib.FIELD_DIST_MW)[..., 0] >= 0).all()  # known maxima
    # larger maps: the envs' own free cells and a random fifth of the other cells with grid >= 0
    sel = [1, 4]
    own = env.global_state(_lib.MAP_IMPORTABLE, envs=sel).cpu().numpy()
    rs = np.random.RandomState(SEED + 3)
    gp = padded_grids(shape)
    free, obst = own[:, 1:1 + N].copy(), own[:, 1 + N:]
    for k, e in enumerate(sel):
        for a in range(N):
            free[k, a] |= ((gp[e % 2] >= 0) & (rs.rand(*gp[0].shape) < 0.2)).astype(np.uint8)
        assert free[k].sum() > own[k, 1:1 + N].sum()
    pos = env.get_state(_lib.FIELD_POS).cpu().numpy()[sel]
    env.set_global_state(free, "free", envs=sel)
    env.check()
    mw = env.get_state(_lib.FIELD_DIST_MW).cpu().numpy()[..., 0]
    assert (mw[sel] == -1).all() and (mw[[0, 2, 3, 5]] >= 0).all()
    st = authored_state(env, sel, free, obst, pos)
    refs = {b: oracle_from_device(st, b, cfg) for b in range(B)}
    step_beside_oracle(env, refs, cfg, 4, 6, "dist", dist_layer=True)
    env.check()
    env.close()


def test_c2_shape_once(torch_cuda):
    """64 envs, 4 agents, 128 x 128, lidar of 21 beams and range 10 (the step
    reads the visibility table): planes of 130 x 130 bytes, 17 x 17 tiles in
    5 x 5 blocks, a workgroup of five waves"""
    import marlcov
    from marlcov import _lib
    cfg = small_cfg(numrobot=4, sensor_type="lidar", sensor_config={"num_lasers": 21, "range": 10})
    twin = marlcov.BatchCoverageEnv(cfg, 64, gen=dict(width=128, length=128, prob_obst=0.1, seed=7, num_grids=64),
                                    seed=11, auto_reset=False)
    twin.reset()
    run_steps(twin, 6)
    sib = twin.sibling(64)
    sel = [0, 21, 42, 63]
    planes = twin.global_state(_lib.MAP_IMPORTABLE, envs=sel)
    assert tuple(planes.shape) == (4, 9, 130, 130) and all(planes[:, p].any() for p in range(9))
    sib.set_global_state(planes, _lib.MAP_IMPORTABLE, envs=sel)
    for f in (_lib.FIELD_MOVED, _lib.FIELD_CURRSTEP, _lib.FIELD_DONE_THRESH):
        sib.set_state(f, twin.get_state(f))
    sib.check()
    assert_fields_equal(fields(sib), fields(twin), sel, "c2 round trip")
    launches = sib.env_launches()
    ra, rb = run_steps(twin, 6, first=6), run_steps(sib, 6, first=6)
    for t, (x, y) in enumerate(zip(ra, rb)):
        for u, v, what in zip(x, y, ("obs", "reward", "done")):
            np.testing.assert_array_equal(u[sel], v[sel], err_msg=f"step {6 + t} {what}")
    assert sib.env_launches() == launches + 6
    assert_fields_equal(fields(sib), fields(twin), sel, "c2 after 6 steps")
    twin.check(), sib.check()
    twin.close(), sib.close()

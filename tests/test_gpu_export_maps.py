"""GPU: mc_export_maps (csrc/mc_export.hip) -- ``BatchCoverageEnv.global_state``:
the tiled env state as dense uint8 planes (scale 1) or one count per 8x8 tile
(scale 8), decoded on the device.

The reference of every comparison is independent of the export: the
``get_state`` tiles copied to the host and decoded with
``marlcov.tiles.tiles_to_cells``, plus FIELD_POS and FIELD_ENV_GRID.  Every
comparison is bit for bit.

Shapes.  Unpadded 35 x 43 pads to 37 x 45: 2 x 2 blocks of tiles (the block
order matters both ways), planes of 1,665 bytes (odd: every plane and slot
starts at another alignment) and edge tiles partly outside the grid.  Unpadded
32 x 46 pads to 34 x 48: rows are 16-byte multiples.  6 envs, 3 agents, two
grids (env e on grid e % 2), square sensor of radius 2, 12 random steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N, SEED, STEPS = 6, 3, 2024, 12
SHAPES = {"37x45": (35, 43), "34x48": (32, 46)}
ORDER = ("grid_neg", "grid_pos", "visited", "obst_any", "robots", "free", "obst")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def small_cfg(**kw):
    c = dict(numrobot=N, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0, terminal_reward=30,
             dist_reward=0, train_maxsteps=1000, test_maxsteps=1000, egoradius=2, mini_map_rad=0, comm_radius=0,
             allow_comm=0, map_sharing=0, single_square_tool=0, dijkstra_input=0, sensor_type="square_sensor",
             sensor_config={"range": 2})
    c.update(kw)
    return c


def small_grids(shape):
    rs = np.random.RandomState(SEED)
    return [rs.choice([1.0, -1.0], size=shape, p=[0.9, 0.1]) for _ in range(2)]


def make_small(shape):
    import marlcov
    env = marlcov.BatchCoverageEnv(small_cfg(), B, grids=small_grids(shape), seed=SEED, auto_reset=False,
                                   env_grid=[e % 2 for e in range(B)])
    env.reset()
    return env


def run_steps(env, steps, first=0, between=None):
    """`steps` random_actions steps; returns the host copies of every step's outputs"""
    out = []
    for t in range(first, first + steps):
        obs, rew, done = env.step(env.random_actions(SEED, t))
        out.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy()))
        if between is not None:
            between()
    return out


def host_planes(env, envs=None):
    """The host decode: {layer: uint8 [len(envs), planes, width, length]} of the
    envs (None: all) from the get_state tiles, FIELD_POS and FIELD_ENV_GRID."""
    from marlcov import _lib
    from marlcov.tiles import tiles_to_cells
    W, L = env.width, env.length
    envs = list(range(env.num_envs)) if envs is None else list(envs)

    def cells(field, index):
        return tiles_to_cells(env.get_state(field)[index].cpu().numpy(), W, L).astype(np.uint8)

    eg = env.get_state(_lib.FIELD_ENV_GRID).cpu().numpy()[envs]
    pos = env.get_state(_lib.FIELD_POS).cpu().numpy()[envs]
    free, obst = cells(_lib.FIELD_FREE, envs), cells(_lib.FIELD_OBST, envs)
    robots = np.zeros((len(envs), 1, W, L), dtype=np.uint8)
    for k in range(len(envs)):
        for i in range(env.num_agents):
            robots[k, 0, pos[k, i, 0], pos[k, i, 1]] = i + 1
    return {
        "grid_neg": cells(_lib.FIELD_GRID_NEG, eg.tolist())[:, None],
        "grid_pos": cells(_lib.FIELD_GRID_POS, eg.tolist())[:, None],
        "visited": cells(_lib.FIELD_VISITED, envs)[:, None],
        "obst_any": obst.max(axis=1, keepdims=True),
        "robots": robots,
        "free": free,
        "obst": obst,
    }


def stack(ref, layers, rows=None):
    """the reference planes of `layers` in output order, for the slots `rows`"""
    d = np.concatenate([ref[n] for n in ORDER if n in layers], axis=1)
    return d if rows is None else d[list(rows)]


def pool8(dense, robots_plane=None):
    """block sums over 8 x 8 tiles of [..., W, L], zero-padded past the grid
    (the robots plane counts robots, not their numbers)"""
    d = dense.astype(np.int64)
    if robots_plane is not None:
        d[:, robots_plane] = d[:, robots_plane] != 0
    W, L = d.shape[-2:]
    tr, tc = -(-W // 8), -(-L // 8)
    full = np.zeros(d.shape[:-2] + (8 * tr, 8 * tc), dtype=np.int64)
    full[..., :W, :L] = d
    return full.reshape(d.shape[:-2] + (tr, 8, tc, 8)).sum(axis=(-3, -1)).astype(np.uint8)


@pytest.fixture(scope="module", params=sorted(SHAPES))
def small(request, torch_cuda):
    """(env after 12 steps, its host decode); neither is changed by a test"""
    env = make_small(SHAPES[request.param])
    run_steps(env, STEPS)
    env.check()
    ref = host_planes(env)
    for a in ref.values():
        a.setflags(write=False)
    yield env, ref
    env.close()


def test_dense_all_layers_all_envs(small):
    from marlcov import _lib
    env, ref = small
    W, L = env.width, env.length
    got = env.global_state(_lib.MAP_ALL)
    env.check()
    assert got.dtype == env._torch.uint8 and tuple(got.shape) == (B, 5 + 2 * N, W, L)
    got = got.cpu().numpy()
    labels = env.global_state_planes(_lib.MAP_ALL)
    assert labels == list(ORDER[:5]) + [f"free{i}" for i in range(N)] + [f"obst{i}" for i in range(N)]
    want = stack(ref, ORDER)
    for p, label in enumerate(labels):
        np.testing.assert_array_equal(got[:, p], want[:, p], err_msg=label)
    # non-vacuity: every layer kind has zero and non-zero cells, and the grids differ
    for name in ORDER:
        assert ref[name].any() and not ref[name].all(), name
    assert sorted(np.unique(ref["robots"]).tolist()) == [0, 1, 2, 3]
    assert not np.array_equal(ref["grid_neg"][0], ref["grid_neg"][1])
    assert np.array_equal(ref["grid_neg"][0], ref["grid_neg"][2])


def test_pooled_all_layers(small):
    from marlcov import _lib
    env, ref = small
    tr, tc = -(-env.width // 8), -(-env.length // 8)
    got = env.global_state(_lib.MAP_ALL, scale=8)
    env.check()
    assert tuple(got.shape) == (B, 5 + 2 * N, tr, tc)
    got = got.cpu().numpy()
    want = pool8(stack(ref, ORDER), robots_plane=4)
    for p, label in enumerate(env.global_state_planes(_lib.MAP_ALL)):
        np.testing.assert_array_equal(got[:, p], want[:, p], err_msg=label)
    assert ((want > 0) & (want < 64)).any()
    if env.width % 8:  # cells of grid_neg's edge tiles beyond the grid do not count
        assert want[:, 0, -1].max() <= 8 * (env.width % 8)
    assert want[:, 4].sum() == B * N


def test_subset_and_order(small):
    env, ref = small
    torch = env._torch
    sel = [4, 1, 1, 5]
    layers = ("free", "robots")
    assert env.global_state_planes(layers) == ["robots"] + [f"free{i}" for i in range(N)]
    want = stack(ref, layers, sel)
    got = env.global_state(layers, envs=sel)
    assert tuple(got.shape) == (4, 1 + N, env.width, env.length)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    out = torch.full_like(got, 0xAB)
    again = env.global_state(layers, envs=torch.tensor(sel, device=env.device), out=out)
    assert again is out
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    # the default layers, and one name
    np.testing.assert_array_equal(env.global_state().cpu().numpy(), stack(ref, ("visited", "obst_any", "robots")))
    np.testing.assert_array_equal(env.global_state("obst", envs=[2]).cpu().numpy(), stack(ref, ("obst",), [2]))
    env.check()


def test_bad_index_leaves_its_slot_and_is_reported(small):
    from marlcov import _lib
    env, ref = small
    torch = env._torch
    idx = torch.tensor([0, B, 2], dtype=torch.int32, device=env.device)
    for scale in (1, 8):
        layers = ("visited", "obst_any", "robots", "obst")
        out = torch.full_like(env.global_state(layers, envs=[0, 0, 0], scale=scale), 0xAB)
        env.check()
        env.global_state(layers, envs=idx, scale=scale, out=out)
        with pytest.raises(_lib.MarlcovError, match=r"0x40.*64=export_maps index.*bit 64"):
            env.check()
        env.check()  # reported once, then clean
        want = stack(ref, layers, [0, 2])
        if scale == 8:
            want = pool8(want, robots_plane=2)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[[0, 2]], want)
        assert (got[1] == 0xAB).all()


def test_export_reads_state_only(torch_cuda):
    from marlcov import _lib
    a, b = make_small(SHAPES["37x45"]), make_small(SHAPES["37x45"])
    ra = run_steps(a, 8)
    rb = run_steps(b, 8, between=lambda: (b.global_state(_lib.MAP_ALL), b.global_state(_lib.MAP_ALL, scale=8)))
    for t, (x, y) in enumerate(zip(ra, rb)):
        for u, v, what in zip(x, y, ("obs", "reward", "done")):
            np.testing.assert_array_equal(u, v, err_msg=f"step {t} {what}")
    np.testing.assert_array_equal(a.get_state(_lib.FIELD_FREE).cpu().numpy(), b.get_state(_lib.FIELD_FREE).cpu().numpy())
    assert a.env_launches() == b.env_launches()
    a.check(), b.check()
    a.close(), b.close()


def test_argument_errors_name_the_argument(small):
    from marlcov import _lib
    env, _ = small
    torch = env._torch
    with pytest.raises(ValueError, match="out must be"):
        env.global_state(out=torch.zeros((B, 3, env.width, env.length + 1), dtype=torch.uint8, device=env.device))
    with pytest.raises(_lib.MarlcovError, match="scale 4"):
        env.global_state(scale=4)
    with pytest.raises(_lib.MarlcovError, match="layers 0x0"):
        env.global_state(layers=0)
    with pytest.raises(ValueError, match="unknown layer 'walls'"):
        env.global_state(layers=("visited", "walls"))
    out = torch.zeros((B - 1, 1, env.width, env.length), dtype=torch.uint8, device=env.device)
    with pytest.raises(_lib.MarlcovError, match=r"count 5 with dev_envs NULL"):
        _lib.check(env.lib.mc_export_maps(env._h, _lib.MAP_VISITED, 1, None, B - 1, out.data_ptr(), out.numel(),
                                          env._stream()), "mc_export_maps")
    with pytest.raises(_lib.MarlcovError, match="out_bytes"):
        _lib.check(env.lib.mc_export_maps(env._h, _lib.MAP_VISITED, 1, None, B, out.data_ptr(), out.numel(),
                                          env._stream()), "mc_export_maps")
    with pytest.raises(_lib.MarlcovError, match="16-byte aligned"):
        flat = torch.zeros(B * env.width * env.length + 16, dtype=torch.uint8, device=env.device)
        _lib.check(env.lib.mc_export_maps(env._h, _lib.MAP_VISITED, 1, None, B, flat.data_ptr() + 1,
                                          B * env.width * env.length, env._stream()), "mc_export_maps")
    assert tuple(env.global_state(envs=[]).shape) == (0, 3, env.width, env.length)
    # the env still steps (on a copy of its state: the module's env stays as it is)
    twin = env.sibling(B)
    twin.fork(list(range(B)), env)
    twin.step(twin.random_actions(SEED, STEPS))
    twin.check()
    twin.close()
    env.check()


def test_c2_shape_once(torch_cuda):
    """64 envs, 4 agents, 128 x 128, lidar of 21 beams and range 10: planes of
    130 x 130 = 16,900 bytes (a multiple of 4, not of 16), 17 x 17 tiles in
    5 x 5 blocks"""
    import marlcov
    cfg = small_cfg(numrobot=4, sensor_type="lidar", sensor_config={"num_lasers": 21, "range": 10})
    env = marlcov.BatchCoverageEnv(cfg, 64, gen=dict(width=128, length=128, prob_obst=0.1, seed=7, num_grids=64),
                                   seed=11, auto_reset=False)
    env.reset()
    run_steps(env, 6)
    sel = [0, 21, 42, 63]
    ref = host_planes(env, sel)
    layers = ("visited", "obst_any", "robots")
    dense = stack(ref, layers)
    assert dense.shape == (4, 3, 130, 130) and all(dense[:, p].any() for p in range(3))
    np.testing.assert_array_equal(env.global_state(envs=sel).cpu().numpy(), dense)
    pooled = env.global_state(envs=sel, scale=8)
    assert tuple(pooled.shape) == (4, 3, 17, 17)
    np.testing.assert_array_equal(pooled.cpu().numpy(), pool8(dense, robots_plane=2))
    # all envs in order (dev_envs NULL) agree with the sampled slots
    np.testing.assert_array_equal(env.global_state()[sel].cpu().numpy(), dense)
    env.check()
    env.close()

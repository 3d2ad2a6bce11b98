"""GPU: DecGridRL's dist_reward distance transform (csrc/mc_dist.hip) compared
with the oracle over the whole extended grid, once per kernel row.

Only a small part of the transform's field leaves the device: (M, witness),
one cell per agent in the reward and the E x E crop around the robot.  Here
the crops are made to tile the field.  egoradius 15 gives E = 31 and pad = 15;
an agent at the padded cell (x, y) gets the crop of the extended rows x ..
x + 30 and columns y .. y + 30 (extended cell = padded cell + pad).  With one
env per x in {1, 32, 63, ...} + {Wp - 2} and one agent per y in {1, 32, 63,
...} + {Lp - 2} the crops cover the extended grid but its outermost ring (the
test asserts exactly that); the ring is left to the (M, witness) check, M
being usually attained there.  The square sensor of range 1 with
single_square_tool adds only the robot's own cell to its map, so the crops
stay full of nonzero distances, and the map itself is authored
(set_global_state): the same free plane for every agent of every env of a
run, patterns that make distances long or put all coverage in the last rows.

Grids are unpadded (RX - 32) x 65: RY = 97 extended columns are three full
strips of 32 and a strip with one valid column, two 64-column map words, and
strip offsets 17 and 49 into them.  RX, the extended rows, takes the edges of
chunk_rows, kMaxRows and kBigMaxRows of the default 512-thread build:

  256   dist_kernel_t<8>, every chunk full, no padding row
  257   first size of dist_kernel_t<17>
  545   first size of dist_kernel_t<26>
  832   last size of the LDS-bitboard kernel (and of the top-cell cache)
  833   first size of dist_big_kernel
  1088  the accepted maximum: 64 chunks of 17 rows, all full, 63 rows past
        row 1024 (where the column pass's row offset of 1024 ended: a covered
        cell in a row u > 1024 + g made every distance below it in its column
        u' - 1024 instead of g + u' - u)

Reference: the oracle env (oracle/cpu_ref.py, SciPy's exact L1 transform; the
reference's cv2 is absent), filled from the authored state and stepped beside
the device: reward, done, the obs with the float32 distance layer, the state
(compare_env) and every (M, witness) (check_dist_mw), all exact.  The first
step is a no-op for every agent: its PRE transform sees exactly the authored
map, its POST transform that map plus each robot's own cell.
"""
import os
import re
import zlib

import numpy as np
import pytest

from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from oracle.cpu_ref import distance_map, l1_distance_to_covered
from test_gpu_parity import base_cfg, bern, check_dist_mw, full_obs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EGO = 15
E = 2 * EGO + 1
PAD = EGO
SEED = 1088
RX = {"rx256": 256, "rx257": 257, "rx545": 545, "rx832": 832, "rx833": 833, "rx1088": 1088}
PATTERNS = ("corners", "bottom_band", "last_row", "one_column", "sparse")
# every pattern where the kernel changes and at the last accepted size, two at the other edges
CASES = [(r, p, None) for r in RX for p in PATTERNS
         if (r in ("rx832", "rx833", "rx1088") or p in ("bottom_band", "sparse")) and (r, p) != ("rx832", "sparse")]
# split over workgroups (the default) and whole in one workgroup (mode 2 / mode 1 of dist_kernel_t)
CASES += [("rx832", "sparse", "1"), ("rx832", "sparse", "0")]
PAST_1024 = ("bottom_band", "last_row", "sparse")  # patterns with coverage in extended rows > 1024 at rx1088


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def kernel_row_edges():
    """The extended row counts at which mc_dist.hip changes kernel or
    instantiation in its default build, read from the source."""
    src = open(os.path.join(ROOT, "marl-coverage_amd", "csrc", "mc_dist.hip")).read()

    def num(pattern):
        m = re.search(pattern, src)
        assert m, pattern
        return [int(g) for g in m.groups()]

    threads, = num(r"#define MC_DT_THREADS (\d+)")
    lo, mid = num(r": \(RX <= (\d+) \? 8 : \(RX <= (\d+) \? 17 : 26\)\)")
    small_max, = num(r"constexpr int kMaxRows = (\d+);")
    big_ch, = num(r"constexpr int kBigCh = (\d+);")
    big_cl, = num(r"constexpr int kBigCL = (\d+);")
    return threads, [lo, lo + 1, mid + 1, small_max, small_max + 1, big_ch * big_cl]


def field_cfg(n):
    return base_cfg(numrobot=n, dist_reward=1, egoradius=EGO, sensor_type="square_sensor",
                    sensor_config={"range": 1}, single_square_tool=1)


def lattice(n):
    """start coordinates whose 31-cell crops tile the extended cells 1 .. n + 2 * PAD - 2 of
    a padded axis of n cells: 1, 32, 63, ... and the last interior cell"""
    return sorted(set(range(1, n - 1, E)) | {n - 2})


def pattern_plane(pattern, case, wp, lp):
    """the authored free plane, uint8 [wp, lp] in padded coordinates (interior cells only)"""
    f = np.zeros((wp, lp), dtype=np.uint8)
    rs = np.random.RandomState(zlib.crc32(case.encode()))
    if pattern == "corners":
        f[[1, 1, wp - 2, wp - 2], [1, lp - 2, 1, lp - 2]] = 1
    elif pattern == "bottom_band":  # about 2 % of the last 48 map rows, nothing else
        f[wp - 49:wp - 1, 1:lp - 1] = rs.rand(48, lp - 2) < 0.02
    elif pattern == "last_row":
        f[wp - 2, 1:lp - 1] = 1
    elif pattern == "one_column":
        f[1:wp - 1, 40] = 1
    elif pattern == "sparse":
        f[1:wp - 1, 1:lp - 1] = rs.rand(wp - 2, lp - 2) < 0.005
    else:
        raise KeyError(pattern)
    assert f.any()
    return f


def ext_field(plane):
    """the reference's d over the extended grid of a padded free plane (float32; all inf
    where the oracle's transform has no covered cell to measure from)"""
    ext = np.pad(plane, PAD)
    if not ext.any():
        return np.full(ext.shape, np.inf, dtype=np.float32)
    return l1_distance_to_covered(ext)


def check_reference_side(pattern, plane, xs, ys, rx, tiles_rows=True):
    """Non-vacuity, on the reference alone: the crops' union, and how many of the first
    step's compared cells are nonzero, far, and decided by coverage past row 1024."""
    ry = plane.shape[1] + 2 * PAD
    d0 = ext_field(plane)
    assert d0.shape == (rx, ry)
    seen = np.zeros((rx, ry), dtype=bool)
    du, dv = np.abs(np.arange(E) - EGO)[:, None], np.abs(np.arange(E) - EGO)[None, :]
    nonzero = far = total = 0
    for x in xs:
        for y in ys:
            seen[x:x + E, y:y + E] = True
            # the POST map of the first step: the pattern and the robot's own cell (the crop's centre)
            crop = np.minimum(d0[x:x + E, y:y + E], du + dv)
            assert crop.shape == (E, E)
            total += crop.size
            nonzero += int((crop > 0).sum())
            far += int((crop >= 16).sum())
    want = np.zeros((rx, ry), dtype=bool)
    if tiles_rows:
        want[1:rx - 1, 1:ry - 1] = True  # everything but the outermost ring
        np.testing.assert_array_equal(seen, want, err_msg="the crops do not tile the extended grid")
    else:  # a few envs: every column of their rows
        rows = seen.any(axis=1)
        want[rows, 1:ry - 1] = True
        np.testing.assert_array_equal(seen, want, err_msg="the crops do not tile their rows")
    assert 2 * nonzero >= total, (nonzero, total)
    assert far >= 1000, far
    if rx > 1026 and pattern in PAST_1024:
        cut = plane.copy()
        cut[1025 - PAD:] = 0  # without the covered cells of the extended rows > 1024
        assert cut.sum() < plane.sum()
        d1 = ext_field(cut)
        decided = seen & (d1 > d0)
        decided[:1026] = False
        assert int(decided.sum()) >= 500, int(decided.sum())
    return d0


def first_dist_mismatch(got, want, ref):
    """the first differing cell of the distance layers of one env, for the message"""
    bad = np.argwhere(got[:, 3] != want[:, 3])
    if not len(bad):
        return ""
    i, r, c = (int(v) for v in bad[0])
    u, v = int(ref._xinds[i]) + r, int(ref._yinds[i]) + c
    return (f" dist layer: {len(bad)} cells differ, first at agent {i} extended cell ({u}, {v}): "
            f"device {got[i, 3, r, c]!r}, oracle {want[i, 3, r, c]!r}")


def step_beside(env, refs, cfg, acts, tag):
    """One step of env and oracles (as test_gpu_import_maps.step_beside_oracle): reward,
    done, the obs with the float32 distance layer, the state, (M, witness) of every map."""
    obs, rew, done = env.step(acts)
    acts = acts.cpu().numpy()
    obs, rew, done = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
    st = device_state(env)
    for b, ref in refs.items():
        o, r, d = ref.step(ref_action(acts[b]))
        tg = f"{tag} env {b}"
        o = np.asarray(o)
        assert float(r) == rew[b], (tg, "reward", float(r), rew[b], first_dist_mismatch(obs[b], o, ref))
        assert bool(d) == bool(done[b]), tg
        np.testing.assert_array_equal(obs[b], o, err_msg=tg + " obs" + first_dist_mismatch(obs[b], o, ref))
        assert o[:, 3].any(), tg + ": the oracle's dist layer is empty"
        compare_env(st, b, ref, tg)
    check_dist_mw(env, refs, tag)


def run_field(torch, rx, length, pattern, case, xs=None, steps=3):
    import marlcov
    from marlcov import _lib
    threads, edges = kernel_row_edges()
    if threads != 512 or edges != sorted(RX.values()):
        pytest.skip(f"mc_dist.hip's row edges are {edges} at {threads} threads, not {sorted(RX.values())} at 512")
    wp, lp = rx - 2 * PAD, length + 2
    ys = lattice(lp)
    xs = lattice(wp) if xs is None else xs
    B, N = len(xs), len(ys)
    plane = pattern_plane(pattern, case, wp, lp)
    check_reference_side(pattern, plane, xs, ys, rx, tiles_rows=xs == lattice(wp))
    cfg = field_cfg(N)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[np.ones((wp - 2, length))], auto_reset=False, seed=SEED)
    assert env.width + 2 * env.pad == rx and env.length + 2 * env.pad == lp + 2 * PAD
    if rx == max(RX.values()):
        assert _lib.load().mc_build_param(_lib.PARAM_DIST_MAX_ROWS) == rx
    pos = np.array([[(x, y) for y in ys] for x in xs], dtype=np.int32)
    env.reset(positions=pos)
    free = torch.from_numpy(plane).to(env.device).expand(B, N, wp, lp)
    env.set_global_state(free, "free")
    env.check()
    assert (env.get_state(_lib.FIELD_DIST_MW)[..., 0] == -1).all()
    # the oracles, from the authored maps (the rest is the env's own state after its reset)
    st = device_state(env)
    np.testing.assert_array_equal(st["pos"], pos)
    st["free"] = np.broadcast_to(plane, (B, N, wp, lp))
    st["vis"] = np.broadcast_to(plane, (B, wp, lp))
    refs = {b: oracle_from_device(st, b, cfg) for b in range(B)}
    step_beside(env, refs, cfg, torch.full((B, N), 4, dtype=torch.uint8, device=env.device), f"{case} no-op")
    assert int(env.get_state(_lib.FIELD_DIST_LISTED).item()) == B * N  # every map was transformed
    for t in range(steps):
        step_beside(env, refs, cfg, env.random_actions(SEED, t), f"{case} t={t}")
    env.check()
    env.close()


@pytest.mark.parametrize("rx,pattern,split", CASES,
                         ids=[f"{r}-{p}" + ("" if s is None else f"-split{s}") for r, p, s in CASES])
def test_field_matches_oracle(torch_cuda, monkeypatch, rx, pattern, split):
    """The whole field but its outermost ring, at one kernel row edge and one coverage
    pattern; rx832-sparse with MARLCOV_DIST_SPLIT 1 and 0."""
    if split is not None:
        monkeypatch.setenv("MARLCOV_DIST_SPLIT", split)
    run_field(torch_cuda, RX[rx], 65, pattern, f"{rx}-{pattern}")


def test_field_wide_map_split_in_parts(torch_cuda, monkeypatch):
    """rx832-sparse on a map of 300 columns (RY = 332: 11 strips, 11 agents per env on
    the column lattice) with 8 envs spread evenly over the rows.  88 listed maps: the
    split transform (mc_dist.hip, dist_kernel_t's S) takes min(11 strips, kMaxParts = 8,
    kSplitSlots / 88 = 5) = 5 parts per map, where the 108 maps of 4 strips of the
    65-column case take 4."""
    monkeypatch.setenv("MARLCOV_DIST_SPLIT", "1")
    wp = RX["rx832"] - 2 * PAD
    xs = sorted({int(round(x)) for x in np.linspace(1, wp - 2, 8)})
    assert len(xs) == 8
    run_field(torch_cuda, RX["rx832"], 300, "sparse", "rx832-sparse-wide", xs=xs)


def test_maps_with_nothing_covered(torch_cuda):
    """Two of four envs get all-zero free planes: at the next step's PRE transform their
    maps have no covered cell (M = -1, the oracle's -1 field: write_map_terms), the POST
    transform sees the robot's own cell only.  40 x 40, egoradius 2, two steps."""
    import marlcov
    from marlcov import _lib
    torch = torch_cuda
    B, N = 4, 3
    cfg = base_cfg(numrobot=N, dist_reward=1, sensor_type="square_sensor", sensor_config={"range": 1},
                   single_square_tool=1)
    rs = np.random.RandomState(40)
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[bern(rs, 40, 40, 0.1) for _ in range(B)], auto_reset=False,
                                   seed=SEED)
    env.reset()
    empty = [1, 3]
    wp, lp = env.width, env.length
    env.set_global_state(torch.zeros((2, N, wp, lp), dtype=torch.uint8, device=env.device), "free", envs=empty)
    env.check()
    mw = env.get_state(_lib.FIELD_DIST_MW).cpu().numpy()[..., 0]
    assert (mw[empty] == -1).all() and (mw[[0, 2]] >= 0).all()
    st = device_state(env)
    for e in empty:
        st["free"][e] = 0
        st["vis"][e] = 0
    refs = {b: oracle_from_device(st, b, cfg) for b in range(B)}
    # the reference's PRE field of an empty map: -1 everywhere, so 1 - d = 2 at every cell
    assert all((distance_map(refs[e]._free_pad[i]) == 2).all() for e in empty for i in range(N))
    for t in range(2):
        step_beside(env, refs, cfg, env.random_actions(SEED, t), f"empty t={t}")
    env.check()
    env.close()

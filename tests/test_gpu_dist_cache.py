"""GPU: the incremental paths of dist_reward's distance layer -- the witness
rule and the window targets of the env kernel (csrc/mc_env_step.h), the
per-map box, the top-cell cache's fast path and the re-transform with theta0
(csrc/mc_dist.hip) -- on authored maps and scripted walks
(dist_cache_cases.py), beside the oracle and beside a predictor of the path
every map takes.

Start-up as test_gpu_dist_field.run_field: an all-free grid, reset(positions),
set_global_state(free) with the authored plane of every agent, every M -1, the
oracles from the authored state, one all-no-op step: the import left the PRE
terms stale, so the step first transforms every map of the handle (without
theta0, outside the work list and its counters: M, witness and cache of every
map are taken there), and the robots stand on covered cells, so its env
kernel lists only maps with an unsettled target.  Then every scripted step is
compared exactly: reward (tolerance 0), done, the obs with the float32
distance layer, the state (compare_env), every (M, witness) against a fresh
oracle transform (check_dist_mw) -- and MC_FIELD_DIST_LISTED / _CACHED and the
MC_FIELD_DIST_TOTALS deltas against the predictor's sums (dist_cache_cases.
MapPredictor, driven by the oracle's newly covered cells and the witness the
device held before the step).  The counters must EQUAL the prediction in
every square-sensor scenario; F (lidar) asserts >=.

The predictor lists a map for three reasons, not two: M unknown, the witness
rule, and a target the staged block does not settle (dist_window).  The last
one does occur at egoradius 2, pad 2: the block starts at 8 floor((x0 - 3) /
8) for the cell x0 the robot stood on before its move, so after a move
towards smaller rows from x0 = 3 (mod 8) the target x - pad - 1 = x0 - 4 lies
outside it, and inside a hole the crop's far corner (d = 4 from the robot's
own cell) has only b = 3 to the block's edge once in 8 moves.  Such a map
keeps its M, is listed, and is served by the cache (its max is unchanged).

Scenarios (geometry checked by test_dist_cache_cases_cpu.py on the oracle):
  A          96 x 200, uncovered squares of 74 (max 80, top set 336) and 48
             cells (max 54) in two corners.  The diagonal walker erodes the
             larger: drops served by the cache down to 60, a re-transform at
             59 with theta0 whose 418 top cells lie in the strips of both
             holes (pruning, candidates across strips and parts), served
             drops down to 54, the hand-over, then moves the witness rule
             leaves unlisted.  Beside it a parked robot (never listed), a
             walker in the smaller hole (listed only by its targets), and a
             walker along the larger hole's edge row and column (its top set
             overflows: up to 1,181 cells).  Default and MARLCOV_DIST_SPLIT=0.
  A-upleft   the same mirrored and walked towards smaller rows and columns:
             every cached cell lies at lower coordinates than the box (the
             span transforms' o < 0 side).
  A'         the smaller hole 53 cells: max 59 = 80 - T - 1.
  A-5x5      range 2, every cell of the window: new cells off the robot's cell.
  B          no cache: one covered column (top set 1,848; CACHED == 0
             throughout), and the two planes of a family (a 30 x w corner
             rectangle, k covered cells on its rim) with top sets of exactly
             kDistK = 512 (w = 38, k = 10: cached) and 513 (k = 9: not).
  C          300 x 30 and 30 x 300: the first try's box is 286 cells (36
             tiles) by 5 (1 tile), past kSpan one way: one span transform is
             off and the other on.
  D          320 x 320: a box of 32 x 32 tiles (no try: a full transform) and
             of 31 x 30, the largest that MC_FAST_TILES stages (served).
  E          pad 7 > egoradius 2: the quirk targets, 6 .. 8 cells up-left,
             lie outside the 16 x 16 block unless it starts 8 .. 10 cells
             before the robot, so a map is listed nearly every step and the
             cache serves it; egoradius 3 (54 targets: dist_window proper).
  F          the C5 instantiation, 16 lidar agents; counters asserted >=.
  G          lifecycle: maxsteps with auto_reset mid-walk, fork into a second
             slot and a sibling, set_global_state on one of two envs.
"""
import copy

import numpy as np
import pytest

import dist_cache_cases as dc
from gpu_util import compare_env, device_state, oracle_from_device, ref_action
from test_gpu_dist_field import first_dist_mismatch
from test_gpu_parity import check_dist_mw, full_obs

pytestmark = pytest.mark.gpu

SEED = 512


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def consts():
    from marlcov import _lib
    c = dc.source_constants()
    if c != dc.GEOMETRY:
        pytest.skip(f"the build's constants are {c}; the scenarios were made for {dc.GEOMETRY}")
    lib = _lib.load()
    assert lib.mc_build_param(_lib.PARAM_DIST_CACHE_CELLS) == c["K"]
    assert lib.mc_build_param(_lib.PARAM_DIST_T) == c["T"]
    return c


def counters(env):
    from marlcov import _lib
    return (int(env.get_state(_lib.FIELD_DIST_LISTED).item()), int(env.get_state(_lib.FIELD_DIST_CACHED).item()),
            np.array(env.get_state(_lib.FIELD_DIST_TOTALS).cpu().tolist(), dtype=np.int64))


def device_mw(env):
    """(M, (witness x, y)) per map, padded coordinates (check_dist_mw's unpacking)"""
    from marlcov import _lib
    mw = env.get_state(_lib.FIELD_DIST_MW).cpu().numpy()
    w = mw[..., 1].astype(np.int64)
    return mw[..., 0], w >> 16, ((w & 0xFFFF) ^ 0x8000) - 0x8000


class Run:
    """An env beside its oracles and predictors."""

    def __init__(self, torch, env, cfg, consts, refs, preds=None, auto_reset=False):
        self.torch, self.env, self.cfg, self.consts, self.refs = torch, env, cfg, consts, refs
        self.auto_reset = auto_reset
        N = env.num_agents
        self.preds = preds or {b: [dc.MapPredictor(consts, cfg) for _ in range(N)] for b in refs}
        self.resets = 0

    def step(self, acts, tag, exact=True, prime=False):
        """One step of env, oracles and predictors; ``acts``: uint8 [N] (every env) or [B, N].
        ``prime``: the first step after an import, which transforms every map of the handle
        before its env kernel (MapPredictor.prime); it must cover no new cell, so that the
        witness that transform picks plays no part.  Returns {env: [StepPath per agent]}."""
        torch, env, cfg, refs = self.torch, self.env, self.cfg, self.refs
        B, N = env.num_envs, env.num_agents
        acts = np.broadcast_to(np.asarray(acts, dtype=np.uint8), (B, N)).copy()
        M, wx, wy = device_mw(env)
        tot0 = counters(env)[2]
        before = {b: (ref._free_pad.copy(), list(zip(ref._xinds.tolist(), ref._yinds.tolist()))) for b, ref in refs.items()}
        obs, rew, done = env.step(torch.from_numpy(acts).to(env.device))
        obs, rew, done = full_obs(env, obs, cfg), rew.cpu().numpy(), done.cpu().numpy()
        st = device_state(env)
        paths, want = {}, np.zeros(3, dtype=np.int64)  # listed, served, full
        for b, ref in refs.items():
            o, r, d = ref.step(ref_action(acts[b]))
            tg = f"{tag} env {b}"
            free_after = ref._free_pad.copy()
            pos1 = list(zip(ref._xinds.tolist(), ref._yinds.tolist()))
            assert float(r) == rew[b], (tg, "reward", float(r), rew[b], first_dist_mismatch(obs[b], np.asarray(o), ref))
            assert bool(d) == bool(done[b]), tg
            reset = bool(d) and self.auto_reset
            if reset:  # the device reset the env in the same launch: the oracle follows from its start cells
                self.resets += 1
                o, _ = ref.reset(False, None, positions=[tuple(int(v) for v in q) for q in st["pos"][b]])
            o = np.asarray(o)
            np.testing.assert_array_equal(obs[b], o, err_msg=tg + " obs" + first_dist_mismatch(obs[b], o, ref))
            assert o[:, 3].any(), tg + ": the oracle's layer 3 is empty"
            compare_env(st, b, ref, tg)
            row = []
            if prime:
                np.testing.assert_array_equal(free_after, before[b][0], err_msg=tg + ": a priming step covered cells")
            for i, p in enumerate(self.preds[b]):
                if prime:
                    M[b, i] = p.prime(before[b][0][i]).new_max
                if reset:  # a fresh map: no cache, M unknown, transformed as the reset left it
                    p.void()
                    q = (int(ref._xinds[i]), int(ref._yinds[i]))
                    row.append(p.step(-1, (0, 0), q, q, ref._free_pad[i], ref._free_pad[i]))
                else:
                    row.append(p.step(int(M[b, i]), (int(wx[b, i]), int(wy[b, i])), before[b][1][i], pos1[i],
                                      before[b][0][i], free_after[i]))
                want += (row[-1].listed, row[-1].served, row[-1].full)
            paths[b] = row
        check_dist_mw(env, refs, tag)
        assert (device_mw(env)[0] >= 0).all(), tag + ": a map's M is unknown after the step"
        listed, cached, tot1 = counters(env)
        np.testing.assert_array_equal(tot1 - tot0, [listed, cached, listed - cached, 1], err_msg=tag + " totals")
        got = np.array([listed, cached, listed - cached])
        detail = {b: [(p.listed, p.hit, p.unsettled, p.served, p.box_tiles, p.new_max) for p in row]
                  for b, row in paths.items()}
        if exact:
            assert len(refs) == B
            np.testing.assert_array_equal(got, want, err_msg=f"{tag}: (listed, served, full) {detail}")
        else:
            assert (got >= want).all(), (tag, got, want, detail)
        return paths


def start(torch, consts, scn, B=1, auto_reset=False, cfg=None, exact=True):
    """The start-up (module docstring): returns the Run after the all-no-op step."""
    import marlcov
    from marlcov import _lib
    cfg = cfg or scn.cfg
    N, Wp, Lp = scn.N, scn.W + 2, scn.L + 2
    env = marlcov.BatchCoverageEnv(cfg, B, grids=[np.ones((scn.W, scn.L))], auto_reset=auto_reset, seed=SEED)
    assert (env.width, env.length) == (Wp, Lp)
    pos = np.broadcast_to(scn.starts, (B, N, 2)).astype(np.int32).copy()
    env.reset(positions=pos)
    env.set_global_state(torch.from_numpy(scn.planes).to(env.device).expand(B, N, Wp, Lp), "free")
    env.check()
    assert (env.get_state(_lib.FIELD_DIST_MW)[..., 0] == -1).all()
    st = device_state(env)
    np.testing.assert_array_equal(st["pos"], pos)
    st["free"] = np.broadcast_to(scn.planes, (B, N, Wp, Lp))
    st["vis"] = np.broadcast_to(scn.planes.max(axis=0), (B, Wp, Lp))
    refs = {b: oracle_from_device(st, b, cfg) for b in range(B)}
    run = Run(torch, env, cfg, consts, refs, auto_reset=auto_reset)
    run.step(np.full(N, dc.STAY, dtype=np.uint8), f"{scn.name} no-op", exact, prime=True)
    return run


def walk(run, scn, t0, t1, exact=True, acts=None):
    """the scripted moves t0 .. t1 - 1; returns [t1 - t0]{env: [StepPath]}"""
    return [run.step(scn.script[t] if acts is None else acts(t), f"{scn.name} move {t + 1}", exact)
            for t in range(t0, t1)]


def run_scenario(torch, consts, scn, exact=True):
    run = start(torch, consts, scn, exact=exact)
    paths = walk(run, scn, 0, len(scn.script), exact)
    run.env.check()
    run.env.close()
    return [row[0] for row in paths]  # [steps][N]


def count(paths, i, what):
    return sum(bool(getattr(row[i], what)) for row in paths)


# ---------------------------------------------------------------------------
# A .. F
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,split", [("a", None), ("a", "0"), ("upleft", None), ("gap", None), ("5x5", None)],
                         ids=["A", "A-split0", "A-upleft", "A-gap", "A-5x5"])
def test_two_holes(torch_cuda, consts, monkeypatch, variant, split):
    """Scenario A and its variants: the served drops, the re-transform with theta0 of a
    map whose top cells lie in two holes, the hand-over and the unlisted tail, with
    exact counters every step.  split 0: MARLCOV_DIST_SPLIT=0, the try inside
    dist_kernel_t with 512 threads and no span transforms."""
    if split is not None:
        monkeypatch.setenv("MARLCOV_DIST_SPLIT", split)
    scn = dc.scenario_a(variant)
    paths = run_scenario(torch_cuda, consts, scn)
    d = scn.roles.index("diagonal")
    assert count(paths, d, "served") >= 20 and count(paths, d, "had_cache") >= 1
    assert all(not row[scn.roles.index("parked")].listed for row in paths)


@pytest.mark.parametrize("which", ["column", "below", "above"])
def test_overflow(torch_cuda, consts, which):
    """Scenario B.  column: 1,848 top cells, no map is ever served.  below / above: the
    planes overflow_pair() finds, top sets of 512 = kDistK (the cache is taken and serves)
    and 513 (no cache until a later transform finds 510)."""
    scn = dc.scenario_b(which)
    paths = run_scenario(torch_cuda, consts, scn)
    served = sum(count(paths, i, "served") for i in range(scn.N))
    if which == "column":
        assert served == 0 and sum(count(paths, i, "full") for i in range(scn.N)) >= 10
    else:
        assert scn.notes["top"] == consts["K"] + (which == "above")
        first = next(row[0] for row in paths if row[0].listed)
        assert first.served == (which == "below") and served >= 20


@pytest.mark.parametrize("transpose", [False, True], ids=["rows", "columns"])
def test_box_longer_than_span(torch_cuda, consts, transpose):
    """Scenario C: the first try after 280 unlisted moves has a box of more than kSpan
    rows (columns, transposed) and a few columns (rows)."""
    scn = dc.scenario_c(transpose)
    paths = run_scenario(torch_cuda, consts, scn)
    first = next(row[0] for row in paths if row[0].listed)
    long, short = first.box_tiles[::-1] if transpose else first.box_tiles
    assert first.served and 8 * long > consts["SPAN"] and 8 * short <= consts["SPAN"]


@pytest.mark.parametrize("which", ["over", "fits"])
def test_box_and_fast_tiles(torch_cuda, consts, which):
    """Scenario D: at the first listing the box is 32 x 32 tiles (no try, a full
    transform, CACHED 0) or 31 x 30 (tried and served)."""
    scn = dc.scenario_d(which)
    paths = run_scenario(torch_cuda, consts, scn)
    first = next(row[0] for row in paths if row[0].listed)
    if which == "over":
        assert first.box_tiles == (32, 32) and not first.tried and first.full and first.had_cache
    else:
        assert first.box_tiles == (31, 30) and first.tried and first.served


@pytest.mark.parametrize("ego", [2, 3])
def test_pad_and_egoradius(torch_cuda, consts, ego):
    """Scenario E.  ego 2, mini_map_rad 7: the quirk targets leave the staged block (the
    parked robot's map is listed and served every step).  ego 3: pad 3, T = 54 targets,
    dist_window instead of dist_window_am / _am2."""
    scn = dc.scenario_e(ego)
    paths = run_scenario(torch_cuda, consts, scn)
    parked = scn.roles.index("parked")
    assert count(paths, parked, "served") == (len(paths) if ego == 2 else 0)
    assert count(paths, scn.roles.index("top_row"), "had_cache") >= 1


def test_c5_instantiation(torch_cuda, consts):
    """Scenario F: 16 agents, 21 beams of range 10, egoradius 2 -- the C5 step kernel --
    on A's plane.  LISTED, CACHED and the full transforms are asserted >= the prediction
    (the lidar's marks are predicted by the same three rules; the inequality leaves room
    for a listing the predictor does not know).  Both the cache and the re-transform of a
    cached map must have run."""
    scn = dc.scenario_f()
    run = start(torch_cuda, consts, scn, exact=False)
    assert ",C5>" in run.env.kernel_variant(), run.env.kernel_variant()
    tot0 = counters(run.env)[2]
    paths = [row[0] for row in walk(run, scn, 0, len(scn.script), exact=False)]
    tot = counters(run.env)[2] - tot0
    with_cache = sum(count(paths, i, "had_cache") for i in range(scn.N))
    assert tot[1] > 0 and with_cache > 0 and tot[2] >= with_cache, (tot, with_cache)
    run.env.check()
    run.env.close()


# ---------------------------------------------------------------------------
# G: lifecycle, on A's plane with the diagonal walker and the parked robot
# ---------------------------------------------------------------------------
def test_auto_reset_mid_walk(torch_cuda, consts):
    """maxsteps = 85 with auto_reset: the walker's map is reset during its served drops.
    The reset map is listed and fully transformed (never served), the oracle goes on from
    the device's start cells, and the script continues for 25 moves."""
    scn = dc.scenario_a("solo")
    cfg = dict(scn.cfg, maxsteps=85)
    run = start(torch_cuda, consts, scn, auto_reset=True, cfg=cfg)
    paths = [row[0] for row in walk(run, scn, 0, 110)]
    assert run.resets == 1
    at = 85 - 2  # the no-op was step 1: move 84 is step 85
    assert paths[at][0].full and not paths[at][0].had_cache and not paths[at][0].served
    assert count(paths[:at], 0, "served") >= 8
    run.env.check()
    run.env.close()


def test_fork_keeps_the_cache(torch_cuda, consts):
    """After 70 moves env 0 is forked into env 1 (which had stayed parked) and into a
    sibling: all three then take the served drops, the re-transform with theta0 and the
    hand-over from the copied caches, each with the counters the predictor gives for it."""
    torch = torch_cuda
    scn = dc.scenario_a("pair")
    run = start(torch, consts, scn, B=2)
    stay = np.full(scn.N, dc.STAY, dtype=np.uint8)
    walk(run, scn, 0, 70, acts=lambda t: np.stack([scn.script[t], stay]))
    env = run.env
    env.fork(torch.tensor([-1, 0], dtype=torch.int32))
    sib = env.sibling(1)
    sib.fork(torch.tensor([0], dtype=torch.int32), source=env)
    env.check()
    sib.check()
    run.refs[1] = copy.deepcopy(run.refs[0])
    for p, q in zip(run.preds[1], run.preds[0]):
        p.copy_from(q)
    other = Run(torch, sib, run.cfg, consts, {0: copy.deepcopy(run.refs[0])},
                {0: [copy.deepcopy(p) for p in run.preds[0]]})
    paths = []
    for t in range(70, 110):
        a = run.step(scn.script[t], f"fork move {t + 1}")
        b = other.step(scn.script[t], f"fork sibling move {t + 1}")
        paths.append([a[0][0], a[1][0], b[0][0]])
    # (the copies may part after the re-transform: it fills each copy's cache in an order of
    # its own, and at the hand-over, both holes at 54, the served witness is the last
    # cached cell at the max)
    for i in range(3):
        assert count(paths, i, "served") >= 20 and count(paths, i, "had_cache") == 1
    env.check()
    sib.check()
    sib.close()
    env.close()


def test_import_voids_one_env(torch_cuda, consts):
    """set_global_state on env 1 of two after 70 moves (its own current maps): env 1's
    maps lose M and cache at once, env 0's keep theirs.  The next step (a no-op) then
    transforms every map of the handle for the PRE terms, env 0's too: their caches are
    retaken at the current max.  Both envs walk on through the served drops."""
    torch = torch_cuda
    scn = dc.scenario_a("pair")
    run = start(torch, consts, scn, B=2)
    walk(run, scn, 0, 70)
    ref, p = run.refs[1], run.refs[1]._pad
    planes = (ref._free_pad[:, p:p + scn.W + 2, p:p + scn.L + 2] > 0).astype(np.uint8)
    run.env.set_global_state(torch.from_numpy(planes[None]).to(run.env.device), "free", envs=[1])
    run.env.check()
    for q in run.preds[1]:
        q.void()
    M = device_mw(run.env)[0]
    assert (M[0] >= 0).all() and (M[1] == -1).all()
    run.step(np.full(scn.N, dc.STAY, dtype=np.uint8), "import no-op", prime=True)
    paths = walk(run, scn, 70, 110)
    assert not any(row[b][scn.roles.index("parked")].listed for row in paths for b in (0, 1))
    served = [sum(bool(row[b][0].served) for row in paths) for b in (0, 1)]
    assert served[0] >= 20 and served[1] >= 15, served
    run.env.check()
    run.env.close()

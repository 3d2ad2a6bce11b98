"""CPU: the scenarios of dist_cache_cases.py hold the phases they are meant to
hold -- shown on the oracle alone, with the predictor's stand-in witness (of
the cells with d == max d the one farthest from the robot).  If a scenario
degenerates (a plane, a walk or a build constant changes), this fails, not the
GPU test that would silently stop reaching its path."""
import functools

import numpy as np
import pytest

import dist_cache_cases as dc


@pytest.fixture(scope="module")
def consts():
    c = dc.source_constants()
    if c != dc.GEOMETRY:
        pytest.skip(f"the source's constants are {c}; the scenarios were made for {dc.GEOMETRY}")
    return c


@functools.lru_cache(maxsize=None)
def simulated(make, *args):
    scn = make(*args)
    return scn, dc.simulate(scn)


def column(sim, i):
    return [row[i] for row in sim]


def test_predictor_blocks():
    """block_unsettled restates dist_window's test: outside the block; inside with the
    nearest covered cell of the block within b; and a covered cell just outside the block
    at distance b does not settle the target."""
    free = np.zeros((40, 40), dtype=np.uint8)
    tg = np.array([[8, 8]])
    assert dc.block_unsettled(free, 2, 0, 0, 16, tg)           # nothing covered
    free[8 + 2, 11 + 2] = 1
    assert not dc.block_unsettled(free, 2, 0, 0, 16, tg)       # d = 3 <= b = 8
    assert dc.block_unsettled(free, 2, 0, 0, 16, np.array([[8, -1]]))  # outside
    far = np.zeros((40, 40), dtype=np.uint8)
    far[2 + 2, 16 + 2] = 1                                     # column 16: the first outside the block
    assert dc.block_unsettled(far, 2, 0, 0, 16, np.array([[2, 13]]))   # b = 3, d = 3 but outside
    far[2 + 2, 15 + 2] = 1
    assert not dc.block_unsettled(far, 2, 0, 0, 16, np.array([[2, 13]]))
    assert dc.window_tiles(2) == 2 and dc.window_tiles(10) == 4
    assert dc.sensing_half_width(dc.square_cfg(1)) == 2 and dc.sensing_half_width(dc.base_cfg()) == 10


@pytest.mark.parametrize("variant", ["a", "upleft", "5x5", "pair", "solo"])
def test_two_holes_phases(consts, variant):
    scn, sim = simulated(dc.scenario_a, variant)
    T = consts["T"]
    assert dc.top_set(dc.two_holes(), 2, T) == (80, 336)
    assert dc.top_set(dc.two_holes(right=0), 2, T)[0] == 54
    p = column(sim, scn.roles.index("diagonal"))
    assert p[0].full and p[0].top == 336 and p[0].valid
    fulls = [t for t, q in enumerate(p) if q.full and t > 0]  # (entry 0: the authored map's transform)
    assert len(fulls) == 1, fulls
    re = p[fulls[0]]
    # the re-transform: a valid cache (theta0), M = 80 - T - 1, 418 top cells in the strips of both holes
    assert re.had_cache and re.tried and re.new_max == 80 - T - 1 and re.top == (412 if variant == "5x5" else 418) and re.valid
    assert re.top_strips >= 2
    drops = [t for t in range(1, len(p)) if p[t].served and p[t].hit]
    assert len([t for t in drops if t < fulls[0]]) >= 20
    after = [t for t in drops if t > fulls[0]]
    assert len(after) >= 5
    hand_over = after[-1]
    assert p[hand_over].new_max == 54 and not any(q.hit for q in p[hand_over + 1:])
    tail = p[hand_over + 1:]
    if variant == "a":
        assert sum(not q.listed for q in tail) >= 40, sum(not q.listed for q in tail)
    assert all(q.served for q in tail if q.listed)  # listed by their targets only, the max unchanged
    if "parked" in scn.roles:
        assert not any(q.listed for q in column(sim, scn.roles.index("parked"))[1:])
    if "left_hole" in scn.roles:
        q = column(sim, scn.roles.index("left_hole"))[1:]
        assert not any(s.hit or s.full for s in q) and sum(s.served for s in q) >= 30
        q = column(sim, scn.roles.index("top_row"))[1:]
        assert sum(s.served and s.hit for s in q) >= 15
        assert any(s.full and s.had_cache and s.top > consts["K"] and not s.valid for s in q)
    if variant == "5x5":  # the new cells reach 2 cells past the robot's: the drops start 4 moves early
        base = column(simulated(dc.scenario_a, "pair")[1], 0)  # (and the walk starts 4 moves further out)
        assert min(t for t, q in enumerate(p) if q.hit) - 4 < min(t for t, q in enumerate(base) if q.hit)
        assert not any(q.unsettled for q in p)  # its targets' neighbourhood is covered: listed by the witness rule alone


def test_gap_phases(consts):
    """A': when the cached max falls to M0 - T - 1 = 59 the map is not served, and 59 is
    the true max (the other hole's): a serve test lax by a few cells would go on serving
    58, 57, ... from the cache."""
    scn, sim = simulated(dc.scenario_a, "gap")
    T = consts["T"]
    assert dc.top_set(dc.two_holes(left=53, right=0), 2, T)[0] == 80 - T - 1
    p = column(sim, 0)
    t = next(t for t, q in enumerate(p) if q.full and t > 0)
    assert p[t].had_cache and p[t].new_max == 80 - T - 1 and p[t - 1].served and p[t - 1].new_max == 80 - T
    assert all(q.new_max == 80 - T - 1 for q in p[t:] if q.listed)
    assert sum(q.listed for q in p[t + 1:]) >= 10


def test_overflow_phases(consts):
    K = consts["K"]
    scn, sim = simulated(dc.scenario_b, "column")
    assert dc.top_set(scn.planes[0], 2, consts["T"])[1] == 1848
    for i in range(scn.N):
        p = column(sim, i)
        assert not any(q.served or q.valid for q in p) and sum(q.full for q in p) >= 5
    below, above = dc.overflow_pair()
    assert (below[3], above[3]) == (K, K + 1), (below, above)
    scn, sim = simulated(dc.scenario_b, "below")
    p = column(sim, 0)
    assert p[0].top == K and p[0].valid and next(q for q in p[1:] if q.listed).served
    scn, sim = simulated(dc.scenario_b, "above")
    p = column(sim, 0)
    assert p[0].top == K + 1 and not p[0].valid
    first = next(t for t in range(1, len(p)) if p[t].listed)
    assert p[first].full and not p[first].had_cache
    assert any(q.full and q.valid for q in p[first:]) and sum(q.served for q in p) >= 20


@pytest.mark.parametrize("transpose", [False, True])
def test_long_box_phases(consts, transpose):
    scn, sim = simulated(dc.scenario_c, transpose)
    assert (scn.W, scn.L) == ((30, 300) if transpose else (300, 30))
    p = column(sim, 0)
    assert p[0].top == 336 and p[0].new_max == 30 and p[0].valid
    first = next(t for t in range(1, len(p)) if p[t].listed)
    assert first > 270
    long, short = p[first].box_tiles[::-1] if transpose else p[first].box_tiles
    assert p[first].tried and p[first].served and 8 * long > consts["SPAN"] >= 8 * short
    assert sum(q.served and q.hit for q in p[first:]) >= 10


def test_fast_tiles_phases(consts):
    F = consts["FAST_TILES"]
    assert 30 * 31 + 65 <= F < 31 * 31 + 65
    scn, sim = simulated(dc.scenario_d, "over")
    p = column(sim, 0)
    assert p[0].top == 336 and p[0].new_max == 66 and p[0].valid
    first = next(t for t in range(1, len(p)) if p[t].listed)
    assert p[first].box_tiles == (32, 32) and not p[first].tried and p[first].full and p[first].had_cache
    assert sum(q.served for q in p[first:]) >= 10
    scn, sim = simulated(dc.scenario_d, "fits")
    p = column(sim, 0)
    first = next(t for t in range(1, len(p)) if p[t].listed)
    assert p[first].box_tiles == (31, 30) and p[first].tried and p[first].served
    assert not any(q.full for q in p[1:])


@pytest.mark.parametrize("ego", [2, 3])
def test_pad_phases(consts, ego):
    scn, sim = simulated(dc.scenario_e, ego)
    parked = column(sim, scn.roles.index("parked"))[1:]
    if ego == 2:  # the quirk targets leave the block: listed by them alone, and served, every step
        assert all(q.listed and q.unsettled and not q.hit and q.served for q in parked)
    else:
        assert not any(q.listed for q in parked)
    top = column(sim, scn.roles.index("top_row"))[1:]
    assert sum(q.served and q.hit for q in top) >= 10 and any(q.full and q.had_cache for q in top)


def test_c5_phases(consts):
    scn, sim = simulated(dc.scenario_f)
    assert scn.N == 16 and dc.sensing_half_width(scn.cfg) == 10
    flat = [q for row in sim[1:] for q in row]
    assert sum(q.served for q in flat) >= 20 and sum(q.full and q.had_cache for q in flat) >= 1

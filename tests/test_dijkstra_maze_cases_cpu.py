"""CPU: every authored case of dijkstra_maze_cases.py has the property it was
authored for -- shown on the oracle's dijkstra_path_map and on
frontier_ref.nearest_target alone.  If a case degenerates (a canvas, a start
or an unknown cell changes), this fails, not the GPU test that would silently
stop testing what it is named for.  Nothing here is skipped or expected to
fail."""
import functools

import numpy as np
import pytest

import dijkstra_maze_cases as mz
from frontier_ref import expected_all, nearest_target
from oracle.cpu_ref import dijkstra_path_map

# (family, egoradius): the word families at both radii the GPU test runs, the rest once
FAMILY_EGOS = [(f, e) for f in mz.FAMILIES for e in (mz.EGOS if f.startswith("words_") else (2,))]


@functools.lru_cache(maxsize=None)
def solved(fam, ego):
    """[(case, i, agent, g, sx, sy, cost, end (extended), path)] of a family"""
    out = []
    for case in mz.family(fam, ego):
        for i, a in enumerate(case.agents):
            g, sx, sy = mz.planning_map(case, i, ego)
            cost, end = nearest_target(g, sx, sy)
            out.append((case, i, a, g, sx, sy, cost, end, dijkstra_path_map(g, sx, sy)))
    return out


def test_every_family_is_here():
    assert set(mz.FAMILIES) == {"detour", "long", "fork", "walk", "dieout", "border", "near", "words_ry128",
                                "words_ry129", "words_three"}
    for fam, ego in FAMILY_EGOS:
        cases = mz.family(fam, ego)
        assert len(cases) >= 1 and len(cases) <= 8
        assert len({c.shape for c in cases}) == 1 and len({len(c.agents) for c in cases}) == 1, fam
        assert len(cases[0].agents) <= 4
        assert len({c.name for c in cases}) == len(cases)


@pytest.mark.parametrize("fam,ego", FAMILY_EGOS)
def test_state_is_consistent(fam, ego):
    """free within the grid's free cells, obst within its obstacles, the wall ring known to
    be obstacle but for the authored ring cells, the robots distinct and on known free cells
    (but the agent that starts on an unexplored cell), and the oracle built from the planes
    holds the planning map the predictors use."""
    for case in mz.family(fam, ego):
        free, obst = mz.case_planes(case)
        gfree = case.canvas.free
        assert case.grid.shape == (gfree.shape[0] - 2, gfree.shape[1] - 2)
        assert not (free & ~gfree).any() and not (obst & gfree).any(), case.name
        assert not (free & obst).any(), case.name
        starts = [tuple(a.start) for a in case.agents]
        assert len(set(starts)) == len(starts), case.name
        st = mz.batch_state([case])
        assert st["free_cnt"][0] == free.sum() and st["vis_cnt"][0] == free.max(axis=0).sum()
        ref = mz.oracle_for(case, mz.square_cfg(len(case.agents), ego, dijkstra_input=1))
        for i, a in enumerate(case.agents):
            unknown = (free[i] | obst[i]) == 0
            assert sorted(map(tuple, np.argwhere(unknown))) == sorted(set(map(tuple, a.unknown))), (case.name, i)
            assert gfree[a.start], (case.name, i)
            assert bool(free[i][a.start]) == (a.d != 0), (case.name, i)
            g, sx, sy = mz.planning_map(case, i, ego)
            np.testing.assert_array_equal(ref._free_pad[i] - ref._obst_pad[i], g)
            assert (int(ref._xinds[i]) + ref._pad, int(ref._yinds[i]) + ref._pad) == (sx, sy)
        expected_all(ref)  # frontier_ref's own cross-checks hold on every case


@pytest.mark.parametrize("fam,ego", FAMILY_EGOS)
def test_declared_properties(fam, ego):
    """d*, the end point, the L1 bound, the number of shortest paths, the fork's losing
    cell, the chamber's last layer and window_lists, as each agent declares them."""
    for case, i, a, g, sx, sy, cost, end, path in solved(fam, ego):
        tag = (case.name, i)
        assert a.d is not None and a.lists is not None, tag
        assert cost == a.d, tag
        assert int(path.sum()) == (a.d + 1 if a.d >= 0 else 0), tag
        if a.d >= 0:
            assert a.end is not None and end == (a.end[0] + ego, a.end[1] + ego), tag
            assert path[end] == 1 and path[sx, sy] == 1, tag
        else:
            assert end is None and a.end is None, tag
        if a.l1_max is not None:
            assert 2 <= abs(end[0] - sx) + abs(end[1] - sy) <= a.l1_max, tag
        if a.min_paths is not None:
            assert mz.count_shortest_paths(g, sx, sy, end) >= a.min_paths, tag
        if a.loser is not None:
            lose = (a.loser[0] + ego, a.loser[1] + ego)
            assert g[lose] == 0 and path[lose] == 0, tag
            # its cost on the map without the winner: the same search would have ended there
            g2 = g.copy()
            g2[end] = 1
            assert nearest_target(g2, sx, sy) == (a.loser_cost, lose), tag
        if a.last_layer is not None:
            assert a.d == -1 and len(mz.bfs_layers(g, sx, sy)) - 1 == a.last_layer, tag
        assert mz.window_lists(g, sx, sy) == a.lists, tag
        # the predictor again from what was declared: listed iff the search passes layer 24
        assert a.lists == ((a.d if a.d >= 0 else a.last_layer) > mz.WINDOW_DEPTH
                           or (a.d < 0 and a.last_layer == mz.WINDOW_DEPTH)), tag


def ds(fam, ego=2):
    return [a.d for _, _, a, *_ in solved(fam, ego)]


def test_window_lists_on_small_maps():
    """the predictor on a bare corridor of n cells: a target at its end, then none"""
    for n in range(2, 30):
        g = -np.ones((3, n + 2))
        g[1, 1:n + 1] = 1
        assert mz.window_lists(g, 1, 1) is (n - 1 >= 24), n  # dies out at layer n - 1 ...
        g[1, n] = 0  # ... or meets the target there
        assert mz.window_lists(g, 1, 1) is (n - 1 > 24), n
    g = np.zeros((3, 3))
    assert not mz.window_lists(g, 1, 1)  # the start is a target
    assert not mz.window_lists(g, 1, 1, depth=0)


def test_detour_family():
    """every geodesic distance of 18..29 at an L1 distance of 2..6: both sides of the
    window kernel's 24 layers while the target stays a few cells away"""
    assert set(ds("detour")) == mz.DETOUR_D and mz.DETOUR_D >= set(range(20, 30))
    for _, _, a, g, sx, sy, cost, end, _ in solved("detour", 2):
        assert a.l1_max == 6 and abs(end[0] - sx) == 2


def test_long_family():
    """d* of about 50, 300 and >= 2000, many times the map's sides"""
    d = ds("long")
    assert [sum(1 for v in d if lo <= v <= hi) for lo, hi in ((45, 55), (295, 305), (1000, 1500))] == [3, 3, 2]
    assert sum(1 for v in d if v >= 2000) == 1  # once: the reference takes longest here
    W, L = mz.family("long")[0].shape
    assert W <= 64 and L <= 72 and max(d) > 30 * max(W, L)
    for case in mz.family("long"):
        assert case.notes["corridor"] > 2000


def test_fork_family():
    """the same four forks with the winner at 11, 24, 25 and 28: ends that differ in x,
    ends of equal x, a smaller cell one layer farther that loses, and a winner with the
    smaller x and the larger y"""
    assert sorted(set(ds("fork"))) == [11, 24, 25, 28]
    for case in mz.family("fork"):
        x, far, y, hook = case.agents
        assert x.end[0] < x.loser[0] and x.end[1] == x.loser[1] and x.loser_cost == x.d
        assert y.end[0] == y.loser[0] and y.end[1] < y.loser[1] and y.loser_cost == y.d
        assert tuple(far.loser) < tuple(far.end) and far.loser_cost == far.d + 1
        assert hook.end[0] < hook.loser[0] and hook.end[1] > hook.loser[1] and hook.loser_cost == hook.d


def test_walk_family():
    """two or more shortest paths to every end; over the family every direction is taken,
    +x, -x and +y are taken where another was valid too, and -x, +y and -y are passed over
    while valid (+x is first and -y last in the reference's order: no other outcome exists)"""
    chosen, won, lost = set(), set(), set()
    for case, i, a, g, sx, sy, cost, end, path in solved("walk", 2):
        assert a.min_paths >= 2
        c, w, l = mz.walk_ties(g, sx, sy, end)
        assert w and l, (case.name, i)
        chosen |= c
        won |= w
        lost |= l
    assert chosen == set(mz.DIR_NAMES)
    assert won == {"+x", "-x", "+y"} and lost == {"-x", "+y", "-y"}


def test_dieout_family():
    assert sorted(a.last_layer for _, _, a, *_ in solved("dieout", 2)) == [1, 5, 23, 24, 25, 26]
    assert [a.lists for _, _, a, *_ in solved("dieout", 2)] == [False] * 3 + [True] * 3
    for case in mz.family("dieout"):
        for a in case.agents:  # unknown cells exist, outside the chamber
            assert len(a.unknown) == 2


def test_border_family():
    """every end is a cell of the wall ring; the corner cells themselves are never chosen;
    the corner-tile robots stand in the map's four corner tiles"""
    Wp, Lp = mz.family("border")[0].shape
    for case, i, a, g, sx, sy, cost, end, path in solved("border", 2):
        x, y = a.end
        assert (x in (0, Wp - 1)) != (y in (0, Lp - 1)), (case.name, i)
    corners = {(0, 0), (0, Lp - 1), (Wp - 1, 0), (Wp - 1, Lp - 1)}
    for name in ("border_corners", "border_corner_tile", "border_corner_tile_far"):
        case = {c.name: c for c in mz.family("border")}[name]
        assert {tuple(u) for a in case.agents for u in a.unknown} >= corners
        if name != "border_corners":
            assert {(a.start[0] >> 3, a.start[1] >> 3) for a in case.agents} == \
                {(0, 0), (0, (Lp - 1) >> 3), ((Wp - 1) >> 3, 0), ((Wp - 1) >> 3, (Lp - 1) >> 3)}
    assert min(ds("border")) <= 24 < max(ds("border"))


def test_near_family():
    d = ds("near")
    assert d.count(0) == 1 and d.count(1) == len(d) - 1
    moves = set()
    for _, _, a, g, sx, sy, cost, end, _ in solved("near", 2):
        if a.d == 1:
            moves.add((end[0] - sx, end[1] - sy))
    assert moves == {(1, 0), (-1, 0), (0, 1), (0, -1)}


@pytest.mark.parametrize("ego", mz.EGOS)
def test_word_families(ego):
    """corridors on the extended columns 63 | 64 (and 127 | 128 with three words a row), a
    walk that turns on each boundary cell, ties across the boundary, RY a multiple of 64
    and RY % 64 == 1"""
    for name, ry, b in mz.WORD_SHAPES:
        (case,) = mz.family(name, ego)
        RY = case.shape[1] + 2 * ego
        assert case.notes["RY"] == RY and (ry is None or RY == ry)
        assert (RY + 63) // 64 == (3 if name != "words_ry128" else 2)
        lo, straight, hi, wide = [s for s in solved(name, ego)]
        for s, col in ((lo, b), (hi, b + 1)):
            path = s[8]
            assert path[:, col].sum() == 9 and path[:, 2 * b + 1 - col].sum() == 1  # down one side, across once
            turn = [c for c in zip(*np.nonzero(path)) if path[c[0] - 1, c[1]] and (path[c[0], c[1] - 1] or
                                                                                  path[c[0], c[1] + 1])]
            assert len(turn) == 1 and turn[0][1] == col
        assert straight[8][:, 63:65].sum() == 2 and (b != 127 or straight[8][:, 127:129].sum() == 2)
        assert wide[8][:, b].sum() + wide[8][:, b + 1].sum() == 12 and wide[2].min_paths == 11
    assert mz.family("words_ry128", ego)[0].notes["RY"] % 64 == 0
    assert mz.family("words_ry129", ego)[0].notes["RY"] % 64 == 1


@pytest.mark.parametrize("kind,n", sorted(mz.LOOP_STEPS))
def test_closed_loop_reference_steps(kind, n):
    """The oracle driven by frontier_ref.expected_all covers the maze at 100 % in
    LOOP_STEPS steps: the figure the GPU closed loop has to meet."""
    ref = mz.loop_oracle(kind, n)
    assert ref._grid.shape == (mz.LOOP_SHAPE[0] + 2, mz.LOOP_SHAPE[1] + 2)
    steps, done = 0, False
    while not done:
        assert steps < 1000
        _, _, done = ref.step(expected_all(ref)[0].astype(np.int64))
        steps += 1
    assert steps == mz.LOOP_STEPS[(kind, n)]
    assert ref.percent_covered() >= 1.0

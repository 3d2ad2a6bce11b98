"""Authored walks for the union dedup of the step kernels' merge (mc_env_step.h):
four robots on an open 94 x 94 map (padded 96 x 96), cells in padded
coordinates.  A robot's staged block of 4 x 4 tiles starts at tile
((x - 11) >> 3, (y - 11) >> 3); two blocks overlap when their origins differ
by at most 3 tiles in both axes, and the dedup counts a cell two robots mark in
one step at the lower-index robot only.

SCENARIOS: name -> (start cells, script of action rows, shared).  `shared`:
some step must have the robots' own new-cell counts add up to more than the
union's (tests/test_union_dedup_cases.py asserts it from the oracle alone).
Every scenario whose blocks overlap is shared but one: origins 3 tiles apart
in x and in y put the robots at least 17 cells apart in both axes, 24 cells
from each other, and two lidars of range 10 reach no common cell; dx3y1 and
dx1y3 stand in for it (a delta of 3 tiles in one axis with the other not zero).
The 4-tile scenarios have no overlap and only the dedup's range tests to pass.
DELTAS: name -> the pair's origin delta in tiles, for the delta scenarios."""
import numpy as np

from oracle.cpu_ref import DecGridRLRef

INNER = 94
FAR = [(84, 84), (84, 50)]  # where robots 2 and 3 wait in the two-robot scenarios
CORNERS = [(20, 20), (20, 76), (76, 20), (76, 76)]  # 7 tiles apart: no two blocks overlap


def grid():
    return np.ones((INNER, INNER))


def _delta(dx, dy):
    """Robots 0 and 1 with block origins (dx, dy) tiles apart and as close as
    that allows: robot 0 on the last cell of origin 0 (18), robot 1 on the
    first cell of origin d (8 d + 11) along the axes with a delta.  They walk
    side by side across the larger delta's axis (new cells on the same rim of
    both lidars, between them), four steps inside their tiles, so the delta
    holds in every step."""
    if dx >= dy:  # apart in x (and less in y): walk +y
        a = (18, 14) if dy else (18, 20)
        b = (8 * dx + 11, 8 * dy + 11) if dy else (8 * dx + 11, 20)
        return [a, b] + FAR, [(1, 1, 4, 4)] * 4
    a = (14, 18) if dx else (20, 18)
    b = (8 * dx + 11, 8 * dy + 11) if dx else (20, 8 * dy + 11)
    return [a, b] + FAR, [(0, 0, 4, 4)] * 4


def _pair(i, j):
    start = list(CORNERS)
    start[j] = (CORNERS[i][0], CORNERS[i][1] - 1)  # robot j beside robot i (behind it in y); the others in their corners
    return start, [(0, 0, 0, 0)] * 3 + [(1, 1, 1, 1)] * 2


SCENARIOS = {
    # lower robots in front, so that every move succeeds: all four blocks coincide
    "one_tile": ([(29, 29), (29, 28), (28, 29), (28, 28)], [(0, 0, 0, 0)] * 3 + [(1, 1, 1, 1)] * 2, True),
    # two robots side by side step together: both newly see the same cells
    "same_cells": ([(30, 30), (30, 31)] + FAR, [(0, 0, 4, 4)] * 4, True),
    # robots 0 and 1 walk x = 17 .. 21: their block origin moves from tile 0 to 1 at x = 19
    "origin_shift": ([(17, 30), (17, 31)] + FAR, [(0, 0, 4, 4)] * 4, True),
}
DELTAS = {}
for d in (1, 2, 3, 4):
    DELTAS[f"dx{d}"], DELTAS[f"dy{d}"], DELTAS[f"dxy{d}"] = (d, 0), (0, d), (d, d)
DELTAS["dx3y1"], DELTAS["dx1y3"] = (3, 1), (1, 3)
for name, (dx, dy) in DELTAS.items():
    s, a = _delta(dx, dy)
    SCENARIOS[name] = (s, a, max(dx, dy) <= 3 and (dx, dy) != (3, 3))
for i in range(4):
    for j in range(i + 1, 4):
        s, a = _pair(i, j)
        SCENARIOS[f"pair{i}{j}"] = (s, a, True)


def oracle_counts(cfg, start, script):
    """Per step of the script on the oracle: (sum over robots of the cells the
    robot newly marked free that the union did not hold, the union's new
    cells), and the cells after every step."""
    np.random.seed(0)
    ref = DecGridRLRef([grid()], cfg)
    ref.reset(False, None, positions=[tuple(p) for p in start])
    out, cells = [], [list(zip(ref._xinds.tolist(), ref._yinds.tolist()))]
    p, W, L = ref._pad, ref._gridwidth, ref._gridlen
    for a in script:
        f0 = ref._free_pad[:, p:p + W, p:p + L] > 0
        v0 = ref._visited > 0
        ref.step(np.asarray(a, dtype=np.int64))
        f1 = ref._free_pad[:, p:p + W, p:p + L] > 0
        v1 = ref._visited > 0
        own = int(sum(np.count_nonzero(f1[i] & ~f0[i] & ~v0) for i in range(len(start))))
        out.append((own, int(np.count_nonzero(v1 & ~v0))))
        cells.append(list(zip(ref._xinds.tolist(), ref._yinds.tolist())))
    return out, np.asarray(cells)

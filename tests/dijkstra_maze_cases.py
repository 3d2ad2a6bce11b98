"""Authored mazes for the BFS path kernels (csrc/mc_dijkstra.hip: the window
kernel, the whole-map LDS kernel, the whole-map HBM kernel; each with the crop
sink of dijkstra_input and the move sink of mc_frontier_actions), and host
predictors of what each kernel has to do on them.  Pure NumPy plus oracle/:
test_dijkstra_maze_cases_cpu.py shows on the oracle alone that every case has
the property it was authored for, test_gpu_dijkstra_mazes.py runs the cases
on the device beside the oracle.

Coordinates.  A case is drawn on the padded plane of Wp x Lp cells (the
device's map and robot coordinates), whose outermost ring is obstacle; x is
the row, y the column.  The oracle plans on the extended plane g = free_pad -
obst_pad of (Wp + 2 pad) x (Lp + 2 pad) cells (extended = padded + pad, pad =
egoradius), whose outer pad cells are never known.  The row bitboards of the
full kernels hold 64 extended columns per word.

A case gives the ground-truth grid, the robots' start cells and, per agent,
the cells it has NOT explored; every other padded cell, the wall ring
included, is known: free cells in the agent's free map, obstacles in its
obstacle map.  Depth comes from the geometry alone.

Every agent declares what it was authored for (Agent below); the CPU test
asserts each declaration against the oracle's dijkstra_path_map and
frontier_ref.nearest_target.  The d* and step figures written here are
literals: they were read once from that reference, never from the device.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from frontier_ref import STEPS, nearest_target
from gpu_util import oracle_from_device

WINDOW_DEPTH = 24  # kDjWinDepth: the BFS layers the window kernel holds exactly
EGO_MAX = 15       # the largest egoradius mc_create accepts: a 31 x 31 crop
EGOS = (EGO_MAX, 2)
DIR_NAMES = ("+x", "-x", "+y", "-y")  # the reference's neighbour order (frontier_ref.STEPS)


def base_cfg(**kw):
    """test_gpu_frontier.base_cfg (restated: that module needs a GPU's imports)"""
    c = dict(numrobot=1, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0, terminal_reward=30,
             dist_reward=0, train_maxsteps=1000, test_maxsteps=1000, egoradius=2, mini_map_rad=0, comm_radius=0,
             allow_comm=0, map_sharing=0, single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
             sensor_config={"num_lasers": 21, "range": 10})
    c.update(kw)
    return c


def square_cfg(n, ego, **kw):
    """The square sensor of range 1 with the single-square tool: a step adds the robot's own
    cell to its free map and the obstacles of the 3 x 3 around it to its obstacle map, so
    the authored knowledge survives a step."""
    c = dict(numrobot=n, egoradius=ego, sensor_type="square_sensor", sensor_config={"range": 1}, single_square_tool=1)
    c.update(kw)
    return base_cfg(**c)


# ---------------------------------------------------------------------------
# drawing
# ---------------------------------------------------------------------------
class Canvas:
    """A padded plane, all obstacle until carved."""

    def __init__(self, Wp, Lp):
        self.free = np.zeros((Wp, Lp), dtype=bool)

    def carve(self, cells):
        for x, y in cells:
            self.free[x, y] = True
        return list(cells)

    def path(self, *pts):
        """the cells of the axis-aligned polyline through ``pts``, in order, carved"""
        cells = [tuple(pts[0])]
        for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
            assert x0 == x1 or y0 == y1, (pts, "not axis-aligned")
            n = abs(x1 - x0) + abs(y1 - y0)
            dx, dy = np.sign(x1 - x0), np.sign(y1 - y0)
            cells += [(int(x0 + k * dx), int(y0 + k * dy)) for k in range(1, n + 1)]
        return self.carve(cells)

    def rect(self, x0, y0, x1, y1):
        """rows x0..x1 and columns y0..y1, carved"""
        return self.carve([(x, y) for x in range(x0, x1 + 1) for y in range(y0, y1 + 1)])

    def wall(self, cells):
        for x, y in cells:
            self.free[x, y] = False

    def grid(self):
        """the unpadded ground-truth grid: 1 free, -1 obstacle"""
        f = self.free
        assert not (f[0].any() or f[-1].any() or f[:, 0].any() or f[:, -1].any()), "the wall ring was carved"
        return np.where(f[1:-1, 1:-1], 1.0, -1.0)


def serpentine_cells(x0, y0, rows, cols):
    """The cells, in order, of a one-cell corridor that fills a box of ``rows`` x ``cols``
    cells at (x0, y0): along every other row, with a door at alternating ends of the wall
    rows between them.  ``rows`` is odd."""
    assert rows % 2 == 1
    cells = []
    for k in range(0, rows, 2):
        ys = range(y0, y0 + cols) if (k // 2) % 2 == 0 else range(y0 + cols - 1, y0 - 1, -1)
        cells += [(x0 + k, y) for y in ys]
        if k + 2 < rows:
            cells.append((x0 + k + 1, ys[-1]))
    return cells


def spiral_cells(x0, y0, rows, cols):
    """The cells, in order from the outer end to the centre, of a rectangular one-cell
    spiral in a box of ``rows`` x ``cols`` cells at (x0, y0): walk ahead while the cell two
    ahead is uncarved, else turn right."""
    done = np.zeros((rows, cols), dtype=bool)
    x, y, dx, dy = 0, 0, 0, 1
    done[0, 0] = True
    cells = [(x0, y0)]

    def open_(u, v):
        return 0 <= u < rows and 0 <= v < cols and not done[u, v]

    def blocked(u, v):
        return 0 <= u < rows and 0 <= v < cols and done[u, v]

    while True:
        for _ in range(2):
            if open_(x + dx, y + dy) and not blocked(x + 2 * dx, y + 2 * dy):
                break
            dx, dy = dy, -dx
        else:
            return cells
        x, y = x + dx, y + dy
        done[x, y] = True
        cells.append((x0 + x, y0 + y))


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
@dataclass
class Agent:
    """One (env, agent) item and what it was authored for (None: nothing declared)."""
    start: tuple            # padded cell
    unknown: list           # padded cells this agent has not explored
    d: int = None           # d*: the cost of the end point; -1: no reachable unexplored cell
    end: tuple = None       # the end point, padded
    loser: tuple = None     # fork: the unexplored cell that must not be chosen
    loser_cost: int = None  # ... and its BFS cost
    l1_max: int = None      # detour: the L1 distance from the start to the end is at most this
    min_paths: int = None   # tie families: at least this many shortest paths reach the end
    last_layer: int = None  # die-out: the last non-empty BFS layer of the sealed chamber
    lists: bool = None      # window_lists


@dataclass
class Case:
    """One env: a grid and its agents."""
    name: str
    canvas: Canvas
    agents: list
    notes: dict = field(default_factory=dict)

    @property
    def grid(self):
        return self.canvas.grid()

    @property
    def shape(self):
        return self.canvas.free.shape

    @property
    def starts(self):
        return np.array([a.start for a in self.agents], dtype=np.int32)


def case_planes(case):
    """(free, obst) uint8 [N, Wp, Lp] of a case: all but each agent's unknown cells."""
    gfree = case.canvas.free
    N = len(case.agents)
    free = np.zeros((N,) + gfree.shape, dtype=np.uint8)
    obst = np.zeros_like(free)
    for i, a in enumerate(case.agents):
        known = np.ones(gfree.shape, dtype=bool)
        for x, y in a.unknown:
            known[x, y] = False
        free[i] = gfree & known
        obst[i] = ~gfree & known
    return free, obst


def batch_state(cases):
    """The dense planes and counters of a batch of cases, as the env itself would have left
    them (test_gpu_dijkstra_big.inject_diamonds): free, obst [B, N, Wp, Lp], vis [B, Wp, Lp],
    free_cnt, vis_cnt [B], pos [B, N, 2]."""
    planes = [case_planes(c) for c in cases]
    free = np.stack([p[0] for p in planes])
    obst = np.stack([p[1] for p in planes])
    vis = free.max(axis=1)
    B = len(cases)
    return {"free": free, "obst": obst, "vis": vis, "free_cnt": free.reshape(B, -1).sum(1).astype(np.int32),
            "vis_cnt": vis.reshape(B, -1).sum(1).astype(np.int32), "pos": np.stack([c.starts for c in cases])}


def oracle_for(case, cfg):
    """the oracle env of a case: the authored planes, robots at the starts, step 0 (as
    oracle_from_device builds it from the device's state)"""
    free, obst = case_planes(case)
    neg = (~case.canvas.free).astype(np.uint8)
    st = {"env_grid": np.array([0]), "neg": neg[None], "pos_plane": (1 - neg)[None],
          "pos": case.starts[None], "moved": np.array([0], dtype=np.uint64),
          "free": free[None], "obst": obst[None], "vis": free.max(axis=0)[None], "currstep": np.array([0]),
          "done_thresh": np.array([float(cfg["done_thresh"])])}
    return oracle_from_device(st, 0, cfg)


# ---------------------------------------------------------------------------
# host predictors (g: the planning map, 1 explored, 0 unexplored, -1 obstacle)
# ---------------------------------------------------------------------------
def bfs_layers(g, sx, sy, stop_at_target=True):
    """The BFS layers over cells != -1 from the start: a list of lists of cells, layer 0
    first.  With ``stop_at_target`` the first layer that holds a 0-cell is the last."""
    h, w = g.shape
    seen = np.zeros(g.shape, dtype=bool)
    seen[sx, sy] = True
    layers = [[(sx, sy)]]
    while True:
        if stop_at_target and any(g[c] == 0 for c in layers[-1]):
            return layers
        nxt = []
        for x, y in layers[-1]:
            for (dx, dy), _ in STEPS:
                nx, ny = x + dx, y + dy
                if 0 <= nx < h and 0 <= ny < w and not seen[nx, ny] and g[nx, ny] != -1:
                    seen[nx, ny] = True
                    nxt.append((nx, ny))
        if not nxt:
            return layers
        layers.append(nxt)


def window_lists(g, sx, sy, depth=WINDOW_DEPTH):
    """True when dijkstra_window appends the item to the list of the full kernel: the start
    is not a target, layers 1..depth hold no 0-cell, and layer ``depth`` is non-empty."""
    layers = bfs_layers(g, sx, sy)
    if any(g[c] == 0 for c in layers[-1]):  # a target at cost len(layers) - 1
        return len(layers) - 1 > depth
    return len(layers) - 1 >= depth  # died out: the last non-empty layer


def cost_map(g, sx, sy):
    """BFS cost of every cell up to the end point's layer (-1: not reached)"""
    cost = -np.ones(g.shape, dtype=np.int64)
    for j, layer in enumerate(bfs_layers(g, sx, sy)):
        for c in layer:
            cost[c] = j
    return cost


def count_shortest_paths(g, sx, sy, end):
    """the number of shortest paths from the start to ``end``: a DP over the BFS costs"""
    layers = bfs_layers(g, sx, sy)
    cost = cost_map(g, sx, sy)
    ways = np.zeros(g.shape, dtype=object)
    ways[sx, sy] = 1
    h, w = g.shape
    for j, layer in enumerate(layers[1:], start=1):
        for x, y in layer:
            ways[x, y] = sum(ways[x + dx, y + dy] for (dx, dy), _ in STEPS
                             if 0 <= x + dx < h and 0 <= y + dy < w and cost[x + dx, y + dy] == j - 1)
    return int(ways[end])


def walk_ties(g, sx, sy, end):
    """The walk back from ``end``: at each cell the neighbours whose cost is one less, in
    the reference's order; the first is taken.  Returns (chosen, won, lost): the directions
    taken at all, taken where two or more were valid, and valid but not taken."""
    cost = cost_map(g, sx, sy)
    h, w = g.shape
    chosen, won, lost = set(), set(), set()
    x, y = end
    while (x, y) != (sx, sy):
        ok = [k for k, ((dx, dy), _) in enumerate(STEPS)
              if 0 <= x + dx < h and 0 <= y + dy < w and cost[x + dx, y + dy] == cost[x, y] - 1]
        chosen.add(DIR_NAMES[ok[0]])
        if len(ok) > 1:
            won.add(DIR_NAMES[ok[0]])
            lost.update(DIR_NAMES[k] for k in ok[1:])
        (dx, dy), _ = STEPS[ok[0]]
        x, y = x + dx, y + dy
    return chosen, won, lost


# ---------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------
# Detour: a three-corridor serpentine of 5 x 18 cells, corridors on padded rows 1, 3 and 5,
# the doors at (2, 18) and (4, 1).  A robot in one corridor, its unknown cell in the next,
# `off` columns nearer the door: L1 = 2 + off, d* = 2 k + 2 - off for a robot k columns
# from the door's.  (d*, off, k) per agent; every d* of 18..29.
DETOUR = {
    "detour_down": ((1, 3, 18), [(20, 0, 9), (21, 1, 10), (22, 2, 11), (23, 3, 12)]),
    "detour_up": ((3, 1, 18), [(24, 4, 13), (25, 1, 12), (28, 2, 14), (18, 0, 8)]),
    "detour_left_door": ((3, 5, 1), [(26, 0, 12), (27, 3, 14), (19, 1, 9), (29, 3, 15)]),
}
DETOUR_D = set(range(18, 30))


def detour_cases():
    out = []
    for name, ((row, trow, door), items) in DETOUR.items():
        cv = Canvas(7, 20)
        cv.carve(serpentine_cells(1, 1, 5, 18))
        away = -1 if door == 18 else 1  # from the door along the corridor
        agents = []
        for d, off, k in items:
            assert d == 2 * k + 2 - off
            agents.append(Agent((row, door + away * k), [(trow, door + away * (k - off))], d=d,
                                end=(trow, door + away * (k - off)), l1_max=6, lists=d > WINDOW_DEPTH))
        out.append(Case(name, cv, agents))
    return out


# Long winding paths on 61 x 70 cells: d* many times either side of the map.
LONG_D = {"serpentine": (50, 300, 2196), "spiral_inwards": (51, 299, 1000), "spiral_outwards": (49, 301, 1500)}


def long_cases():
    out = []
    for name, ds in LONG_D.items():
        cv = Canvas(63, 72)
        cells = cv.carve(serpentine_cells(1, 1, 61, 70) if name == "serpentine" else spiral_cells(1, 1, 61, 70))
        if name == "spiral_outwards":
            cells = cells[::-1]
        # robots on the corridor's first three cells, each one's unknown cell d* further along
        agents = [Agent(cells[i], [cells[i + d]], d=d, end=cells[i + d], min_paths=1, lists=True)
                  for i, d in enumerate(ds)]
        out.append(Case("long_" + name, cv, agents, notes={"corridor": len(cells)}))
    return out


# End-point ties: forks with a stem of s cells and two branches, on 44 x 48 cells.
#   x      stem along +y, branches along -x and +x: the ends differ in x
#   far    the same with the -x branch one cell longer: the smaller cell is a layer farther
#   y      stem along +x, branches along -y and +y: the ends have equal x
#   hook   x with each branch turned by 2 cells at its end, the -x one towards +y and the
#          +x one towards -y: the winner has the smaller x and the larger y
# total: the winner's cost, on both sides of the window's 24 layers.
FORK_TOTALS = {"short": 11, "at24": 24, "at25": 25, "long": 28}


def fork_cases():
    out = []
    for name, total in FORK_TOTALS.items():
        b = 5 if name == "short" else 8
        cv = Canvas(46, 50)
        agents = []

        def add(start, junction, end_a, end_b, mid_a=None, mid_b=None, loser_cost=total):
            cv.path(start, junction)
            cv.path(*(p for p in (junction, mid_a, end_a) if p is not None))
            cv.path(*(p for p in (junction, mid_b, end_b) if p is not None))
            win, lose = (end_a, end_b) if loser_cost == total else (end_b, end_a)
            agents.append(Agent(start, [end_a, end_b], d=total, end=win, loser=lose, loser_cost=loser_cost,
                                min_paths=1, lists=total > WINDOW_DEPTH))

        s = total - b
        x, y = 1 + b, 1  # x
        add((x, y), (x, y + s), (x - b, y + s), (x + b, y + s))
        x, y = 2 + b, 25  # far: the -x end is (x, y)-smaller and costs one more
        add((x, y), (x, y + s), (x - b - 1, y + s), (x + b, y + s), loser_cost=total + 1)
        x, y = 22, 1 + b  # y
        add((x, y), (x + s, y), (x + s, y - b), (x + s, y + b))
        s, x, y = total - b - 2, 22 + b, 22  # hook
        add((x, y), (x, y + s), (x - b, y + s + 2), (x + b, y + s - 2), (x - b, y + s), (x + b, y + s))
        out.append(Case("fork_" + name, cv, agents))
    return out


# Walk-back ties on 22 x 26 cells, four structures per env; `flips` mirror a structure in
# x and / or y, so every direction is somewhere the first valid neighbour and somewhere not.
def _flip(cells, box, fx, fy):
    (x0, y0), (h, w) = box
    return [((2 * x0 + h - 1 - x) if fx else x, (2 * y0 + w - 1 - y) if fy else y) for x, y in cells]


WALK_BOXES = [((1, 1), (9, 10)), ((1, 13), (9, 10)), ((12, 1), (9, 10)), ((12, 13), (9, 10))]
WALK_FLIPS = [(False, False), (False, True), (True, False), (True, True)]


def walk_cases():
    out = []

    def room(x0, y0):  # an open room of 4 x 7 cells, corner to corner: 84 paths
        return [(x, y) for x in range(x0, x0 + 4) for y in range(y0, y0 + 7)], (x0, y0), (x0 + 3, y0 + 6), 9, 84

    def ring(x0, y0):  # a ring corridor of 5 x 8 cells, corner to corner: 2 paths
        cells = [(x, y) for x in range(x0, x0 + 5) for y in range(y0, y0 + 8)
                 if x in (x0, x0 + 4) or y in (y0, y0 + 7)]
        return cells, (x0, y0), (x0 + 4, y0 + 7), 11, 2

    def ring_x(x0, y0):  # a ring of 7 x 6 from the middle of one column to the middle of the other
        cells = [(x, y) for x in range(x0, x0 + 7) for y in range(y0, y0 + 6)
                 if x in (x0, x0 + 6) or y in (y0, y0 + 5)]
        return cells, (x0 + 3, y0), (x0 + 3, y0 + 5), 11, 2

    def ring_y(x0, y0):  # a ring of 6 x 7 from the middle of one row to the middle of the other
        cells = [(x, y) for x in range(x0, x0 + 6) for y in range(y0, y0 + 7)
                 if x in (x0, x0 + 5) or y in (y0, y0 + 6)]
        return cells, (x0, y0 + 3), (x0 + 5, y0 + 3), 11, 2

    def bend(x0, y0):  # a 2-wide corridor with a bend: along 2 rows, then down 2 columns: 57 paths
        cells = [(x, y) for x in range(x0, x0 + 8) for y in range(y0, y0 + 9)
                 if x < x0 + 2 or y >= y0 + 7]
        return cells, (x0, y0), (x0 + 7, y0 + 8), 15, 57

    def tall(x0, y0):  # a room of 7 x 4 cells
        return [(x, y) for x in range(x0, x0 + 7) for y in range(y0, y0 + 4)], (x0, y0), (x0 + 6, y0 + 3), 9, 84

    envs = {"walk_rooms": [room] * 4, "walk_rings": [ring] * 4, "walk_mixed": [ring_x, ring_y, bend, tall]}
    for name, shapes in envs.items():
        cv = Canvas(22, 26)
        agents = []
        for shape, box, (fx, fy) in zip(shapes, WALK_BOXES, WALK_FLIPS):
            cells, start, end, d, paths = shape(*box[0])
            cells, (start, end) = _flip(cells, box, fx, fy), _flip([start, end], box, fx, fy)
            cv.carve(cells)
            agents.append(Agent(start, [end], d=d, end=end, min_paths=paths, lists=False))
        out.append(Case(name, cv, agents))
    return out


# Die-out: sealed one-cell chambers whose last BFS layer is k, the robot at one end; the
# unknown cells (a free pocket and a wall cell) lie outside.  Both sides of the window
# kernel's trips of three layers and of its list decision at layer 24.
DIEOUT_LAYERS = {"dieout_window": (1, 5, 23), "dieout_listed": (24, 25, 26)}


def dieout_cases():
    out = []
    for name, ks in DIEOUT_LAYERS.items():
        cv = Canvas(12, 34)
        cv.carve([(10, 5)])  # the pocket no chamber reaches
        agents = []
        for n, k in enumerate(ks):
            cells = cv.carve(serpentine_cells(1, 1 + 11 * n, 7, 9)[:k + 1])
            agents.append(Agent(cells[0], [(10, 5), (10, 7)], d=-1, last_layer=k, lists=k >= WINDOW_DEPTH))
        out.append(Case(name, cv, agents))
    return out


# Ring and border targets on 24 x 28 cells: the interior fully explored but for one
# wall-ring cell.  A fence one cell inside the outermost free cells (rows 2 and 23 over
# columns 4..25, columns 2 and 27 over rows 4..21: open at its four corners) makes the
# detours; the rest is open floor, so most ends are reached by very many shortest paths.
BORDER_D = {"border_sides": (25, 21, 25, 21), "border_corners": (25, 25, 25, 25),
            "border_corner_tile": (7, 7, 3, 3), "border_corner_tile_far": (45, 45, 49, 49)}


def border_cases():
    Wp, Lp = 26, 30
    out = []

    def canvas():
        cv = Canvas(Wp, Lp)
        cv.rect(1, 1, Wp - 2, Lp - 2)
        cv.wall([(x, y) for x in (2, Wp - 3) for y in range(4, Lp - 4)])
        cv.wall([(x, y) for y in (2, Lp - 3) for x in range(4, Wp - 4)])
        return cv

    # the ring cells beside the four corners' free cells, each with the corner cell itself
    # (which no path reaches: its neighbours are known walls)
    corner = [[(0, 1), (0, 0)], [(1, Lp - 1), (0, Lp - 1)], [(Wp - 2, 0), (Wp - 1, 0)],
              [(Wp - 1, Lp - 2), (Wp - 1, Lp - 1)]]
    sides = [[(0, 14)], [(13, Lp - 1)], [(Wp - 1, 15)], [(12, 0)]]
    inner = [(3, 14), (13, Lp - 4), (Wp - 4, 15), (12, 3)]  # beside the fence, 3 cells from the target
    mid = [(12, 14), (12, 15), (13, 14), (13, 15)]
    tile = [(4, 4), (4, Lp - 5), (Wp - 2, 3), (Wp - 2, Lp - 4)]  # in the four corner tiles
    specs = {"border_sides": (inner, sides, 3), "border_corners": (mid, corner, None),
             "border_corner_tile": (tile, corner, None), "border_corner_tile_far": (tile, corner[::-1], None)}
    for s in tile:  # the window kernel's 8 x 8 tiles around these reach 4 tiles past the map
        assert s[0] >> 3 in (0, (Wp - 1) >> 3) and s[1] >> 3 in (0, (Lp - 1) >> 3)
    for name, (starts, unknown, l1) in specs.items():
        agents = [Agent(s, u, d=d, end=u[0], l1_max=l1, lists=d > WINDOW_DEPTH)
                  for s, u, d in zip(starts, unknown, BORDER_D[name])]
        out.append(Case(name, canvas(), agents))
    return out


# Word boundaries: corridors on the extended columns b | b + 1 (b = 63 or 127), which are
# the padded columns c0 = b - pad and c1 = c0 + 1, on 34 rows:
#   turn_lo   down column c0, then along +y across the boundary: the walk back turns on c0
#   straight  one row from column 2 to column Lp - 3, across every boundary
#   turn_hi   down column c1, then along -y across the boundary: the walk back turns on c1
#   wide      a 2-wide corridor on c0 | c1, corner to corner: ties across the boundary
# (name, RY, boundary): RY = Lp + 2 pad extended columns.
WORD_SHAPES = [("words_ry128", 128, 63), ("words_ry129", 129, 63), ("words_three", None, 127)]


def word_case(name, ego):
    ry, b = {n: (r, bb) for n, r, bb in WORD_SHAPES}[name]
    Lp = 140 if ry is None else ry - 2 * ego
    c0 = b - ego
    c1 = c0 + 1
    assert 6 <= c0 and c1 + 5 <= Lp - 2
    cv = Canvas(36, Lp)
    agents = []
    p = cv.path((1, c0), (9, c0), (9, c1 + 4))
    agents.append(Agent(p[0], [p[-1]], d=13, end=p[-1], min_paths=1, lists=False))
    p = cv.path((11, 2), (11, Lp - 3))
    agents.append(Agent(p[0], [p[-1]], d=Lp - 5, end=p[-1], min_paths=1, lists=True))
    p = cv.path((13, c1), (21, c1), (21, c0 - 4))
    agents.append(Agent(p[0], [p[-1]], d=13, end=p[-1], min_paths=1, lists=False))
    cv.rect(23, c0, 33, c1)
    agents.append(Agent((23, c0), [(33, c1)], d=11, end=(33, c1), min_paths=11, lists=False))
    return Case(name, cv, agents, notes={"ego": ego, "RY": Lp + 2 * ego, "boundary": b, "c0": c0})


# Start on a target and the target adjacent, in a serpentine of 9 x 12 cells (corridors
# on rows 1, 3, ..., doors at (2, 12), (4, 1), (6, 12), (8, 1)); every agent also has a far
# unknown cell that must not matter.
def near_cases():
    far = (9, 12)

    def case(name, items):
        cv = Canvas(11, 14)
        cv.carve(serpentine_cells(1, 1, 9, 12))
        return Case(name, cv, [Agent(s, list(u) + [far], d=d, end=e, lists=False) for s, u, d, e in items])

    return [
        case("near_a", [((3, 6), [(3, 6)], 0, (3, 6)),            # its own cell
                        ((1, 12), [(2, 12)], 1, (2, 12)),         # +x: the door below
                        ((3, 12), [(2, 12)], 1, (2, 12))]),       # -x: the door above
        case("near_b", [((5, 6), [(5, 7)], 1, (5, 7)),            # +y
                        ((7, 6), [(7, 5)], 1, (7, 5)),            # -y
                        ((3, 1), [(4, 1), (3, 2)], 1, (3, 2))]),  # +x and +y unknown: (3, 2) < (4, 1)
        case("near_c", [((1, 5), [(1, 4), (1, 6)], 1, (1, 4)),    # -y and +y unknown: the smaller y
                        ((5, 1), [(4, 1), (5, 2)], 1, (4, 1)),    # -x and +y unknown: the smaller x
                        ((7, 12), [(6, 12), (8, 12), (7, 11)], 1, (6, 12))]),
    ]


FAMILIES = ("detour", "long", "fork", "walk", "dieout", "border", "near", "words_ry128", "words_ry129",
            "words_three")


@functools.lru_cache(maxsize=None)
def family(name, ego=2):
    """The cases (envs) of one batch: one grid shape, one N.  Only the word families depend
    on the egoradius (their corridors sit on fixed extended columns)."""
    if name.startswith("words_"):
        return (word_case(name, ego),)
    return tuple({"detour": detour_cases, "long": long_cases, "fork": fork_cases, "walk": walk_cases,
                  "dieout": dieout_cases, "border": border_cases, "near": near_cases}[name]())


def planning_map(case, i, ego):
    """(g, sx, sy) of agent i at egoradius ``ego``: the oracle's free_pad - obst_pad and
    start cell, built from the planes alone"""
    free, obst = case_planes(case)
    g = np.pad(free[i].astype(np.float64) - obst[i], ego)
    return g, case.agents[i].start[0] + ego, case.agents[i].start[1] + ego


# ---------------------------------------------------------------------------
# closed loop: the greedy follower on mazes of 19 x 23 cells
# ---------------------------------------------------------------------------
LOOP_SHAPE = (19, 23)
LOOP_STARTS = {1: [(1, 1)], 3: [(1, 1), (1, 2), (1, 3)]}
# steps the oracle-driven loop takes to 100 % coverage (measured once on the CPU reference
# by test_dijkstra_maze_cases_cpu.py, which asserts them again; never taken from the device)
LOOP_STEPS = {("serpentine", 1): 235, ("serpentine", 3): 76, ("spiral", 1): 235, ("spiral", 3): 76}


def loop_cfg(n):
    return base_cfg(numrobot=n, maxsteps=1000, sensor_config={"num_lasers": 9, "range": 3})


def loop_grid(kind):
    cv = Canvas(LOOP_SHAPE[0] + 2, LOOP_SHAPE[1] + 2)
    cv.carve((serpentine_cells if kind == "serpentine" else spiral_cells)(1, 1, *LOOP_SHAPE))
    return cv.grid()


def loop_oracle(kind, n):
    """the oracle env of a closed-loop run at its start: a reset with the robots on the
    corridor's first cells"""
    from oracle.cpu_ref import DecGridRLRef
    np.random.seed(0)
    ref = DecGridRLRef([loop_grid(kind)], loop_cfg(n))
    ref.reset(False, None, positions=LOOP_STARTS[n])
    return ref

"""Authored maps and scripted walks that force each incremental path of
dist_reward's distance layer (csrc/mc_dist.hip, the env kernel's witness and
window rules in csrc/mc_env_step.h), and a predictor of the path every map
takes per step.  Pure NumPy plus oracle/: test_dist_cache_cases_cpu.py shows
on the oracle alone that every scenario holds the phases it is meant to hold,
test_gpu_dist_cache.py runs the scenarios on the device beside the oracle.

Coordinates.  A grid of W x L cells becomes a padded plane of Wp x Lp = (W +
2) x (L + 2) cells (an obstacle ring, never covered; the device's map, robot
and witness coordinates) and an extended plane of (Wp + 2 pad) x (Lp + 2 pad)
(the oracle's ``_free_pad``; extended = padded + pad).  The distance field is
taken over the extended plane, so an uncovered square of s x s grid cells in
a grid corner is an uncovered (s + pad + 1)^2 corner of the field, and its
max(d) is s + 2 (pad + 1), attained at the field's corner cell alone.

The rules the predictor restates ("The dist_reward
layer"), per map and step:

  listed   M is unknown; or a newly covered cell is closer than M to the
           witness (bits_within); or a target -- the 5 end cells at the quirk
           index, the E x E crop -- is not settled by the agent's staged block
           (dist_window: the block of 8 window_tiles(H) rows and columns whose
           origin is 8 floor((x0 - H - 1) / 8) at the cell x0 the robot stood
           on BEFORE its move; a target at distance b from the block's outside
           is settled iff a covered cell of the block is within b of it)
  served   listed, the cache valid, the box's tiles + 65 <= MC_FAST_TILES, the
           targets settled by the 40 x 40 block of cache_try, and the new
           max(d) >= M0 - kDistT
  full     listed and not served: M0 = the new max(d), valid = (the cells
           with d >= M0 - kDistT over the extended plane number <= kDistK)

The box is the union of the sensing windows [x - H, x + H] x [y - H, y + H]
of the steps since the map was last served or transformed (grown only while
the cache is valid), counted in 8 x 8 tiles of the padded plane.

  primed   the first step after an import (set_global_state) transforms every
           map of the handle before its env kernel, for the PRE terms, outside
           the work list and its counters: M0 = max(d), valid as after a full
           transform, the box empty, M and a witness known (MapPredictor.prime)
"""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass, field

import numpy as np

from gpu_util import oracle_from_device
from oracle.cpu_ref import l1_distance_to_covered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the build the geometry below was made for
GEOMETRY = {"K": 512, "T": 20, "FAST_TILES": 1024, "SPAN": 256, "STRIP": 32}
UP, DOWN, LEFT, RIGHT, STAY = 2, 0, 3, 1, 4  # action codes: -x, +x, -y, +y, no-op


def source_constants():
    """kDistK, kDistT, MC_FAST_TILES, kSpan and kStrip of the default build, read from the
    source (as test_gpu_dist_field.kernel_row_edges does)."""
    def src(name):
        return open(os.path.join(ROOT, "marl-coverage_amd", "csrc", name)).read()

    def num(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))

    internal, dist = src("mc_internal.h"), src("mc_dist.hip")
    return {"K": num(internal, r"#define MC_DIST_K (\d+)"), "T": num(internal, r"#define MC_DIST_T (\d+)"),
            "FAST_TILES": num(dist, r"#define MC_FAST_TILES (\d+)"), "SPAN": num(dist, r"constexpr int kSpan = (\d+);"),
            "STRIP": num(dist, r"constexpr int kStrip = (\d+);")}


def window_tiles(H):
    """mc_internal.h window_tiles: the staged block's tiles per side"""
    return (2 * H + 3 + 7 + 7) // 8


def sensing_half_width(cfg):
    """H as mc_create derives it: max(the sensor's reach, egoradius)"""
    sc = cfg["sensor_config"]
    hs = int(np.ceil(sc["range"])) if cfg["sensor_type"] == "lidar" else int(sc["range"])
    return max(hs, int(cfg["egoradius"]))


def base_cfg(**kw):
    """test_gpu_parity.base_cfg with dist_reward (restated: that module needs a GPU's imports)"""
    c = dict(numrobot=1, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0, terminal_reward=30,
             dist_reward=1, train_maxsteps=1000, test_maxsteps=1000, egoradius=2, mini_map_rad=0, comm_radius=0,
             allow_comm=0, map_sharing=0, single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
             sensor_config={"num_lasers": 21, "range": 10})
    c.update(kw)
    return c


def square_cfg(n, **kw):
    """egoradius 2, pad 2, the square sensor of range 1 that covers the robot's own cell only"""
    c = dict(numrobot=n, sensor_type="square_sensor", sensor_config={"range": 1}, single_square_tool=1)
    c.update(kw)
    return base_cfg(**c)


# ---------------------------------------------------------------------------
# the predictor
# ---------------------------------------------------------------------------
def targets(px, py, pad, ego):
    """the targets of a robot at the padded cell (px, py), padded coordinates: the 5 end
    cells of the next step at the quirk index, then the E x E crop (cache_try's target_cell)"""
    out = [(px + dx - pad, py + dy - pad) for dx, dy in ((0, 0), (1, 0), (0, 1), (-1, 0), (0, -1))]
    out += [(px - ego + r, py - ego + c) for r in range(2 * ego + 1) for c in range(2 * ego + 1)]
    return np.array(out, dtype=np.int64)


def block_unsettled(free_ext, pad, x0, y0, size, tg):
    """True if a target of ``tg`` is not settled by the block of size x size padded cells at
    (x0, y0): it lies outside the block, or no covered cell of the block is within b of it,
    b its distance to the block's outside (dist_window / cache_try's target loop)"""
    lx, ly = tg[:, 0] - x0, tg[:, 1] - y0
    b = np.minimum(np.minimum(lx, size - 1 - lx), np.minimum(ly, size - 1 - ly)) + 1
    if (b <= 0).any():
        return True
    r0, r1 = max(x0 + pad, 0), min(x0 + pad + size, free_ext.shape[0])
    c0, c1 = max(y0 + pad, 0), min(y0 + pad + size, free_ext.shape[1])
    cov = np.argwhere(free_ext[r0:r1, c0:c1] > 0)
    if not len(cov):
        return True
    cov = cov + (r0 - pad, c0 - pad)  # padded coordinates
    d = (np.abs(cov[None, :, 0] - tg[:, None, 0]) + np.abs(cov[None, :, 1] - tg[:, None, 1])).min(axis=1)
    return bool((d > b).any())


def pick_witness(d, px, py, pad):
    """A stand-in for the device's witness where no device is at hand: of the cells with
    d == max(d), the one farthest from the robot (padded coordinates)"""
    cells = np.argwhere(d == d.max()) - pad
    far = np.abs(cells[:, 0] - px) + np.abs(cells[:, 1] - py)
    return tuple(int(v) for v in cells[int(np.argmax(far))])


@dataclass
class StepPath:
    """what one map did in one step"""
    listed: bool = False
    hit: bool = False        # the witness rule listed it
    unsettled: bool = False  # a target the staged block left open listed it
    served: bool = False
    full: bool = False
    had_cache: bool = False  # a full transform of a map whose cache was valid (theta0 from the try)
    tried: bool = False
    box: tuple = None        # the box of the try: (x0, y0, x1, y1), padded cells
    box_tiles: tuple = (0, 0)  # its tile rows and columns
    new_max: int = -1
    top: int = 0             # after a full transform: cells with d >= M0 - T
    top_strips: int = 0      # and the strips of kStrip columns they lie in
    valid: bool = False      # the cache after the step


class MapPredictor:
    """The state machine of one map (module docstring)."""

    def __init__(self, consts, cfg):
        self.c = consts
        self.pad = max(int(cfg["egoradius"]), int(cfg["mini_map_rad"]))
        self.ego = int(cfg["egoradius"])
        self.H = sensing_half_width(cfg)
        self.valid = False
        self.M0 = -1
        self.box = None

    def void(self):
        """a reset or an import: the cache is dropped"""
        self.valid, self.box = False, None

    def copy_from(self, other):
        self.valid, self.M0, self.box = other.valid, other.M0, other.box

    def prime(self, free):
        """The transform of every map that the first step after an import (or any state
        upload) runs before its env kernel, for the PRE terms: M and the witness become
        known and the cache is taken, no counter moves.  Returns its StepPath."""
        out = StepPath(full=True)
        self.box = None
        covered = bool((free > 0).any())
        d = l1_distance_to_covered(free) if covered else None
        out.new_max = self.M0 = int(d.max()) if covered else -1
        if covered:
            top = np.argwhere(d >= self.M0 - self.c["T"])
            out.top, out.top_strips = len(top), len(set((top[:, 1] // self.c["STRIP"]).tolist()))
        out.valid = self.valid = covered and 0 < out.top <= self.c["K"]
        return out

    def step(self, M, witness, pos0, pos1, free_before, free_after):
        """One step of the map.  ``M``, ``witness``: the device's (or the stand-in's) max(d)
        and witness cell (padded) before the step, M < 0: unknown; ``pos0`` / ``pos1``: the
        robot's padded cell before / after its move; ``free_*``: the extended free plane."""
        c, pad, H = self.c, self.pad, self.H
        out = StepPath()
        new = np.argwhere((free_after > 0) & (free_before == 0)) - pad
        if M > 0 and len(new):
            out.hit = bool(((np.abs(new[:, 0] - witness[0]) + np.abs(new[:, 1] - witness[1])) < M).any())
        tg = targets(pos1[0], pos1[1], pad, self.ego)
        if M >= 0 and not out.hit:
            bx, by = 8 * ((pos0[0] - H - 1) // 8), 8 * ((pos0[1] - H - 1) // 8)
            out.unsettled = block_unsettled(free_after, pad, bx, by, 8 * window_tiles(H), tg)
        out.listed = M < 0 or out.hit or out.unsettled
        if self.valid:
            w = (pos1[0] - H, pos1[1] - H, pos1[0] + H, pos1[1] + H)
            b = self.box
            self.box = w if b is None else (min(b[0], w[0]), min(b[1], w[1]), max(b[2], w[2]), max(b[3], w[3]))
        out.valid = self.valid
        if not out.listed:
            return out
        covered = bool((free_after > 0).any())
        d = l1_distance_to_covered(free_after) if covered else None
        out.new_max = int(d.max()) if covered else -1
        if self.valid:
            b = self.box
            out.box = b
            out.box_tiles = (b[2] // 8 - b[0] // 8 + 1, b[3] // 8 - b[1] // 8 + 1)
            out.tried = out.box_tiles[0] * out.box_tiles[1] + 25 + 40 <= c["FAST_TILES"]
        if out.tried:
            # cache_try's 40 x 40 block: the 5 x 5 tiles around the targets' bounding box
            e = self.ego
            tx = (min(pos1[0] - pad - 1, pos1[0] - e) + max(pos1[0] - pad + 1, pos1[0] + e)) >> 1
            ty = (min(pos1[1] - pad - 1, pos1[1] - e) + max(pos1[1] - pad + 1, pos1[1] + e)) >> 1
            settled = not block_unsettled(free_after, pad, 8 * ((tx >> 3) - 2), 8 * ((ty >> 3) - 2), 40, tg)
            out.served = settled and out.new_max >= self.M0 - c["T"]
        self.box = None
        if not out.served:
            out.full, out.had_cache = True, self.valid
            self.M0 = out.new_max
            if covered:
                top = np.argwhere(d >= self.M0 - c["T"])
                out.top = len(top)
                out.top_strips = len(set((top[:, 1] // c["STRIP"]).tolist()))
            self.valid = covered and 0 < out.top <= c["K"]
        out.valid = self.valid
        return out


# ---------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------
@dataclass
class Scenario:
    name: str
    W: int                 # the unpadded grid (all free)
    L: int
    cfg: dict
    planes: np.ndarray     # uint8 [N, Wp, Lp]: the authored free plane of every agent
    starts: np.ndarray     # int32 [N, 2] padded cells
    script: np.ndarray     # uint8 [steps, N] action codes
    roles: tuple = ()
    notes: dict = field(default_factory=dict)

    @property
    def N(self):
        return len(self.starts)


def walk(start, legs):
    """the cells and action codes of a walk: ``legs`` is a sequence of (codes, moves), the
    codes cycled for that many moves"""
    delta = {DOWN: (1, 0), RIGHT: (0, 1), UP: (-1, 0), LEFT: (0, -1), STAY: (0, 0)}
    x, y = start
    cells, acts = [(x, y)], []
    for codes, moves in legs:
        for k in range(moves):
            a = codes[k % len(codes)]
            x, y = x + delta[a][0], y + delta[a][1]
            acts.append(a)
            cells.append((x, y))
    return cells, acts


def _swap(script, a, b):
    """action codes a and b exchanged"""
    lut = np.arange(5, dtype=np.uint8)
    lut[a], lut[b] = b, a
    return lut[script]


def build(name, W, L, cfg, plane, agents, steps=None, mirror=False, flip=False, transpose=False, **notes):
    """``agents``: (role, start, legs, [own plane]) per agent; every walk is padded with
    no-ops to the longest (or cut to ``steps``).  ``mirror`` flips the columns of planes
    and walks, ``flip`` their rows, ``transpose`` then swaps rows and columns: the planes
    are authored with their holes in the first rows and columns, where the coordinates are
    short, and most are run flipped (a walk towards larger rows and columns keeps its
    targets inside the staged block on covered ground; towards smaller ones the target
    x - pad - 1 leaves the block every 8th move).  Asserts that the walks stay on the
    grid and never meet (a refused move would leave the script)."""
    Wp, Lp = W + 2, L + 2
    paths, acts, planes = [], [], []
    for ag in agents:
        cells, a = walk(ag[1], ag[2])
        paths.append(cells)
        acts.append(a)
        planes.append(ag[3] if len(ag) > 3 else plane)
    T = max(len(a) for a in acts) if steps is None else steps
    for cells, a in zip(paths, acts):
        del a[T:], cells[T + 1:]
        cells += [cells[-1]] * (T + 1 - len(cells))
        a += [STAY] * (T - len(a))
    for t in range(T + 1):
        now = [p[t] for p in paths]
        assert len(set(now)) == len(now), (name, "two robots on one cell at move", t)
        assert all(1 <= x <= Wp - 2 and 1 <= y <= Lp - 2 for x, y in now), (name, "off the grid at move", t)
    # robots move in turn: none may enter the cell another leaves in the same step
    for t in range(T):
        before = {p[t] for p in paths}
        for p in paths:
            assert p[t + 1] == p[t] or p[t + 1] not in before, (name, "a move into an occupied cell at", t)
    planes = np.stack(planes).astype(np.uint8)
    starts = np.array([p[0] for p in paths], dtype=np.int32)
    script = np.array(acts, dtype=np.uint8).T.reshape(T, len(agents))
    if mirror:
        planes = planes[:, :, ::-1].copy()
        starts[:, 1] = Lp - 1 - starts[:, 1]
        script = _swap(script, RIGHT, LEFT)
    if flip:
        planes = planes[:, ::-1, :].copy()
        starts[:, 0] = Wp - 1 - starts[:, 0]
        script = _swap(script, UP, DOWN)
    if transpose:
        planes = planes.transpose(0, 2, 1).copy()
        starts = starts[:, ::-1].copy()
        swap = {DOWN: RIGHT, RIGHT: DOWN, UP: LEFT, LEFT: UP, STAY: STAY}
        script = np.vectorize(swap.get)(script).astype(np.uint8)
        W, L = L, W
    assert planes.shape[1:] == (W + 2, L + 2)
    return Scenario(name, W, L, cfg, planes, starts, script, tuple(ag[0] for ag in agents), notes)


def holes_plane(W, L, holes):
    """everything covered but the given (rows, columns) slices of padded cells"""
    f = np.zeros((W + 2, L + 2), dtype=np.uint8)
    f[1:-1, 1:-1] = 1
    for rows, cols in holes:
        f[rows, cols] = 0
    return f


AW, AL = 96, 200  # scenario A's grid: extended 102 x 206, 7 strips of 32 columns


def two_holes(left=48, right=74):
    """A's plane: uncovered squares of ``right`` cells in the top-right and of ``left``
    cells in the top-left corner"""
    Lp = AL + 2
    return holes_plane(AW, AL, [(slice(1, 1 + right), slice(Lp - 1 - right, Lp - 1)),
                                (slice(1, 1 + left), slice(1, 1 + left))])


def scenario_a(variant="a", steps=None):
    """Two holes, hand-over (test_gpu_dist_cache.py's docstring).  Authored with the holes
    in the first rows; run flipped (the walkers head for larger rows) but for ``upleft``,
    which mirrors the columns instead: its walkers head for smaller rows and columns, so
    every cached cell lies at lower coordinates than the box."""
    diag = [((UP, RIGHT), 148)]  # from beside the right hole's inner corner to the grid's corner (1, 200)
    parked = ("parked", (90, 100), [])
    if variant in ("a", "upleft"):
        # a: the diagonal walker goes on along the grid's edge row, 30 more unlisted moves
        agents = [("diagonal", (75, 126), diag + ([((LEFT,), 30)] if variant == "a" else [])), parked,
                  ("left_hole", (49, 49), [((UP, LEFT), 96)]),
                  ("top_row", (1, 126), [((RIGHT,), 73), ((DOWN,), 74)])]
        if variant == "a":
            return build("A", AW, AL, square_cfg(4), two_holes(), agents, steps, flip=True)
        return build("A-upleft", AW, AL, square_cfg(4), two_holes(), agents, steps, mirror=True)
    if variant in ("pair", "solo"):  # the lifecycle cases: the diagonal walker (and the parked robot)
        agents = [("diagonal", (75, 126), diag)] + ([parked] if variant == "pair" else [])
        return build("A-" + variant, AW, AL, square_cfg(len(agents)), two_holes(), agents, steps, flip=True)
    if variant == "gap":  # A': the left hole's max is 80 - T - 1
        agents = [("diagonal", (75, 126), diag), parked]
        return build("A'", AW, AL, square_cfg(2), two_holes(left=53), agents, steps, flip=True)
    if variant == "5x5":  # range 2, every cell of the 5 x 5 window: the new cells lie off the robot's cell
        cfg = square_cfg(2, sensor_config={"range": 2}, single_square_tool=0)
        # (it starts two cells further out: the first step's window must cover nothing new)
        agents = [("diagonal", (77, 124), [((UP, RIGHT), 152)]), parked]
        return build("A-5x5", AW, AL, cfg, two_holes(), agents, steps, flip=True)
    raise KeyError(variant)


def top_set(plane, pad, T):
    """(max d, the number of cells with d >= max d - T) of a padded free plane"""
    d = l1_distance_to_covered(np.pad(plane, pad))
    return int(d.max()), int((d >= d.max() - T).sum())


def rim_plane(h, w, k):
    """B's family: an uncovered h x w rectangle in the top-left corner of A's grid, with k
    covered cells on its last row, from the grid's edge"""
    f = holes_plane(AW, AL, [(slice(1, 1 + h), slice(1, 1 + w))])
    f[h, 1:1 + k] = 1
    return f


@functools.lru_cache(maxsize=None)
def overflow_pair(K=GEOMETRY["K"], T=GEOMETRY["T"], pad=2):
    """The two planes of rim_plane's family (30 rows) whose top sets are the largest <= K
    and the smallest > K: ((h, w, k, size), (h, w, k, size))."""
    below = above = None
    h = 30
    for w in range(h, h + 21, 2):
        for k in range(0, 16):
            n = top_set(rim_plane(h, w, k), pad, T)[1]
            if n <= K and (below is None or n > below[3]):
                below = (h, w, k, n)
            if n > K and (above is None or n < above[3]):
                above = (h, w, k, n)
    return below, above


def scenario_b(which, steps=None):
    """Overflow: top sets past kDistK leave the map without a cache."""
    if which == "column":  # one covered column: 1,848 cells within T of the max
        f = np.zeros((AW + 2, AL + 2), dtype=np.uint8)
        f[1:-1, 1] = 1
        agents = [("row_walker", (40, 1), [((RIGHT,), 40)]), ("column_walker", (60, 1), [((UP,), 40)])]
        return build("B-column", AW, AL, square_cfg(2), f, agents, steps)
    below, above = overflow_pair()
    h, w, k, n = below if which == "below" else above
    # the diagonal from beside the hole's inner corner towards the grid's corner
    agents = [("diagonal", (h + 1, w + 1), [((UP, LEFT), 2 * h), ((LEFT,), w - h)]), ("parked", (90, 100), [])]
    return build(f"B-{which}", AW, AL, square_cfg(2), rim_plane(h, w, k), agents, steps, top=n)


def scenario_c(transpose=False, steps=None):
    """A box taller than kSpan: 300 x 30 with a 24 x 24 hole at one end (authored in the
    first rows, run flipped).  The walker crosses 270 covered rows unlisted, its box
    growing, and enters the hole: the first try's box has more than kSpan rows."""
    W, L = 300, 30
    f = holes_plane(W, L, [(slice(1, 25), slice(1, 25))])
    agents = [("walker", (299, 10), [((UP,), 298)])]
    return build("C" + ("-transposed" if transpose else ""), W, L, square_cfg(1), f, agents, steps, flip=True,
                 transpose=transpose)


def scenario_d(which, steps=None):
    """A box past MC_FAST_TILES: 320 x 320 with a 60 x 60 hole in a corner (authored top
    left, run mirrored and flipped).  The walker goes along a row and then along a column
    into the hole, unlisted on covered ground; at its first listing the box is 32 x 32
    tiles (``over``: no try) or 30 x 31, the largest that fits (``fits``: 930 + 65 <= 1024
    < 31 x 31 + 65)."""
    W = L = 320
    f = holes_plane(W, L, [(slice(1, 61), slice(1, 61))])
    x0, y0, left, up = D_WALKS[which]
    agents = [("walker", (x0, y0), [((LEFT,), left), ((UP,), up)])]
    return build(f"D-{which}", W, L, square_cfg(1), f, agents, steps, mirror=True, flip=True)


# (start row, start column, moves along the row, moves along the column), authored.  Run,
# the walker enters the hole's first row at row 261 in column 291: the box ends in tile
# row 263 // 8 = 32 and tile column 293 // 8 = 36.  over: its first move ends at (10, 49), box from
# (8, 47): tile rows 1 .. 32, tile columns 5 .. 36.  fits: from (25, 65), box from (23,
# 63): tile rows 2 .. 32, tile columns 7 .. 36.  20 more moves inside the hole.
D_WALKS = {"over": (311, 273, 243, 271), "fits": (296, 257, 227, 256)}


def scenario_e(ego=2, steps=60):
    """pad > egoradius.  ego 2: mini_map_rad 7, the quirk targets sit 7 cells up-left of
    the robot; ego 3: pad 3, 54 targets (dist_window instead of its agent-major forms)."""
    cfg = square_cfg(3, mini_map_rad=7 if ego == 2 else 0, egoradius=ego)
    agents = [("diagonal", (75, 126), [((UP, RIGHT), 148)]), ("parked", (90, 100), []),
              ("top_row", (1, 126), [((RIGHT,), 73), ((DOWN,), 74)])]
    return build(f"E-ego{ego}", AW, AL, cfg, two_holes(), agents, steps, flip=True)


def scenario_f(steps=50):
    """The C5 instantiation: 16 agents, the base lidar, on A's plane.  The walkers start
    below both holes (right: columns 127 .. 200, rows 1 .. 74; left: 1 .. 48), more than
    the lidar's range away, and walk into them."""
    cfg = base_cfg(numrobot=16)
    agents = []
    for k in range(8):
        agents.append((f"right{k}", (86 + 2 * (k % 2), 120 + 9 * k), [((UP,), 36), ((RIGHT, UP), 30)]))
        agents.append((f"left{k}", (60 + 2 * (k % 2), 20 + 6 * k), [((UP,), 36), ((LEFT, UP), 30)]))
    return build("F", AW, AL, cfg, two_holes(), agents, steps, flip=True)


# ---------------------------------------------------------------------------
# the oracle alone
# ---------------------------------------------------------------------------
def oracle_for(scn):
    """the oracle env of a scenario at its start: the authored planes, robots at the
    starts, step 0 (as oracle_from_device builds it from the device's state)"""
    Wp, Lp = scn.W + 2, scn.L + 2
    neg = np.ones((Wp, Lp), dtype=np.uint8)
    neg[1:-1, 1:-1] = 0
    st = {"env_grid": np.array([0]), "neg": neg[None], "pos_plane": (1 - neg)[None],
          "pos": scn.starts[None].astype(np.int32), "moved": np.array([0], dtype=np.uint64),
          "free": scn.planes[None], "obst": np.zeros_like(scn.planes)[None],
          "vis": scn.planes.max(axis=0)[None], "currstep": np.array([0]),
          "done_thresh": np.array([float(scn.cfg["done_thresh"])])}
    return oracle_from_device(st, 0, scn.cfg)


def simulate(scn, consts=None, steps=None):
    """The scenario on the oracle alone, with pick_witness standing in for the device's
    witness: [steps + 2][N] StepPath, entry 0 the transform of the authored maps (prime),
    entry 1 the all-no-op first step, entry 1 + k move k."""
    consts = consts or GEOMETRY
    ref = oracle_for(scn)
    N, pad = scn.N, ref._pad
    pred = [MapPredictor(consts, scn.cfg) for _ in range(N)]
    out = [[q.prime(ref._free_pad[i]) for i, q in enumerate(pred)]]
    mw = [(out[0][i].new_max, pick_witness(l1_distance_to_covered(ref._free_pad[i]), int(ref._xinds[i]),
                                           int(ref._yinds[i]), pad)) for i in range(N)]
    script = np.concatenate([np.full((1, N), STAY, dtype=np.uint8), scn.script])
    for t, acts in enumerate(script[:None if steps is None else steps + 1]):
        before = ref._free_pad.copy()
        pos0 = [(int(ref._xinds[i]), int(ref._yinds[i])) for i in range(N)]
        ref.step(acts.astype(np.int64))  # (code 4 matches no move)
        row = []
        for i in range(N):
            pos1 = (int(ref._xinds[i]), int(ref._yinds[i]))
            p = pred[i].step(mw[i][0], mw[i][1], pos0[i], pos1, before[i], ref._free_pad[i])
            if p.listed:
                d = l1_distance_to_covered(ref._free_pad[i])
                mw[i] = (int(d.max()), pick_witness(d, pos1[0], pos1[1], pad))
            row.append(p)
        out.append(row)
    return out

"""What mc_frontier_actions must return for one agent of an oracle env, from
the oracle's own ``dijkstra_path_map`` (oracle/cpu_ref.py:240-276, called as
in :431-433).  A helper of the frontier tests, not a conftest."""
from __future__ import annotations

import numpy as np

from oracle.cpu_ref import dijkstra_path_map

ACT_STAY = 4
# the reference's neighbour order +x, -x, +y, -y with the MC_ACT_* code of each step
STEPS = (((1, 0), 0), ((-1, 0), 2), ((0, 1), 1), ((0, -1), 3))


def planning_map(ref, i):
    """(g, sx, sy): the map and start cell of dec_grid_rl.py:354-358."""
    p = ref._pad
    return ref._free_pad[i] - ref._obst_pad[i], int(ref._xinds[i]) + p, int(ref._yinds[i]) + p


def nearest_target(g, sx, sy):
    """The end point by a search of its own: BFS layers over cells != -1 from
    the start; the (x, y)-smallest 0-cell of the first layer that holds one
    (the pop order (cost, x, y)).  Returns (cost, (x, y)) or (-1, None)."""
    h, w = g.shape
    seen = np.zeros(g.shape, bool)
    seen[sx, sy] = True
    layer, cost = [(sx, sy)], 0
    while layer:
        hits = [c for c in layer if g[c] == 0]
        if hits:
            return cost, min(hits)
        nxt = []
        for x, y in layer:
            for (dx, dy), _ in STEPS:
                nx, ny = x + dx, y + dy
                if 0 <= nx < h and 0 <= ny < w and not seen[nx, ny] and g[nx, ny] != -1:
                    seen[nx, ny] = True
                    nxt.append((nx, ny))
        layer, cost = nxt, cost + 1
    return -1, None


def expected(ref, i):
    """(action, dist, (goal x, goal y)) of agent i in padded-grid coordinates."""
    p = ref._pad
    g, sx, sy = planning_map(ref, i)
    path = dijkstra_path_map(g, sx, sy)
    cells = int(path.sum())
    own = (sx - p, sy - p)
    cost, end = nearest_target(g, sx, sy)
    if cells == 0:  # no reachable unexplored cell: empty path
        assert cost == -1
        return ACT_STAY, -1, own
    dist = cells - 1
    assert dist == cost and path[end] == 1, (dist, cost, end)
    if dist == 0:  # the start cell itself is unexplored
        assert end == (sx, sy)
        return ACT_STAY, 0, own
    h, w = g.shape
    on_path = [code for (dx, dy), code in STEPS
               if 0 <= sx + dx < h and 0 <= sy + dy < w and path[sx + dx, sy + dy] == 1]
    assert len(on_path) == 1, f"agent {i}: {len(on_path)} neighbours of the start lie on the path"
    # the end point again, from the path alone: the cell other than the start
    # with one path neighbour (the cells of a shortest path touch only their
    # predecessor and successor)
    ends = []
    for x, y in zip(*np.nonzero(path)):
        nb = sum(1 for (dx, dy), _ in STEPS
                 if 0 <= x + dx < h and 0 <= y + dy < w and path[x + dx, y + dy] == 1)
        if nb == 1 and (x, y) != (sx, sy):
            ends.append((int(x), int(y)))
    assert ends == [end], (ends, end)
    return on_path[0], dist, (end[0] - p, end[1] - p)


def expected_all(ref):
    """(actions uint8 [N], dist int32 [N], goal int32 [N, 2]) of every agent."""
    out = [expected(ref, i) for i in range(ref._numrobot)]
    return (np.array([a for a, _, _ in out], np.uint8), np.array([d for _, d, _ in out], np.int32),
            np.array([q for _, _, q in out], np.int32).reshape(-1, 2))


def action_from_layer(layer):
    """The move a crop of the path (obs layer 3, E x E, the robot at the
    centre) shows: the one set 4-neighbour of the centre, STAY when none."""
    e = layer.shape[0] // 2
    on = [code for (dx, dy), code in STEPS if layer[e + dx, e + dy] == 1]
    assert len(on) <= 1, on
    return on[0] if on else ACT_STAY

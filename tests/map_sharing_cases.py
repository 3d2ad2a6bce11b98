"""Inputs of the map-sharing tests (share_kernel, csrc/mc_grid_kernels.hip,
against DecGridRLRef.shareMaps): authored robot chains, the random-walk case
table and the tile-count formula.  A helper of test_map_sharing_inputs_cpu.py
and test_gpu_map_sharing.py, not a conftest; it needs no GPU."""
from __future__ import annotations

import numpy as np

# the chains' grid: all free, 70 x 40; 72 x 42 with its border, 96 map tiles
CHAIN_W, CHAIN_L = 70, 40
# (N, R): N robots, consecutive ones at Chebyshev distance exactly R
CHAINS = ((8, 6), (16, 4), (63, 1), (64, 1))


def base_cfg(**kw):
    c = dict(numrobot=1, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0,
             terminal_reward=30, dist_reward=0, train_maxsteps=1000, test_maxsteps=1000,
             egoradius=2, mini_map_rad=0, comm_radius=0, allow_comm=0, map_sharing=0,
             single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
             sensor_config={"num_lasers": 21, "range": 10})
    c.update(kw)
    return c


def sharing_cfg(**kw):
    return base_cfg(allow_comm=1, map_sharing=1, **kw)


def tiles(W, L):
    """Map words (8 x 8-cell tiles, in 4 x 4-tile blocks) of a bordered W x L
    grid: share_kernel runs ceil(tiles / 64) workgroups per env."""
    tr, tc = -(-W // 8), -(-L // 8)
    return -(-tr // 4) * -(-tc // 4) * 16


def bern(rs, w, l, p):
    return rs.choice([1.0, -1.0], size=(w, l), p=[1 - p, p])


def tri(rs, w, l):
    return rs.choice([-1.0, 0.0, 1.0], size=(w, l), p=[0.15, 0.15, 0.7])


def chain_grid():
    return np.ones((CHAIN_W, CHAIN_L))


def chain(N, R):
    """(config, grid, cells): a snake of N robots on the all-free chain grid.
    Robot 0 at bordered cell (2, 2); each next one R further along x while
    2 <= x <= 69, else y += R and the direction reverses."""
    cells = [(2, 2)]
    x, y, step = 2, 2, R
    while len(cells) < N:
        if 2 <= x + step <= CHAIN_W - 1:
            x += step
        else:
            y += R
            step = -step
        assert 2 <= y <= CHAIN_L - 1, (N, R)
        cells.append((x, y))
    cfg = sharing_cfg(numrobot=N, comm_radius=R, sensor_config={"num_lasers": 9, "range": 2})
    return cfg, chain_grid(), cells


def chain_adjacency(N):
    """The chain's comm graph: i and j adjacent iff |i - j| <= 1."""
    i = np.arange(N)
    return (np.abs(i[:, None] - i[None, :]) <= 1).astype(np.float64)


def known_sets(ref):
    """bool [N, W + 2p, L + 2p]: the cells each agent knows (free or obstacle)."""
    return (ref._free_pad > 0) | (ref._obst_pad > 0)


def share_one_hop(known, adj):
    """What shareMaps must leave: every agent's set OR its neighbours' old sets."""
    a = (np.asarray(adj) > 0) | np.eye(len(known), dtype=bool)
    return np.stack([known[a[i]].any(axis=0) for i in range(len(known))])


def share_in_place(known, adj):
    """A wrong kernel: agents updated in ascending order, reading maps that
    earlier agents already rewrote."""
    a = (np.asarray(adj) > 0) | np.eye(len(known), dtype=bool)
    k = known.copy()
    for i in range(len(k)):
        k[i] = k[a[i]].any(axis=0)
    return k


def share_closure(known, adj):
    """A wrong kernel: the union over the whole connected component."""
    n = len(known)
    a = (np.asarray(adj) > 0) | np.eye(n, dtype=bool)
    for _ in range(n):  # reachability by repeated squaring
        b = (a.astype(np.int64) @ a.astype(np.int64)) > 0
        if np.array_equal(a, b):
            break
        a = b
    return np.stack([known[a[i]].any(axis=0) for i in range(n)])


# the radius-boundary cases on the chain grid: (comm_radius, cells, expected
# off-diagonal pairs of the comm graph)
def boundary(R):
    """Robots 0 and 1 at distance exactly R, robot 2 at R + 1 from both."""
    cells = [(10, 10), (10 + R, 10), (10, 10 + R + 1)]
    cfg = sharing_cfg(numrobot=3, comm_radius=R, sensor_config={"num_lasers": 9, "range": 2})
    return cfg, chain_grid(), cells


def boundary_adjacency():
    a = np.eye(3)
    a[0, 1] = a[1, 0] = 1
    return a


# name: (config, grid maker, B, T) -- the loop of test_batch_matches_oracle
WALK_CASES = {
    # bordered 130 x 130, 400 tiles: 7 share blocks, 16 live lanes in the last
    "c2_like": (sharing_cfg(numrobot=4, comm_radius=20), lambda rs: bern(rs, 128, 128, 0.1), 4, 12),
    # more than 32 robots
    "n33": (sharing_cfg(numrobot=33, comm_radius=5, sensor_config={"num_lasers": 7, "range": 3}),
            lambda rs: bern(rs, 30, 30, 0.1), 2, 12),
    # the accepted maximum and the one below it
    "n64": (sharing_cfg(numrobot=64, comm_radius=4), lambda rs: bern(rs, 40, 40, 0.1), 2, 10),
    "n63": (sharing_cfg(numrobot=63, comm_radius=4), lambda rs: bern(rs, 40, 40, 0.1), 2, 10),
    # bordered 38 x 72, 96 tiles: two blocks, 32 dead lanes in the second
    "tri_square_tool": (sharing_cfg(numrobot=5, comm_radius=6, single_square_tool=1, sensor_type="square_sensor",
                                    sensor_config={"range": 2}), lambda rs: tri(rs, 36, 70), 4, 25),
    "dist_n16": (sharing_cfg(numrobot=16, comm_radius=8, dist_reward=1), lambda rs: bern(rs, 64, 64, 0.1), 2, 6),
    # the path layer is computed on the shared map
    "dijkstra_n5": (sharing_cfg(numrobot=5, comm_radius=6, dijkstra_input=1), lambda rs: tri(rs, 36, 70), 4, 30),
}

# the tile count of each case's bordered grid (tiles() and the device must agree)
WALK_TILES = {"c2_like": 400, "n33": 16, "n64": 64, "n63": 64, "tri_square_tool": 96, "dist_n16": 144,
              "dijkstra_n5": 96}

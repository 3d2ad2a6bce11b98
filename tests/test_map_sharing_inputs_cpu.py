"""The authored inputs of the map-sharing GPU tests can tell a wrong share
from a right one: on each robot chain of map_sharing_cases.py the oracle's
shareMaps (one hop per step, all agents from the old maps) differs from an
in-place update and from the transitive closure on almost every agent.
Oracle only, no GPU."""
import numpy as np
import pytest

import map_sharing_cases as msc
from oracle.cpu_ref import DecGridRLRef


def test_tiles_formula():
    # bordered sizes: the chain grid, the 128 x 128 case, the 36 x 70 cases and
    # the largest maps of the older sharing cases (one 64-lane block)
    assert msc.tiles(72, 42) == 96
    assert msc.tiles(130, 130) == 400
    assert msc.tiles(38, 72) == 96
    assert msc.tiles(42, 42) == 64 and msc.tiles(62, 62) == 64
    rs = np.random.RandomState(0)
    for name, (cfg, maker, B, T) in msc.WALK_CASES.items():
        w, l = maker(rs).shape
        assert msc.tiles(w + 2, l + 2) == msc.WALK_TILES[name], name
        assert cfg["map_sharing"] == 1 and cfg["allow_comm"] == 1 and cfg["comm_radius"] > 0, name


@pytest.mark.parametrize("N,R", msc.CHAINS, ids=[f"n{n}_r{r}" for n, r in msc.CHAINS])
def test_chain_separates_wrong_shares(N, R):
    cfg, grid, cells = msc.chain(N, R)
    assert len(set(cells)) == N
    for (x0, y0), (x1, y1) in zip(cells, cells[1:]):
        assert max(abs(x0 - x1), abs(y0 - y1)) == R
    np.random.seed(0)
    ref = DecGridRLRef([grid], cfg)
    ref.reset(False, None, positions=cells)
    adj = ref._adjacency_matrix.copy()
    # consecutive robots adjacent, all others further away
    np.testing.assert_array_equal(adj, msc.chain_adjacency(N))
    old = msc.known_sets(ref)
    assert len({k.tobytes() for k in old}) == N  # no two agents start with the same map
    o, r, d = ref.step(np.full(N, 4, dtype=np.int64))  # a no-op code: nobody moves
    assert not d
    new = msc.known_sets(ref)
    want = msc.share_one_hop(old, adj)
    np.testing.assert_array_equal(new, want)
    assert int((new != old).any(axis=(1, 2)).sum()) == N  # every agent learnt something
    differs = lambda k: int((k != want).any(axis=(1, 2)).sum())
    assert differs(msc.share_in_place(old, adj)) >= N - 2
    assert differs(msc.share_closure(old, adj)) == N


@pytest.mark.parametrize("R", [1, 7])
def test_radius_boundary_cells(R):
    cfg, grid, cells = msc.boundary(R)
    np.random.seed(0)
    ref = DecGridRLRef([grid], cfg)
    ref.reset(False, None, positions=cells)
    np.testing.assert_array_equal(ref._adjacency_matrix, msc.boundary_adjacency())
    d = lambda a, b: max(abs(a[0] - b[0]), abs(a[1] - b[1]))
    assert d(cells[0], cells[1]) == R and d(cells[0], cells[2]) == R + 1 and d(cells[1], cells[2]) == R + 1
    old = msc.known_sets(ref)
    ref.step(np.full(3, 4, dtype=np.int64))
    new = msc.known_sets(ref)
    np.testing.assert_array_equal(new[2], old[2])            # R + 1 away: nothing arrives
    np.testing.assert_array_equal(new[0], old[0] | old[1])  # exactly R: shared
    np.testing.assert_array_equal(new[1], old[0] | old[1])
    assert (new[0] != old[0]).any() and (old[2] & ~new[0]).any()

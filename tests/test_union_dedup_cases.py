"""CPU, the oracle alone: the authored walks of tests/union_dedup_cases.py do what
tests/test_gpu_union_dedup.py needs of them.  Every move of every script
succeeds, the block origins are as far apart as the scenario's name says, and
every `shared` scenario -- every one whose blocks overlap but dxy3, which no
two lidars of range 10 can share a cell in -- has a step in which the robots'
own new-cell counts add up to more than the union's new cells: a step whose
reward is wrong without the dedup.  A condition, not a measurement: a scenario without such a
step has to be rewritten."""
import numpy as np
import pytest

from union_dedup_cases import DELTAS, SCENARIOS, oracle_counts

CFG = dict(numrobot=4, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0, terminal_reward=30,
           dist_reward=0, train_maxsteps=1000, test_maxsteps=1000, egoradius=2, mini_map_rad=0, comm_radius=0,
           allow_comm=0, map_sharing=0, single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
           sensor_config={"num_lasers": 21, "range": 10})


def origins(cells):
    return (np.asarray(cells) - 11) >> 3


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_is_what_its_name_says(name):
    start, script, shared = SCENARIOS[name]
    counts, cells = oracle_counts(CFG, start, script)
    moved = np.abs(np.diff(cells, axis=0)).sum(axis=2)
    want = np.asarray([[1 if b <= 3 else 0 for b in row] for row in script])
    np.testing.assert_array_equal(moved, want)  # every move succeeds, a no-op byte stays
    o = origins(cells)
    if shared:
        assert any(own > union for own, union in counts), counts
    else:  # no overlap of the blocks, or out of each other's reach: no cell is marked twice
        assert all(own == union for own, union in counts), counts
    if name in DELTAS:  # the pair's origins that many tiles apart in every step
        assert (o[:, 1] - o[:, 0] == DELTAS[name]).all(), o[:, :2]
        if not shared:
            d = np.abs(cells[:, 1] - cells[:, 0])
            assert max(DELTAS[name]) == 4 or (np.hypot(d[:, 0], d[:, 1]) > 20).all()
    if name.startswith("pair"):  # the only pair whose blocks overlap
        i, j = int(name[4]), int(name[5])
        for a in range(4):
            for b in range(a + 1, 4):
                near = (np.abs(o[:, a] - o[:, b]) <= 3).all(axis=1)
                assert near.all() if (a, b) == (i, j) else not near.any(), (a, b)
    if name == "one_tile":
        assert (o == o[:, :1]).all()
    if name == "origin_shift":
        assert o[0, 0, 0] == 0 and o[-1, 0, 0] == 1

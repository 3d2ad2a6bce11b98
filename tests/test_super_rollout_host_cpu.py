"""CPU-only: mc_sg_step_many / mc_sg_launches (fused SuperGridRL rollouts,
include/marlcov.h) are exported, typed, additive within ABI v12 and reject a
null handle before touching the device; and the oracle facts that
tests/test_gpu_super_rollout.py's distance-layer test relies on."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import marlcov  # noqa: F401
    from marlcov import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_step_many_symbols_typed_and_abi_unchanged(lib):
    from marlcov import _lib
    typed = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    res, args = typed["mc_sg_step_many"]
    assert len(args) == 11  # env, actions + stride, quot + stride, num_steps, reward + stride, done + stride, stream
    res, args = typed["mc_sg_launches"]
    assert len(args) == 2
    assert hasattr(lib, "mc_sg_step_many") and hasattr(lib, "mc_sg_launches")
    assert _lib.ABI_VERSION == 12 == lib.mc_abi_version()  # the additions raise no version


def test_step_many_null_handle_fails_without_a_device(lib):
    assert lib.mc_sg_step_many(None, None, 0, None, 0, 1, None, 0, None, 0, None) == -1
    msg = lib.mc_last_error().decode()
    assert "mc_sg_step_many" in msg and "null" in msg, msg
    assert lib.mc_sg_launches(None, 0) == -1
    msg = lib.mc_last_error().decode()
    assert "mc_sg_launches" in msg and "null" in msg, msg


def test_rollout_is_public():
    import marlcov
    for name in ("rollout", "launches", "step_many_raw"):
        assert callable(getattr(marlcov.BatchSuperGridEnv, name))


def test_distance_layer_case_defeats_a_region_write():
    """The case of test_rollout_rewrites_whole_distance_layer, on the oracle:
    over the 20 rolled-out steps max(d) stays 2, 61 cells of the layer change,
    and 43 of them lie outside the 9 x 9 region around the final cell that a
    one-step region write (side 2 (r + M_old + 1) + 1) would store."""
    from oracle.super_ref import SuperGridRLRef, l1_distance_to_uncovered
    cfg = dict(numrobot=1, train_maxsteps=1000, test_maxsteps=1000, collision_penalty=5, senseradius=1,
               free_penalty=0.2, done_thresh=1, done_incr=0, terminal_reward=30, dist_reward=0, use_scanning=0)
    np.random.seed(0)
    ref = SuperGridRLRef([np.ones((12, 48))], cfg)
    ref.reset(False, None, positions=np.array([[6, 2]]))
    for _ in range(3):
        ref.step(2)
    before, m_old = ref.get_state()[0][-1].copy(), l1_distance_to_uncovered(ref._free).max()
    for _ in range(20):
        ref.step(2)
    after, m_new = ref.get_state()[0][-1], l1_distance_to_uncovered(ref._free).max()
    assert (ref._xinds[0], ref._yinds[0]) == (6, 25)
    assert m_old == m_new == 2
    changed = np.argwhere(before != after)
    h = cfg["senseradius"] + int(m_old) + 1
    outside = [c for c in changed if abs(c[0] - 6) > h or abs(c[1] - 25) > h]
    assert (len(changed), len(outside)) == (61, 43)

"""CPU-only: mc_copy_envs / mc_sg_copy_envs (fork and restore env state on
the device, include/marlcov.h ABI v11) are exported, typed and reject null
handles before touching the device."""
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    import marlcov  # noqa: F401
    from marlcov import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize("name", ["mc_copy_envs", "mc_sg_copy_envs"])
def test_copy_envs_null_handles(lib, name):
    fn = getattr(lib, name)
    assert fn(None, None, None, None) == -1
    msg = lib.mc_last_error().decode()
    assert name in msg and "null" in msg, msg


def test_copy_envs_signatures_and_abi(lib):
    from marlcov import _lib
    typed = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for name in ("mc_copy_envs", "mc_sg_copy_envs"):
        assert name in typed
        res, args = typed[name]
        assert len(args) == 4  # dst, src, dev_src, stream
    assert _lib.ABI_VERSION == 12 == lib.mc_abi_version()  # v11 added the calls, v12 mc_sg_kernel_variant
    assert _lib.ERR_FORK == 1 << 5


def test_fork_and_sibling_are_public():
    import marlcov
    for cls in (marlcov.BatchCoverageEnv, marlcov.BatchSuperGridEnv):
        assert callable(getattr(cls, "fork")) and callable(getattr(cls, "sibling"))

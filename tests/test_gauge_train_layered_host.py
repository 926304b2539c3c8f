"""Host-side checks of l2hmc_u1_force_hvp (include/l2hmc_hip.h), the Hessian-vector product the layered gauge
training walk needs: declared, bound and exported; bad arguments and lattices too large for LDS are refused before any
launch; rows = 0 is accepted.  No GPU needed."""
import pytest

from l2hmc_amd import _lib, build as lbuild

ADDR = 256          # any non-NULL address: these calls never reach a launch


@pytest.fixture(scope="module")
def L():
    lbuild.build()
    return _lib.lib()


def _err(L):
    return L.l2hmc_last_error().decode()


def test_force_hvp_is_declared_bound_and_exported(L):
    name = "l2hmc_u1_force_hvp"
    assert name in _lib.declared_symbols() and name in _lib._PROTOS and hasattr(L, name)
    assert L.l2hmc_abi_version() == 1


def test_force_hvp_checks_arguments(L):
    f = L.l2hmc_u1_force_hvp
    assert f(ADDR, ADDR, -1, 6, 6, 1.0, ADDR, None) == 1 and "bad shape" in _err(L)
    for T, X in ((0, 6), (6, 0), (-3, 5), (3, -5)):
        assert f(ADDR, ADDR, 4, T, X, 1.0, ADDR, None) == 1 and "bad shape" in _err(L)
    for ptrs in ((None, ADDR, ADDR), (ADDR, None, ADDR), (ADDR, ADDR, None)):
        assert f(ptrs[0], ptrs[1], 4, 6, 6, 1.0, ptrs[2], None) == 1 and "NULL" in _err(L)
    assert f(None, None, 0, 6, 6, 1.0, None, None) == 0
    assert f(None, None, 0, 3, 5, 2.5, None, None) == 0


def test_force_hvp_refuses_lattices_that_do_not_fit_lds(L):
    f = L.l2hmc_u1_force_hvp
    # 20 bytes per site in one workgroup's 160 KiB: 8192 sites fit, 8193 do not
    assert f(ADDR, ADDR, 4, 128, 128, 1.0, ADDR, None) == 1 and "does not fit LDS" in _err(L)
    assert f(ADDR, ADDR, 4, 1, 8193, 1.0, ADDR, None) == 1 and "does not fit LDS" in _err(L)
    assert f(None, None, 0, 128, 128, 1.0, None, None) == 1      # refused whatever the row count
    assert f(None, None, 0, 64, 128, 1.0, None, None) == 0       # 8192 sites: accepted

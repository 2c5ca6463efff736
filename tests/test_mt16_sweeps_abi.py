"""sip_lqr_plan_set_separate_sweeps / sip_lqr_has_separate_sweeps / sip_kkt_plan_set_chain_separate_sweeps on host-only
plans (no compute calls): the opt-in takes effect exactly on the plans of the n = 32 matrix-core kernel, changes their
name and multi-rhs workspace and nothing else; a plan that never opts in is what it was."""
import ctypes

import pytest

OK, INVALID = 0, -1
SUFFIX = " + chain_factor_mt16 + chain_solve_mt16"
F64, F32 = 0, 1
BATCH, T = 4, 5
TODAY = {(F64, 32, 8): "chain_factor_solve_mt16<32,8,mfma16x16x4>/f64",
         (F32, 32, 4): "chain_factor_solve_mt16<32,4,mfma16x16x4>/f32",
         (F64, 20, 3): "chain_factor_solve_mt16<32,4,mfma16x16x4>/f64 embedding (20,3)"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_hip()
    from sip_optimal_control_amd._lib import load_library
    return load_library()


def _plan(lib, dtype, n, m):
    h = ctypes.c_void_p()
    assert lib.sip_lqr_plan_create(dtype, BATCH, T, n, m, 0, ctypes.byref(h)) == OK
    return h


def _facts(lib, h):
    return (lib.sip_lqr_kernel_name(h).decode(), int(lib.sip_lqr_workspace_bytes(h)),
            int(lib.sip_lqr_solve_multi_workspace_bytes(h, 8)))


def test_the_three_symbols_exist(lib):
    from sip_optimal_control_amd import _lib
    raw = ctypes.CDLL(_lib.library_path())
    for name in ("sip_lqr_plan_set_separate_sweeps", "sip_lqr_has_separate_sweeps",
                 "sip_kkt_plan_set_chain_separate_sweeps"):
        assert hasattr(raw, name), name


@pytest.mark.parametrize("dtype,n,m", sorted(TODAY))
def test_opt_in_on_mt16_plans(lib, dtype, n, m):
    h = _plan(lib, dtype, n, m)
    name0, ws0, cols0 = _facts(lib, h)
    assert name0 == TODAY[(dtype, n, m)] and cols0 == 0
    assert lib.sip_lqr_has_separate_sweeps(h) == 0
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 0) == OK and _facts(lib, h) == (name0, ws0, cols0)   # on = 0
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK
    assert lib.sip_lqr_has_separate_sweeps(h) == 1
    name1, ws1, cols1 = _facts(lib, h)
    assert name1 != name0 and name1.startswith(name0) and name1.endswith(SUFFIX), name1
    assert ws1 >= ws0
    exact = n == 32
    assert (cols1 > 0) == exact, cols1            # the one-sweep multi-rhs kernel: exact shapes only
    if exact:                                     # g (32) | k (m) per node and column, at most 16 columns a sweep
        esize = 8 if dtype == F64 else 4
        assert cols1 == BATCH * (T + 1) * 8 * (32 + m) * esize
        assert int(lib.sip_lqr_solve_multi_workspace_bytes(h, 40)) == BATCH * (T + 1) * 16 * (32 + m) * esize
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == INVALID          # a second opt-in
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 0) == OK
    assert _facts(lib, h) == (name1, ws1, cols1)
    lib.sip_lqr_plan_destroy(h)


@pytest.mark.parametrize("n,m", [(12, 4), (40, 4)])
def test_other_plans_are_left_alone(lib, n, m):
    h = _plan(lib, F64, n, m)
    before = _facts(lib, h)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK
    assert lib.sip_lqr_has_separate_sweeps(h) == 0
    assert _facts(lib, h) == before
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK               # nothing took effect: not "a second opt-in"
    lib.sip_lqr_plan_destroy(h)


def test_split_on_the_general_engine_is_left_alone(lib, monkeypatch):
    monkeypatch.setenv("SIP_LQR_SPLIT", "general")
    h = _plan(lib, F64, 32, 8)
    before = _facts(lib, h)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK and lib.sip_lqr_has_separate_sweeps(h) == 0
    assert _facts(lib, h) == before
    lib.sip_lqr_plan_destroy(h)


def test_null_plan(lib):
    assert lib.sip_lqr_plan_set_separate_sweeps(None, 1) == INVALID
    assert lib.sip_lqr_plan_set_separate_sweeps(None, 0) == INVALID
    assert lib.sip_lqr_has_separate_sweeps(None) == 0
    assert lib.sip_kkt_plan_set_chain_separate_sweeps(None, 1) == INVALID


@pytest.mark.parametrize("dtype,n,m", sorted(TODAY))
def test_a_plan_that_never_opts_in_is_todays(lib, dtype, n, m):
    h = _plan(lib, dtype, n, m)
    name, _, cols = _facts(lib, h)
    assert name == TODAY[(dtype, n, m)] and cols == 0 and lib.sip_lqr_has_separate_sweeps(h) == 0
    lib.sip_lqr_plan_destroy(h)

"""sip_kkt_plan_set_chain_separate_sweeps (BatchedNewtonKKT(..., chain_separate_sweeps=True)): the Newton-KKT step of a
uniform chain whose Riccati plan runs the n = 32 matrix-core kernel, with the separate factor / solve sweeps off and on,
against KKTOracle; the theta Schur complement (p columns of K^-1 J_theta through sip_lqr_solve_multi) likewise.

Both legs run at (32, 8, 4) and at the embedded (20, 3, 5), at 1e-9.  The F of a condensed problem (V ~ J^T R2^-1 J)
has a diagonal far from 1, and a sweep of F = I + D^1/2 V D^1/2 as it stands loses six digits on it: before the fused
fp64 kernel scaled F to a unit diagonal, as the factor sweep of the opt-in always did, the off legs at (32, 8, 4)
measured 1.85e-9 (factor + solve) and 1.2e-8 (theta) and were left out of this file.  With the scaling the two legs
measure the same 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.kkt import KKTOracle
from tests import reference_kkt_problems as rk

pytestmark = pytest.mark.gpu
REL = 1e-9
OK, INVALID = 0, -1
SUFFIX = " + chain_factor_mt16 + chain_solve_mt16"


@pytest.fixture(scope="module")
def lib():
    from sip_optimal_control_amd._lib import load_library
    return load_library()


def _make(dims, batch, on):
    from sip_optimal_control_amd import BatchedNewtonKKT
    return BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                            batch=batch, root=dims.root, theta_dim=dims.p, chain_separate_sweeps=on)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


@pytest.mark.parametrize("n,m,T,on", [(32, 8, 4, False), (32, 8, 4, True), (20, 3, 5, False), (20, 3, 5, True)])
def test_factor_then_two_solves(n, m, T, on):
    """factor + solve with two right-hand sides within 1e-9 of KKTOracle, the opt-in off and on."""
    batch = 3
    dims = rk.newton_kkt_dims(n, m, T)
    arrays = rk.newton_kkt_problem(dims, seed=100 * n + m, batch=batch, r2_max=1e2)
    kkt = _make(dims, batch, on)
    assert kkt.kernel_name.startswith("chain:chain_factor_solve_mt16<32,")
    assert (SUFFIX in kkt.kernel_name) == on, kkt.kernel_name
    d = _dev(*arrays)
    assert kkt.factor(*d[:5]).cpu().tolist() == [0] * batch
    o = KKTOracle(dims)
    rhs2 = np.cos(np.arange(batch * dims.kkt_dim)).reshape(batch, -1)
    for rhs in (arrays[5], rhs2):
        sol = kkt.solve(d[0], _dev(rhs)[0]).cpu().numpy()
        ref, ref_status = o.batch(*arrays[:5], rhs, threads=4)
        assert ref_status.tolist() == [0] * batch
        err = (np.abs(sol - ref) / np.abs(ref).max(axis=1, keepdims=True)).max()
        print(f"{kkt.kernel_name}: factor + solve {err:.2e}")
        assert err <= REL, err


def _theta_schur_complement(on):
    n, m, T, p, batch = 32, 8, 4, 3, 3
    base = rk.newton_kkt_dims(n, m, T)
    dims = rk.KKTDims(base.parents, base.children, base.sd, base.cd, base.ncd, base.ngd, base.ecd, base.egd,
                      theta_dim=p)
    model, w, r1, r2, r3, rhs, theta_model = rk.newton_kkt_problem(dims, seed=7 + n, batch=batch, r2_max=1e2)
    kkt = _make(dims, batch, on)
    assert kkt.kernel_name.startswith("chain:chain_factor_solve_mt16<32,8,") and (SUFFIX in kkt.kernel_name) == on, \
        kkt.kernel_name
    d = _dev(model, theta_model, w, r1, r2, r3, rhs)
    assert kkt.factor_theta(*d[:6]).cpu().tolist() == [0] * batch
    sol = kkt.solve_theta(d[0], d[1], d[6]).cpu().numpy()
    o = KKTOracle(dims)
    for q in range(batch):
        assert o.factor_theta(model[q], theta_model[q], w[q], r1[q], r2[q], r3[q]) == 0
        ref = o.solve_theta(model[q], theta_model[q], rhs[q])
        err = np.abs(sol[q] - ref).max() / np.abs(ref).max()
        print(f"{kkt.kernel_name}: theta, problem {q}: {err:.2e}")
        assert err <= REL, (q, err)


def test_theta_schur_complement():
    """(32, 8, 4) with p = 3: factor_theta (the 3 columns of K^-1 J_theta) + solve_theta within 1e-9 of the oracle."""
    _theta_schur_complement(True)


def test_theta_schur_complement_without_the_opt_in():
    """The same with the opt-in off: the columns go through the fused sweep one by one."""
    _theta_schur_complement(False)


def _kkt_plan(lib, n, m, horizon=4, batch=3):
    from tests import reference_kkt_problems as rk
    d = rk.newton_kkt_dims(n, m, horizon)
    ints = lambda v: (ctypes.c_int * max(1, len(v)))(*[int(x) for x in v])
    h = ctypes.c_void_p()
    assert lib.sip_kkt_plan_create(batch, d.E, d.root, ints(d.parents), ints(d.children), ints(d.sd), ints(d.cd),
                                   ints(d.ncd), ints(d.ngd), ints(d.ecd), ints(d.egd), 0, ctypes.byref(h)) == OK
    return h


def test_kkt_setter_follows_the_rules_of_tree_fused(lib):
    h = _kkt_plan(lib, 32, 8)
    name0, work0 = lib.sip_kkt_kernel_name(h).decode(), int(lib.sip_kkt_work_bytes(h))
    assert name0.startswith("chain:chain_factor_solve_mt16<32,8,mfma16x16x4>/f64") and SUFFIX not in name0
    assert lib.sip_kkt_plan_set_chain_separate_sweeps(h, 0) == OK
    assert lib.sip_kkt_kernel_name(h).decode() == name0
    assert lib.sip_kkt_plan_set_chain_separate_sweeps(h, 1) == OK
    name1 = lib.sip_kkt_kernel_name(h).decode()
    assert name1.startswith("chain:chain_factor_solve_mt16<32,8,mfma16x16x4>/f64" + SUFFIX), name1
    assert name1.replace(SUFFIX, "") == name0                              # what followed the Riccati kernel stays
    assert int(lib.sip_kkt_work_bytes(h)) >= work0
    assert lib.sip_kkt_plan_set_chain_separate_sweeps(h, 1) == INVALID     # a second opt-in
    lib.sip_kkt_plan_destroy(h)
    # after sip_kkt_plan_set_theta it is too late
    h = _kkt_plan(lib, 32, 8)
    assert lib.sip_kkt_plan_set_theta(h, 3) == OK
    assert lib.sip_kkt_plan_set_chain_separate_sweeps(h, 1) == INVALID
    lib.sip_kkt_plan_destroy(h)
    # a chain on another kernel: OK, nothing changes
    h = _kkt_plan(lib, 12, 4)
    name0, work0 = lib.sip_kkt_kernel_name(h).decode(), int(lib.sip_kkt_work_bytes(h))
    assert lib.sip_kkt_plan_set_chain_separate_sweeps(h, 1) == OK
    assert (lib.sip_kkt_kernel_name(h).decode(), int(lib.sip_kkt_work_bytes(h))) == (name0, work0)
    lib.sip_kkt_plan_destroy(h)

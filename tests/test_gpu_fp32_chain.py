"""fp32 plans of the chain C ABI beyond the C4 shape (32, 8): chain_factor_solve_mt16<32,4>/f32 (controls in register
0 of the four lane groups only, the fp32 row map row(g, v) = 4 g + v, the float branches of chain_mt16.hpp) and the
general engine in fp32 (launch_factor<float> / launch_solve<float> of generic_plan.hpp on tree_lds.hpp up to about
n = 48 and on tree_generic.hpp above; every fp32 plan other than (32, 4) and (32, 8) runs on it).

The checks are those of test_gpu_mf32_parity.py.  The reference is the CPU oracle on the fp32-rounded inputs cast to
double; x, u, y and K, k within 1e-4 max-abs relative to the max-abs of the oracle's row of that problem; statuses
exact; the KKT residual of sampled problems, evaluated in fp64, below 2e-4 of the right-hand-side norm.  1e-4 is a
cap, not a measurement (the fp32 recursion itself loses 6e-8 .. 3e-7 at these shapes): every test prints what it
measured, and a case more than 3x above the accepted (32, 8) kernel (sol 3.3e-6, gains 2.2e-6) is a
finding to explain, though not a failure."""
import numpy as np
import pytest

import chain_guards as cg
import full_batch_problems as fb

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL, KKT_TOL = cg.F32_TOL, cg.F32_KKT_TOL
GENERAL = "tree_generic(chain layout)/f32"
F32 = torch.float32


def _solver(n, m, T, batch):
    from sip_optimal_control_amd import BatchedChainLQR
    return BatchedChainLQR(n, m, T, batch, dtype=F32)


def _mt16_m4(T, batch):
    s = _solver(32, 4, T, batch)
    assert "mt16<32,4" in s.kernel_name and s.kernel_name.endswith("/f32"), s.kernel_name
    return s


def _general(n, m, T, batch):
    s = _solver(n, m, T, batch)
    assert s.kernel_name == GENERAL, s.kernel_name
    return s


def _factor_solve_against_the_oracle(oracle_lib, solver, mats, vecs, tag):
    """factor_solve against the oracle on the rounded problem: statuses exact and zero, x, u, y, K, k at 1e-4, the
    reference able to tell neighbouring problems apart at that tolerance, sampled KKT residuals < 2e-4."""
    n, m, T, batch = solver.shape.n, solver.shape.m, solver.shape.T, solver.batch
    sol, gains, status = solver.factor_solve(mats, vecs)
    torch.cuda.synchronize()
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert (ref_status == 0).all()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    fb.assert_discriminates(ref_sol, TOL, what=(tag, "sol"))
    es, eg = cg.rel_err(cg.host(sol), ref_sol).max(), 0.0
    if T > 0:
        fb.assert_discriminates(ref_gains, TOL, what=(tag, "gains"))
        eg = cg.rel_err(cg.host(gains), ref_gains).max()
    worst = max(cg.kkt_residual(n, m, T, mats[p], vecs[p], sol[p]) for p in sorted({0, batch - 1}))
    print(f"{tag} ({n},{m},T={T},batch={batch}) vs oracle (fp32-rounded problem): sol {es:.2e}, gains {eg:.2e}, "
          f"KKT residual {worst:.2e}")
    cg.assert_close(cg.host(sol), ref_sol, TOL, (tag, "sol"))
    cg.assert_close(cg.host(gains), ref_gains, TOL, (tag, "gains"))
    assert worst < KKT_TOL, worst


def _injected_failures(oracle_lib, solver, n, m, general):
    """The ten failures of test_gpu_mf32_parity at T = 12: factor_solve and factor report the oracle's statuses;
    the good problem still matches; on the general engine a failed problem's sol is left untouched."""
    T, batch = 12, 10
    mats, vecs = cg.make(n, m, T, batch, seed=77, dtype=F32)
    expected = cg.inject_ten_failures(n, m, T, mats)
    assert expected == [0, 3, 1, 1, 2, 2, 3, 1, 1, 3]
    ref_sol, _, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert list(ref_status) == expected          # the oracle agrees with the construction
    bad = [p for p in range(batch) if expected[p] != 0]
    sol = solver.empty_sol().fill_(cg.F_SENTINEL)
    _, _, status = solver.factor_solve(mats, vecs, sol)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    cg.assert_close(cg.host(sol[:1]), ref_sol[:1], TOL, "the good problem next to nine failing ones")
    if general:
        assert bool((sol[bad] == cg.F_SENTINEL).all()), "factor_solve wrote the sol of a failed problem"
    gains, st2 = solver.factor(mats)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(st2.cpu().numpy(), ref_status)
    sol2 = solver.empty_sol().fill_(cg.F_SENTINEL)
    solver.solve(mats, vecs, gains, sol2)
    torch.cuda.synchronize()
    cg.assert_close(cg.host(sol2[:1]), ref_sol[:1], TOL, "split solve, the good problem")
    if general:
        assert bool((sol2[bad] == cg.F_SENTINEL).all()), "solve wrote the sol of a failed problem"


def _split_entry_points(oracle_lib, solver, seed):
    """factor, then solve with two right-hand sides, then solve_multi with 3 columns (one by one: no column
    workspace), each against the oracle at 1e-4; solve's sol and the gains it leaves are BITWISE those of
    factor_solve on the same inputs."""
    n, m, T, batch = solver.shape.n, solver.shape.m, solver.shape.T, solver.batch
    mats, vecs = cg.make(n, m, T, batch, seed=seed, dtype=F32)
    _, vecs2 = cg.make(n, m, T, batch, seed=seed + 1, dtype=F32)
    sol_fs, gains_fs, st_fs = (t.clone() for t in solver.factor_solve(mats, vecs))
    gains, status = solver.factor(mats)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and (st_fs.cpu().numpy() == 0).all()
    ref = {id(v): cg.oracle_of(oracle_lib, n, m, T, mats, v) for v in (vecs, vecs2)}
    ek = cg.assert_close(cg.gains_K(cg.host(gains), n, m, T), cg.gains_K(ref[id(vecs)][1], n, m, T), TOL, "K of factor")
    sol_a = solver.solve(mats, vecs, gains).clone()
    gains_a = gains.clone()
    sol_b = solver.solve(mats, vecs2, gains).clone()
    gains_b = gains.clone()
    torch.cuda.synchronize()
    assert torch.equal(sol_a, sol_fs) and torch.equal(gains_a, gains_fs), "solve differs from factor_solve in some bit"
    errs = []
    for v, s, g in ((vecs, sol_a, gains_a), (vecs2, sol_b, gains_b)):
        errs.append((cg.assert_close(cg.host(s), ref[id(v)][0], TOL, "solve: sol"),
                     cg.assert_close(cg.host(g), ref[id(v)][1], TOL, "solve: gains")))
    assert solver.solve_multi_workspace_bytes(3) == 0          # the columns go one by one
    gen = torch.Generator(device="cuda:0").manual_seed(seed + 2)
    cols = torch.randn(3, batch, solver.shape.vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(F32)
    sol_cols = solver.solve_multi(mats, cols, gains)
    torch.cuda.synchronize()
    ec = max(cg.assert_close(cg.host(sol_cols[c]), cg.oracle_of(oracle_lib, n, m, T, mats, cols[c])[0], TOL,
                             ("solve_multi", c)) for c in range(3))
    print(f"{solver.kernel_name} ({n},{m},T={T}) split: K of factor {ek:.2e}, solve (sol, gains) {errs}, "
          f"solve_multi {ec:.2e}")


# ---- 1. chain_factor_solve_mt16<32,4>/f32 ----------------------------------------------------------------------------
@pytest.mark.parametrize("T,batch", [(100, 6), (30, 5), (1, 2), (0, 3), (7, 1)])
def test_mt16_m4_matches_the_oracle_on_the_rounded_problem(oracle_lib, T, batch):
    mats, vecs = cg.make(32, 4, T, batch, seed=4300 + T, dtype=F32)
    _factor_solve_against_the_oracle(oracle_lib, _mt16_m4(T, batch), mats, vecs, "mt16<32,4>/f32")


def test_mt16_m4_injected_failures_report_the_reference_status(oracle_lib):
    _injected_failures(oracle_lib, _mt16_m4(12, 10), 32, 4, general=False)


def test_mt16_m4_split_entry_points(oracle_lib):
    """mt16 re-runs the full sweep for the split calls (run_fused: mode 2 without a solve-only kernel becomes mode
    0), so sip_lqr_solve computes what sip_lqr_factor_solve computes: bitwise equality is asserted."""
    _split_entry_points(oracle_lib, _mt16_m4(20, 5), seed=4400)


# ---- 2. the general engine in fp32 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,T,batch", [
    (12, 4, 50, 5),      # the C3 shape in fp32
    (4, 2, 20, 7), (1, 1, 3, 4),
    (32, 5, 12, 3),      # an m that mt16 does not have
    (17, 3, 9, 5),       # odd dimensions
    (40, 6, 6, 3),       # on the LDS kernels in fp32 (lds_scalars(40, 6) * 4 = 43 KB); fp64 would be on the global ones
    (52, 4, 4, 3),       # lds_scalars(52, 4) * 4 > 64 KB: the global kernels
    (12, 4, 0, 2), (12, 4, 1, 1)])
def test_general_engine_fp32_matches_the_oracle(oracle_lib, n, m, T, batch):
    mats, vecs = cg.make(n, m, T, batch, seed=5000 + 31 * n + T, dtype=F32)
    _factor_solve_against_the_oracle(oracle_lib, _general(n, m, T, batch), mats, vecs, "general/f32")


def test_general_engine_fp32_on_the_global_kernels(oracle_lib, monkeypatch):
    """SIP_LQR_TREE=global: tree_generic.hpp's kernels at a shape that would fit the LDS ones."""
    monkeypatch.setenv("SIP_LQR_TREE", "global")
    n, m, T, batch = 7, 3, 8, 5
    mats, vecs = cg.make(n, m, T, batch, seed=5100, dtype=F32)
    _factor_solve_against_the_oracle(oracle_lib, _general(n, m, T, batch), mats, vecs, "general/f32 (global)")


@pytest.mark.parametrize("n,m", [(12, 4), (40, 6)])
def test_general_engine_fp32_injected_failures_leave_sol_untouched(oracle_lib, n, m):
    """... like test_split_solve_skips_failed_problems in fp64: the solve kernels return at a nonzero status."""
    _injected_failures(oracle_lib, _general(n, m, 12, 10), n, m, general=True)


@pytest.mark.parametrize("n,m,T,batch", [(12, 4, 20, 6), (52, 4, 4, 3)])
def test_general_engine_fp32_split_entry_points(oracle_lib, n, m, T, batch):
    """sip_lqr_factor_solve on the general engine is launch_factor then launch_solve on the caller's buffers;
    sip_lqr_factor + sip_lqr_solve are the same two launches (the solve reads the status copy kept in the
    workspace).  One wavefront per problem, no atomics, a fixed order of every sum: the arithmetic is the same, so
    bitwise equality is asserted here too (on the LDS kernels and on the global ones)."""
    _split_entry_points(oracle_lib, _general(n, m, T, batch), seed=5200 + n)


@pytest.mark.parametrize("m,T", [(8, 100), (4, 30)])
def test_two_fp32_implementations_agree_with_the_oracle(oracle_lib, monkeypatch, m, T):
    """n = 32 in fp32 on the matrix-core kernel (what a plan gets) and on the general engine
    (SIP_LQR_VARIANT=general): two independent implementations, each within 1e-4 of the oracle; their mutual
    distance is printed."""
    n, batch = 32, 3
    mats, vecs = cg.make(n, m, T, batch, seed=5300 + m, dtype=F32)
    fast = _solver(n, m, T, batch)
    assert f"mt16<32,{m}" in fast.kernel_name and fast.kernel_name.endswith("/f32")
    monkeypatch.setenv("SIP_LQR_VARIANT", "general")
    general = _general(n, m, T, batch)
    s1, g1, st1 = (t.clone() for t in fast.factor_solve(mats, vecs))
    s2, g2, st2 = (t.clone() for t in general.factor_solve(mats, vecs))
    torch.cuda.synchronize()
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert (ref_status == 0).all() and bool((st1 == 0).all()) and bool((st2 == 0).all())
    e1 = (cg.assert_close(cg.host(s1), ref_sol, TOL, "mt16 sol"), cg.assert_close(cg.host(g1), ref_gains, TOL, "mt16 gains"))
    e2 = (cg.assert_close(cg.host(s2), ref_sol, TOL, "general sol"),
          cg.assert_close(cg.host(g2), ref_gains, TOL, "general gains"))
    print(f"(32,{m},T={T}) fp32 (sol, gains): mt16 vs oracle {e1[0]:.2e} {e1[1]:.2e}, general vs oracle {e2[0]:.2e} "
          f"{e2[1]:.2e}, mt16 vs general {cg.rel_err(cg.host(s1), cg.host(s2)).max():.2e} "
          f"{cg.rel_err(cg.host(g1), cg.host(g2)).max():.2e}")

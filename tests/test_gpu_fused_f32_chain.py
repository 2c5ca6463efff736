"""The fused fp32 chain kernel chain_factor_solve_qf32 (csrc/chain_qf32.hpp; opt-in: BatchedChainLQR(...,
fused_f32=True) / sip_lqr_plan_set_fused_f32) on the GPU.

The checks are those of test_gpu_fp32_chain.py.  The reference is the CPU oracle on the fp32-rounded inputs cast to
double; x, u, y and K, k within cg.F32_TOL = 1e-4 (max-abs of a problem's row relative to the max-abs of the oracle's
row), statuses exact, the KKT residual of sampled problems, evaluated in fp64, below cg.F32_KKT_TOL = 2e-4 of the
right-hand-side norm.  Both are caps the project applies to every fp32 path, not measurements: every test prints what
it measured, next to the general fp32 engine on the same inputs where a test runs both (DESIGN section 4.9 records the
figures; more than 3x worse than the general engine is a finding to explain there, not a failure)."""
import numpy as np
import pytest

import chain_guards as cg
import full_batch_problems as fb

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL, KKT_TOL = cg.F32_TOL, cg.F32_KKT_TOL
GENERAL = "tree_generic(chain layout)/f32"
F32 = torch.float32
GRID = [(n, m) for n in (4, 6, 8, 12) for m in (1, 2, 3, 4)]
ROWS = GRID + [(1, 1), (5, 3), (9, 2), (15, 8)]
TEN_FAILURES = [0, 3, 1, 1, 2, 2, 3, 1, 1, 3]


def _fused(n, m, T, batch):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(n, m, T, batch, dtype=F32, fused_f32=True)
    assert s.has_fused_f32 and f"qf32<{n},{m}" in s.kernel_name and s.kernel_name.endswith("/f32"), s.kernel_name
    return s


def _general(n, m, T, batch):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(n, m, T, batch, dtype=F32)
    assert s.kernel_name == GENERAL and not s.has_fused_f32, s.kernel_name
    return s


def _against_the_oracle(oracle_lib, solver, mats, vecs, tag, kkt=True):
    """factor_solve against the oracle on the rounded problem: statuses exact and zero, every problem's x, u, y, K, k
    within TOL, the reference able to tell neighbouring problems apart at that tolerance, the KKT residual of problems
    0 and batch - 1 below KKT_TOL.  Returns (worst sol error, worst gains error)."""
    n, m, T, batch = solver.shape.n, solver.shape.m, solver.shape.T, solver.batch
    sol, gains, status = solver.factor_solve(mats, vecs)
    torch.cuda.synchronize()
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert (ref_status == 0).all()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    fb.assert_discriminates(ref_sol, TOL, what=(tag, "sol"))
    if T > 0:
        fb.assert_discriminates(ref_gains, TOL, what=(tag, "gains"))
    es = float(cg.rel_err(cg.host(sol), ref_sol).max())
    eg = float(cg.rel_err(cg.host(gains), ref_gains).max()) if T > 0 else 0.0
    worst = max(cg.kkt_residual(n, m, T, mats[p], vecs[p], sol[p]) for p in sorted({0, batch - 1})) if kkt else 0.0
    print(f"{tag} ({n},{m},T={T},batch={batch}) vs oracle (fp32-rounded problem): sol {es:.2e}, gains {eg:.2e}, "
          f"KKT residual {worst:.2e}")
    cg.assert_close(cg.host(sol), ref_sol, TOL, (tag, "sol"))
    cg.assert_close(cg.host(gains), ref_gains, TOL, (tag, "gains"))
    assert worst < KKT_TOL, worst
    return es, eg


# ---- 1. parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,T,batch", [(12, 4, 50, 5), (4, 2, 20, 7), (1, 1, 3, 4), (5, 3, 9, 6), (9, 2, 7, 3),
                                         (15, 8, 6, 5), (8, 3, 2, 9), (12, 4, 1, 1), (12, 4, 0, 2)])
def test_matches_the_oracle_on_the_rounded_problem(oracle_lib, n, m, T, batch):
    mats, vecs = cg.make(n, m, T, batch, seed=7000 + 31 * n + T, dtype=F32)
    _against_the_oracle(oracle_lib, _fused(n, m, T, batch), mats, vecs, "qf32")


# ---- 2. every row -----------------------------------------------------------------------------------------------------
def test_every_row_matches_the_oracle(oracle_lib):
    T, batch = 3, 5
    for n, m in ROWS:
        mats, vecs = cg.make(n, m, T, batch, seed=7100 + 16 * n + m, dtype=F32)
        _against_the_oracle(oracle_lib, _fused(n, m, T, batch), mats, vecs, "qf32 row", kkt=False)


# ---- 3. two fp32 implementations --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,T,batch", [(12, 4, 50, 5), (5, 3, 9, 6)])
def test_two_fp32_implementations_agree_with_the_oracle(oracle_lib, n, m, T, batch):
    """The opt-in plan and a default (general engine) plan on the same inputs: two independent implementations, each
    within the cap; both errors and their mutual distance are printed."""
    mats, vecs = cg.make(n, m, T, batch, seed=7200 + n, dtype=F32)
    s1, g1, st1 = (t.clone() for t in _fused(n, m, T, batch).factor_solve(mats, vecs))
    s2, g2, st2 = (t.clone() for t in _general(n, m, T, batch).factor_solve(mats, vecs))
    torch.cuda.synchronize()
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert (ref_status == 0).all() and bool((st1 == 0).all()) and bool((st2 == 0).all())
    e1 = (float(cg.rel_err(cg.host(s1), ref_sol).max()), float(cg.rel_err(cg.host(g1), ref_gains).max()))
    e2 = (float(cg.rel_err(cg.host(s2), ref_sol).max()), float(cg.rel_err(cg.host(g2), ref_gains).max()))
    print(f"({n},{m},T={T}) fp32 (sol, gains): qf32 vs oracle {e1[0]:.2e} {e1[1]:.2e}, general vs oracle {e2[0]:.2e} "
          f"{e2[1]:.2e}, qf32 vs general {cg.rel_err(cg.host(s1), cg.host(s2)).max():.2e} "
          f"{cg.rel_err(cg.host(g1), cg.host(g2)).max():.2e}")
    cg.assert_close(cg.host(s1), ref_sol, TOL, "qf32 sol"), cg.assert_close(cg.host(g1), ref_gains, TOL, "qf32 gains")
    cg.assert_close(cg.host(s2), ref_sol, TOL, "general sol")
    cg.assert_close(cg.host(g2), ref_gains, TOL, "general gains")


# ---- 4. statuses ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(12, 4), (5, 3)])
def test_injected_failures_report_the_reference_status(oracle_lib, n, m):
    T, batch = 12, 10
    solver = _fused(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=7300 + n, dtype=F32)
    expected = cg.inject_ten_failures(n, m, T, mats)
    assert expected == TEN_FAILURES
    ref_sol, _, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert list(ref_status) == expected          # the oracle agrees with the construction
    sol, _, status = solver.factor_solve(mats, vecs)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == TEN_FAILURES
    e = cg.assert_close(cg.host(sol[:1]), ref_sol[:1], TOL, "the good problem next to nine failing ones")
    gains, st2 = solver.factor(mats)
    torch.cuda.synchronize()
    assert st2.cpu().tolist() == TEN_FAILURES
    sol2 = solver.solve(mats, vecs, gains)
    torch.cuda.synchronize()
    e2 = cg.assert_close(cg.host(sol2[:1]), ref_sol[:1], TOL, "split solve, the good problem")
    print(f"qf32 ({n},{m}) ten failures: statuses exact, the good problem {e:.2e} (factor_solve) {e2:.2e} (solve)")


# ---- 5. split entry points --------------------------------------------------------------------------------------------
def test_split_entry_points(oracle_lib):
    """factor, then solve with two right-hand sides, then solve_multi with 3 columns (one by one: no column
    workspace), each against the oracle; the plan re-runs the full sweep for the split calls, so solve's sol and the
    gains it leaves are BITWISE those of factor_solve on the same inputs."""
    n, m, T, batch = 12, 4, 20, 5
    solver = _fused(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=7400, dtype=F32)
    _, vecs2 = cg.make(n, m, T, batch, seed=7401, dtype=F32)
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
    gen = torch.Generator(device="cuda:0").manual_seed(7402)
    cols = torch.randn(3, batch, solver.shape.vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(F32)
    sol_cols = solver.solve_multi(mats, cols, gains)
    torch.cuda.synchronize()
    ec = max(cg.assert_close(cg.host(sol_cols[c]), cg.oracle_of(oracle_lib, n, m, T, mats, cols[c])[0], TOL,
                             ("solve_multi", c)) for c in range(3))
    print(f"{solver.kernel_name} ({n},{m},T={T}) split: K of factor {ek:.2e}, solve (sol, gains) {errs}, "
          f"solve_multi {ec:.2e}")


# ---- 6. buffers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(12, 4), (5, 3), (15, 8)])
def test_every_entry_point_stays_inside_its_buffers(oracle_lib, n, m):
    """cg.guarded_entry_points: sol, gains, status, the workspace (exactly sip_lqr_workspace_bytes) and the solution
    columns framed by sentinels, the workspace full of NaN before factor_solve / factor, the inputs unwritten."""
    T, batch = 4, 6                                # two wavefronts, the second with two valid rows
    solver = _fused(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=7500 + n, dtype=F32)
    g, es, eg, ek = cg.guarded_entry_points(solver, mats, vecs, oracle_lib, TOL)
    assert g.broken() == []
    print(f"qf32 ({n},{m},T={T},batch={batch}) guarded: sol {es:.2e}, gains {eg:.2e}, K of factor {ek:.2e}")


# ---- 7. problem addressing --------------------------------------------------------------------------------------------
def test_every_problem_of_a_ragged_batch_and_its_permutation(oracle_lib):
    """batch 259 = 64 full wavefronts and one with three valid rows: every problem against the oracle, and the batch
    with its problems permuted gives bitwise the permuted results (a problem's answer does not depend on its row, its
    wavefront or its neighbours)."""
    n, m, T, batch = 6, 2, 5, 259
    solver = _fused(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=7600, dtype=F32)
    perm = (np.arange(batch) * 101 + 17) % batch          # 101 is coprime to 259 = 7 * 37: a permutation
    assert sorted(perm) == list(range(batch)) and (perm != np.arange(batch)).sum() >= batch - 1
    same, (sol, gains, status, _, _, _) = cg.permuted_runs_agree(solver, mats, vecs, perm)
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert (ref_status == 0).all() and bool((status == 0).all())
    fb.assert_discriminates(ref_sol, TOL, what="sol"), fb.assert_discriminates(ref_gains, TOL, what="gains")
    es = cg.assert_close(cg.host(sol), ref_sol, TOL, "sol")
    eg = cg.assert_close(cg.host(gains), ref_gains, TOL, "gains")
    print(f"qf32 ({n},{m},T={T},batch={batch}): sol {es:.2e}, gains {eg:.2e}, permuted run bitwise equal: {same}")
    assert same


@pytest.mark.parametrize("batch", [1, 4])
def test_one_problem_and_one_full_wavefront(oracle_lib, batch):
    n, m, T = 6, 2, 5
    mats, vecs = cg.make(n, m, T, batch, seed=7700 + batch, dtype=F32)
    _against_the_oracle(oracle_lib, _fused(n, m, T, batch), mats, vecs, "qf32")


# ---- 8. shapes without a row ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(16, 4), (32, 8)])
def test_the_opt_in_is_a_no_op_on_shapes_without_a_row(oracle_lib, n, m):
    from sip_optimal_control_amd import BatchedChainLQR
    T, batch = 6, 3
    default = BatchedChainLQR(n, m, T, batch, dtype=F32)
    asked = BatchedChainLQR(n, m, T, batch, dtype=F32, fused_f32=True)
    assert asked.kernel_name == default.kernel_name and asked.has_fused_f32 is False
    mats, vecs = cg.make(n, m, T, batch, seed=7800 + n, dtype=F32)
    _against_the_oracle(oracle_lib, asked, mats, vecs, asked.kernel_name)

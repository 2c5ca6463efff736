"""The separate sweeps of the fused fp32 chain kernel on the GPU: chain_factor_qf32 and chain_solve_cols_qf32
(csrc/chain_qf32_sweeps.hpp; opt-in: BatchedChainLQR(..., fused_f32=True, separate_sweeps=True)).

The reference throughout is the CPU oracle on the fp32-rounded inputs cast to double (cg.oracle_of); x, u, y and K, k
within cg.F32_TOL = 1e-4 (max-abs of a problem's row relative to the max-abs of the oracle's row), statuses exact, the KKT
residual of sampled problems below cg.F32_KKT_TOL = 2e-4.  Both are the caps the project applies to every fp32 path, not
measurements: every test prints what it measured (DESIGN section 4.9.1 records the figures)."""
import numpy as np
import pytest

import chain_guards as cg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL, KKT_TOL = cg.F32_TOL, cg.F32_KKT_TOL
F32 = torch.float32
SUFFIX = " + chain_factor_qf32 + chain_solve_qf32"
GRID = [(n, m) for n in (4, 6, 8, 12) for m in (1, 2, 3, 4)]
ROWS = GRID + [(1, 1), (5, 3), (9, 2), (15, 8)]
TEN_FAILURES = [0, 3, 1, 1, 2, 2, 3, 1, 1, 3]


def _sweeps(n, m, T, batch):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(n, m, T, batch, dtype=F32, fused_f32=True, separate_sweeps=True)
    assert s.has_fused_f32 and s.has_separate_sweeps, s.kernel_name
    assert s.kernel_name == f"chain_factor_solve_qf32<{n},{m},direct>/f32" + SUFFIX, s.kernel_name
    return s


def _fused_only(n, m, T, batch):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(n, m, T, batch, dtype=F32, fused_f32=True)
    assert s.has_fused_f32 and not s.has_separate_sweeps and SUFFIX not in s.kernel_name, s.kernel_name
    return s


def _columns(solver, ncols, seed):
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randn(ncols, solver.batch, solver.shape.vecs_len, dtype=torch.float64, device="cuda:0",
                       generator=gen).to(F32)


def _sentinel_sol(solver):
    return torch.full((solver.batch, solver.shape.vecs_len), cg.F_SENTINEL, dtype=F32, device="cuda:0")


def _factor(oracle_lib, solver, mats, vecs, tag):
    """factor on gains full of the sentinel: statuses exact and zero, K against the oracle's.  Returns (gains, the
    oracle's (sol, gains) for `vecs`, the error of K)."""
    n, m, T = solver.shape.n, solver.shape.m, solver.shape.T
    gains = torch.full((solver.batch, solver.shape.gains_len), cg.F_SENTINEL, dtype=F32, device="cuda:0")
    _, status = solver.factor(mats, gains)
    torch.cuda.synchronize()
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert (ref_status == 0).all()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    ek = 0.0
    if T > 0:
        ek = cg.assert_close(cg.gains_K(cg.host(gains), n, m, T), cg.gains_K(ref_gains, n, m, T), TOL, (tag, "K of factor"))
    return gains, (ref_sol, ref_gains), ek


def _solve(solver, mats, vecs, gains, ref, tag, kkt=True):
    """solve on a sol full of the sentinel: x, u, y and K, k against the oracle's.  Returns (sol error, gains error,
    KKT residual of problems 0 and batch - 1)."""
    n, m, T, batch = solver.shape.n, solver.shape.m, solver.shape.T, solver.batch
    sol = solver.solve(mats, vecs, gains, _sentinel_sol(solver))
    torch.cuda.synchronize()
    es = float(cg.rel_err(cg.host(sol), ref[0]).max())
    eg = float(cg.rel_err(cg.host(gains), ref[1]).max()) if T > 0 else 0.0
    res = max(cg.kkt_residual(n, m, T, mats[p], vecs[p], sol[p]) for p in sorted({0, batch - 1})) if kkt else 0.0
    print(f"{tag} ({n},{m},T={T},batch={batch}) solve vs oracle: sol {es:.2e}, gains {eg:.2e}, KKT residual {res:.2e}")
    cg.assert_close(cg.host(sol), ref[0], TOL, (tag, "sol"))
    cg.assert_close(cg.host(gains), ref[1], TOL, (tag, "gains"))
    assert res < KKT_TOL, res
    return es, eg, res


def _solve_multi(oracle_lib, solver, mats, cols, gains, tag, skip=()):
    """solve_multi on solution columns full of the sentinel, every column against the oracle's solve of that column;
    the problems in `skip` must be left untouched.  Returns the worst error."""
    n, m, T = solver.shape.n, solver.shape.m, solver.shape.T
    ncols = cols.shape[0]
    assert solver.solve_multi_workspace_bytes(ncols) == solver.batch * 4 * (T + 1) * min(ncols, 8) * (2 * n + m)
    out = torch.full((ncols, solver.batch, solver.shape.vecs_len), cg.F_SENTINEL, dtype=F32, device="cuda:0")
    solver.solve_multi(mats, cols, gains, out)
    torch.cuda.synchronize()
    keep = np.array([p for p in range(solver.batch) if p not in skip])
    worst = 0.0
    for c in range(ncols):
        ref_col = cg.oracle_of(oracle_lib, n, m, T, mats, cols[c])[0]
        worst = max(worst, cg.assert_close(cg.host(out[c])[keep], ref_col[keep], TOL, (tag, "solve_multi", ncols, c)))
        for p in skip:
            assert bool((out[c, p] == cg.F_SENTINEL).all()), (tag, "a failed problem was written", c, p)
    return worst


# ---- 1. factor, two solves, factor_solve ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,T,batch", [(12, 4, 20, 5), (5, 3, 9, 6), (15, 8, 6, 5), (1, 1, 3, 4), (9, 2, 7, 3),
                                         (12, 4, 1, 1), (12, 4, 0, 2)])
def test_factor_then_two_solves_then_factor_solve(oracle_lib, n, m, T, batch):
    solver = _sweeps(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=8000 + 31 * n + T, dtype=F32)
    _, vecs2 = cg.make(n, m, T, batch, seed=8001 + 31 * n + T, dtype=F32)
    gains, ref, ek = _factor(oracle_lib, solver, mats, vecs, "qf32 sweeps")
    ref2 = cg.oracle_of(oracle_lib, n, m, T, mats, vecs2)[:2]
    print(f"qf32 sweeps ({n},{m},T={T},batch={batch}) K of factor {ek:.2e}")
    _solve(solver, mats, vecs, gains, ref, "qf32 sweeps, rhs 1")
    _solve(solver, mats, vecs2, gains, ref2, "qf32 sweeps, rhs 2")
    # factor_solve on the opt-in plan is the fused kernel: bitwise what a fused_f32-only plan gives
    sol_a, gains_a, st_a = (t.clone() for t in solver.factor_solve(mats, vecs))
    sol_b, gains_b, st_b = (t.clone() for t in _fused_only(n, m, T, batch).factor_solve(mats, vecs))
    torch.cuda.synchronize()
    assert torch.equal(sol_a, sol_b) and torch.equal(gains_a, gains_b) and torch.equal(st_a, st_b), \
        "factor_solve of the opt-in plan differs from the fused_f32-only plan in some bit"
    cg.assert_close(cg.host(sol_a), ref[0], TOL, "factor_solve sol")


# ---- 2. every row -------------------------------------------------------------------------------------------------------
def test_every_row_factor_solve_and_two_columns(oracle_lib):
    T, batch = 3, 5
    for n, m in ROWS:
        solver = _sweeps(n, m, T, batch)
        mats, vecs = cg.make(n, m, T, batch, seed=8100 + 16 * n + m, dtype=F32)
        gains, ref, ek = _factor(oracle_lib, solver, mats, vecs, "qf32 sweeps row")
        es, eg, _ = _solve(solver, mats, vecs, gains, ref, "qf32 sweeps row", kkt=False)
        ec = _solve_multi(oracle_lib, solver, mats, _columns(solver, 2, 8150 + n), gains, "qf32 sweeps row")
        print(f"qf32 sweeps row ({n},{m}): K of factor {ek:.2e}, solve {es:.2e} {eg:.2e}, solve_multi(2) {ec:.2e}")


# ---- 3. the solve reads the factor state, not the cost ------------------------------------------------------------------
@pytest.mark.parametrize("n,m,T,batch", [(12, 4, 6, 5), (5, 3, 4, 6)])
def test_the_solve_reads_the_factor_state_not_the_cost(oracle_lib, n, m, T, batch):
    from sip_optimal_control_amd import ChainShape
    solver = _sweeps(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=8200 + n, dtype=F32)
    gains, ref, _ = _factor(oracle_lib, solver, mats, vecs, "qf32 sweeps")
    cols = _columns(solver, 3, 8201 + n)
    ref_cols = [cg.oracle_of(oracle_lib, n, m, T, mats, cols[c])[0] for c in range(3)]
    shape = ChainShape(n, m, T)
    poisoned = mats.clone()
    for i in range(T + 1):
        o = shape.mats_off(i)
        poisoned[:, o["Q"]:o["Q"] + n * n] = float("nan")
        if i < T:
            poisoned[:, o["M"]:o["M"] + n * m] = float("nan")
            poisoned[:, o["R"]:o["R"] + m * m] = float("nan")
    kept = ~torch.isnan(poisoned[0])
    assert int(kept.sum()) == (T + 1) * n + T * (n * n + n * m)          # A, B and delta stay
    sol = solver.solve(poisoned, vecs, gains, _sentinel_sol(solver))
    out = torch.full((3, batch, shape.vecs_len), cg.F_SENTINEL, dtype=F32, device="cuda:0")
    solver.solve_multi(poisoned, cols, gains, out)
    torch.cuda.synchronize()
    es = cg.assert_close(cg.host(sol), ref[0], TOL, "solve after the cost was overwritten")
    eg = cg.assert_close(cg.host(gains), ref[1], TOL, "gains after the cost was overwritten")
    ec = max(cg.assert_close(cg.host(out[c]), ref_cols[c], TOL, ("solve_multi after the cost was overwritten", c))
             for c in range(3))
    print(f"qf32 sweeps ({n},{m},T={T}) Q, M, R = NaN after factor: solve {es:.2e}, gains {eg:.2e}, solve_multi(3) {ec:.2e}")


# ---- 4. column counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,T,batch", [(12, 4, 5, 6), (5, 3, 4, 3)])
def test_solve_multi_column_counts(oracle_lib, n, m, T, batch):
    from sip_optimal_control_amd import ChainShape
    solver = _sweeps(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=8300 + n, dtype=F32)
    gains, ref, _ = _factor(oracle_lib, solver, mats, vecs, "qf32 sweeps")
    errs = {}
    for ncols in (1, 3, 9, 17):
        errs[ncols] = _solve_multi(oracle_lib, solver, mats, _columns(solver, ncols, 8310 + ncols), gains, "qf32 sweeps")
    # 8 columns, problem 2 with R_1 = -1e4 I: G fails at edge 1, its columns stay untouched, the others pass
    bad = mats.clone()
    o = ChainShape(n, m, T).mats_off(1)["R"]
    bad[2, o:o + m * m] = -1e4 * torch.eye(m, dtype=F32, device="cuda:0").reshape(-1)
    gains_bad, status = solver.factor(bad)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 3] + [0] * (batch - 3)
    errs[8] = _solve_multi(oracle_lib, solver, bad, _columns(solver, 8, 8318), gains_bad, "qf32 sweeps", skip=(2,))
    # a single solve afterwards still matches (the plan's state is that of the last factor: the good problems of `bad`)
    sol = solver.solve(bad, vecs, gains_bad, _sentinel_sol(solver))
    torch.cuda.synchronize()
    keep = np.array([p for p in range(batch) if p != 2])
    es = cg.assert_close(cg.host(sol)[keep], ref[0][keep], TOL, "solve after solve_multi")
    assert bool((sol[2] == cg.F_SENTINEL).all())
    print(f"qf32 sweeps ({n},{m},T={T},batch={batch}) solve_multi by columns {errs}, solve afterwards {es:.2e}")


# ---- 5. statuses --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(12, 4), (5, 3)])
def test_injected_failures(oracle_lib, n, m):
    T, batch = 12, 10
    solver = _sweeps(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=8400 + n, dtype=F32)
    assert cg.inject_ten_failures(n, m, T, mats) == TEN_FAILURES
    ref_sol, _, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert list(ref_status) == TEN_FAILURES
    gains, status = solver.factor(mats)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == TEN_FAILURES
    sol = solver.solve(mats, vecs, gains, _sentinel_sol(solver))
    torch.cuda.synchronize()
    e = cg.assert_close(cg.host(sol[:1]), ref_sol[:1], TOL, "the good problem next to nine failing ones")
    assert bool((sol[1:] == cg.F_SENTINEL).all()), "sol of a failed problem was written"
    print(f"qf32 sweeps ({n},{m}) ten failures: statuses exact, the good problem {e:.2e}, the others untouched")


# ---- 6. buffers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(12, 4), (5, 3), (15, 8)])
def test_every_entry_point_stays_inside_its_buffers(oracle_lib, n, m):
    T, batch = 4, 6                                # two wavefronts, the second with two valid rows
    solver = _sweeps(n, m, T, batch)
    assert solver.solve_multi_workspace_bytes(3) == batch * 4 * (T + 1) * 3 * (2 * n + m)
    mats, vecs = cg.make(n, m, T, batch, seed=8500 + n, dtype=F32)
    g, es, eg, ek = cg.guarded_entry_points(solver, mats, vecs, oracle_lib, TOL)
    assert g.broken() == []
    print(f"qf32 sweeps ({n},{m},T={T},batch={batch}) guarded: sol {es:.2e}, gains {eg:.2e}, K of factor {ek:.2e}")


# ---- 7. problem addressing ----------------------------------------------------------------------------------------------
def _split_run(solver, mats, vecs, cols):
    gains, status = solver.factor(mats, torch.zeros_like(solver.empty_gains()))     # factor leaves the k part alone
    gains_k = gains.clone()
    sol = solver.solve(mats, vecs, gains).clone()
    out = solver.solve_multi(mats, cols, gains).clone()
    torch.cuda.synchronize()
    return gains_k, status.clone(), sol, gains.clone(), out


def test_every_problem_of_a_ragged_batch_and_its_permutation(oracle_lib):
    """batch 259 = 64 full wavefronts and one with three valid rows: every problem against the oracle, and the batch
    with its problems permuted gives bitwise the permuted results."""
    n, m, T, batch = 6, 2, 5, 259
    solver = _sweeps(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=8600, dtype=F32)
    cols = _columns(solver, 3, 8601)
    perm = (np.arange(batch) * 101 + 17) % batch          # 101 is coprime to 259 = 7 * 37: a permutation
    assert sorted(perm) == list(range(batch)) and (perm != np.arange(batch)).sum() >= batch - 1
    gains, ref, ek = _factor(oracle_lib, solver, mats, vecs, "qf32 sweeps ragged")
    es, eg, _ = _solve(solver, mats, vecs, gains, ref, "qf32 sweeps ragged")
    ec = _solve_multi(oracle_lib, solver, mats, cols, gains, "qf32 sweeps ragged")
    first = _split_run(solver, mats, vecs, cols)
    pt = torch.as_tensor(perm, device="cuda:0")
    second = _split_run(solver, mats[pt].contiguous(), vecs[pt].contiguous(), cols[:, pt].contiguous())
    same = all(torch.equal(b, a[:, pt] if a.dim() == 3 else a[pt]) for a, b in zip(first, second))
    print(f"qf32 sweeps ({n},{m},T={T},batch={batch}): K of factor {ek:.2e}, solve {es:.2e} {eg:.2e}, "
          f"solve_multi(3) {ec:.2e}, permuted run bitwise equal: {same}")
    assert same


@pytest.mark.parametrize("batch", [1, 4])
def test_one_problem_and_one_full_wavefront(oracle_lib, batch):
    n, m, T = 6, 2, 5
    solver = _sweeps(n, m, T, batch)
    mats, vecs = cg.make(n, m, T, batch, seed=8700 + batch, dtype=F32)
    gains, ref, _ = _factor(oracle_lib, solver, mats, vecs, "qf32 sweeps")
    _solve(solver, mats, vecs, gains, ref, "qf32 sweeps")
    ec = _solve_multi(oracle_lib, solver, mats, _columns(solver, 3, 8701), gains, "qf32 sweeps")
    print(f"qf32 sweeps ({n},{m},T={T},batch={batch}) solve_multi(3) {ec:.2e}")

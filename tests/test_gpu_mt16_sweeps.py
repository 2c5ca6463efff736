"""The separate sweeps of the n = 32 matrix-core chain kernels (sip_lqr_plan_set_separate_sweeps;
BatchedChainLQR(..., separate_sweeps=True)): chain_factor_mt16 behind factor(), chain_solve_mt16 behind solve() (one
column, g and k through the spill and the gains) and behind solve_multi() (up to 16 columns per sweep through the column
workspace; embedded shapes column by column), on exact and embedded shapes, fp64 and fp32.

The reference is always the CPU oracle on the inputs as stored (tests/chain_guards.py); tolerances are the project's
own: 1e-9 in fp64, 1e-4 in fp32, max-abs of a problem's row relative to the max-abs of the oracle's row."""
import numpy as np
import pytest

import chain_guards as cg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
SUFFIX = " + chain_factor_mt16 + chain_solve_mt16"


def _tol(dtype):
    return cg.F64_TOL if dtype == F64 else cg.F32_TOL


def _solver(n, m, T, batch, dtype):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(n, m, T, batch, dtype=dtype, separate_sweeps=True)
    assert s.has_separate_sweeps and "chain_factor_solve_mt16<32," in s.kernel_name and s.kernel_name.endswith(SUFFIX), \
        s.kernel_name
    assert ("embedding" in s.kernel_name) == (n != 32 or m not in (4, 8))
    return s


def _cols(num, batch, vecs_len, dtype, seed):
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randn(num, batch, vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(dtype)


PARITY = [(F64, 32, 8, 6, 3), (F64, 32, 4, 5, 3), (F64, 32, 8, 0, 3), (F64, 32, 8, 1, 2), (F64, 32, 7, 3, 2),
          (F64, 20, 3, 6, 5), (F64, 17, 1, 4, 2), (F64, 31, 5, 5, 3),
          (F32, 32, 8, 4, 3), (F32, 32, 4, 7, 2),
          (F64, 32, 8, 100, 6), (F32, 32, 8, 100, 6)]


@pytest.mark.parametrize("dtype,n,m,T,batch", PARITY, ids=lambda v: str(v).replace("torch.", ""))
def test_factor_then_two_solves_match_the_oracle(oracle_lib, dtype, n, m, T, batch):
    """factor: the oracle's statuses and K; two solves with different right-hand sides on the one factorization: x, u,
    y and K, k; factor_solve on the same plan still matches."""
    tol = _tol(dtype)
    solver = _solver(n, m, T, batch, dtype)
    mats, vecs = cg.make(n, m, T, batch, seed=310 + n + m, dtype=dtype)
    _, vecs2 = cg.make(n, m, T, batch, seed=911 + n + m, dtype=dtype)
    refs = [cg.oracle_of(oracle_lib, n, m, T, mats, v) for v in (vecs, vecs2)]
    assert (refs[0][2] == 0).all()
    gains = solver.empty_gains().fill_(cg.F_SENTINEL)
    solver.status.fill_(cg.I_SENTINEL)
    _, status = solver.factor(mats, gains)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), refs[0][2])
    ek = cg.assert_close(cg.gains_K(cg.host(gains), n, m, T), cg.gains_K(refs[0][1], n, m, T), tol, "K of factor")
    errs = []
    for v, (ref_sol, ref_gains, _) in zip((vecs, vecs2), refs):
        sol = solver.empty_sol().fill_(cg.F_SENTINEL)
        solver.solve(mats, v, gains, sol)
        torch.cuda.synchronize()
        es, eg = cg.rel_err(cg.host(sol), ref_sol).max(), cg.rel_err(cg.host(gains), ref_gains).max() if T else 0.0
        errs.append((float(es), float(eg)))
        print(f"{solver.kernel_name} ({n},{m},T={T}) solve: sol {es:.2e}, gains {eg:.2e}")
        cg.assert_close(cg.host(sol), ref_sol, tol, "solve: x, u, y")
        cg.assert_close(cg.host(gains), ref_gains, tol, "solve: K, k")
    sol, gains_fs, status = solver.factor_solve(mats, vecs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), refs[0][2])
    cg.assert_close(cg.host(sol), refs[0][0], tol, "factor_solve: sol")
    cg.assert_close(cg.host(gains_fs), refs[0][1], tol, "factor_solve: gains")
    print(f"{solver.kernel_name} ({n},{m},T={T},batch={batch}): K of factor {ek:.2e}, solves {errs}")


MULTI = [(F64, 32, 8, 5, 3, 1), (F64, 32, 8, 5, 3, 3), (F64, 32, 8, 5, 3, 16), (F64, 32, 8, 5, 3, 17),
         (F32, 32, 4, 4, 3, 8), (F64, 20, 3, 4, 3, 2)]


@pytest.mark.parametrize("dtype,n,m,T,batch,cols", MULTI, ids=lambda v: str(v).replace("torch.", ""))
def test_solve_multi_every_column_against_the_oracle(oracle_lib, dtype, n, m, T, batch, cols):
    """Every column against the oracle's solve of that column; 17 columns take a second sweep.  In the 16-column case
    problem 2 fails (R_1 = -1e4 I): status 3, all its solution columns stay at the sentinel, the others are exact.
    A single solve afterwards still matches."""
    from sip_optimal_control_amd import ChainShape
    tol = _tol(dtype)
    solver = _solver(n, m, T, batch, dtype)
    shape = ChainShape(n, m, T)
    mats, _ = cg.make(n, m, T, batch, seed=700 + n + cols, dtype=dtype)
    failing = cols == 16
    if failing:
        off = shape.mats_off(1)["R"]
        mats[2, off:off + m * m] = -1e4 * torch.eye(m, dtype=dtype, device="cuda:0").reshape(-1)
    vecs_cols = _cols(cols, batch, shape.vecs_len, dtype, seed=5)
    assert (solver.solve_multi_workspace_bytes(cols) > 0) == (n == 32)       # one sweep per 16 columns: exact shapes
    gains, status = solver.factor(mats)
    sol_cols = torch.full((cols, batch, shape.vecs_len), cg.F_SENTINEL, dtype=dtype, device="cuda:0")
    solver.solve_multi(mats, vecs_cols, gains, sol_cols)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st.tolist() == ([0, 0, 3] if failing else [0] * batch)
    ok = st == 0
    worst = 0.0
    for col in range(cols):
        ref_sol, _, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs_cols[col])
        np.testing.assert_array_equal(st, ref_status)
        worst = max(worst, cg.assert_close(cg.host(sol_cols[col])[ok], ref_sol[ok], tol, ("solve_multi", col)))
    if failing:
        assert bool((sol_cols[:, 2] == cg.F_SENTINEL).all()), "a column of the failed problem was written"
    one = solver.solve(mats, vecs_cols[0].contiguous(), gains)
    torch.cuda.synchronize()
    ref_sol, _, _ = cg.oracle_of(oracle_lib, n, m, T, mats, vecs_cols[0])
    cg.assert_close(cg.host(one)[ok], ref_sol[ok], tol, "solve after solve_multi")
    print(f"{solver.kernel_name} ({n},{m},T={T}) solve_multi, {cols} columns: {worst:.2e}")


@pytest.mark.parametrize("dtype,n,m", [(F64, 32, 8), (F32, 32, 8), (F64, 20, 3)], ids=["f64", "f32", "f64-embedded"])
def test_injected_failures(oracle_lib, dtype, n, m):
    """The ten injected failures of chain_guards at T = 12 through factor: the oracle's statuses; in the solve that
    follows the good problem matches and the sol of every failed problem stays at the sentinel (through the embedding
    too: the unpack of the padded sol skips them)."""
    T, batch = 12, 10
    solver = _solver(n, m, T, batch, dtype)
    mats, vecs = cg.make(n, m, T, batch, seed=77, dtype=dtype)
    expected = cg.inject_ten_failures(n, m, T, mats)
    ref_sol, _, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert list(ref_status) == expected == [0, 3, 1, 1, 2, 2, 3, 1, 1, 3]
    gains, status = solver.factor(mats)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    sol = solver.empty_sol().fill_(cg.F_SENTINEL)
    solver.solve(mats, vecs, gains, sol)
    torch.cuda.synchronize()
    cg.assert_close(cg.host(sol[:1]), ref_sol[:1], _tol(dtype), "the good problem next to nine failing ones")
    assert bool((sol[1:] == cg.F_SENTINEL).all()), "solve wrote the sol of a failed problem"


@pytest.mark.parametrize("dtype,n,m,T,batch", [(F32, 32, 4, 5, 3), (F32, 32, 8, 4, 3), (F64, 32, 8, 4, 3),
                                               (F64, 20, 3, 6, 5)], ids=lambda v: str(v).replace("torch.", ""))
def test_guarded_entry_points(oracle_lib, dtype, n, m, T, batch):
    """Every entry point on guarded buffers: guard bands intact, a NaN-filled workspace before factor, inputs bitwise
    what they were, every result against the oracle."""
    solver = _solver(n, m, T, batch, dtype)
    mats, vecs = cg.make(n, m, T, batch, seed=40 + n + m, dtype=dtype)
    g, es, eg, ek = cg.guarded_entry_points(solver, mats, vecs, oracle_lib, _tol(dtype))
    assert g.broken() == []
    print(f"{solver.kernel_name} ({n},{m},T={T}) guarded: sol {es:.2e}, gains {eg:.2e}, K of factor {ek:.2e}")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_order_independence(dtype):
    """One problem per wavefront: a batch of 5 run again under a permutation gives the same bits, permuted, for
    factor + solve and for solve_multi with 3 columns."""
    n, m, T, batch = 32, 8, 4, 5
    perm = torch.as_tensor([3, 0, 4, 2, 1], device="cuda:0")
    solver = _solver(n, m, T, batch, dtype)
    mats, vecs = cg.make(n, m, T, batch, seed=21, dtype=dtype)
    cols = _cols(3, batch, solver.shape.vecs_len, dtype, seed=22)

    def run(mats_, vecs_, cols_):
        gains, status = solver.factor(mats_)
        sol = solver.solve(mats_, vecs_, gains)
        gains_after_solve = gains.clone()
        sol_cols = solver.solve_multi(mats_, cols_, gains)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        return sol.clone(), gains_after_solve, sol_cols.clone()

    sol, gains, sol_cols = run(mats, vecs, cols)
    sol_p, gains_p, sol_cols_p = run(mats[perm].contiguous(), vecs[perm].contiguous(), cols[:, perm].contiguous())
    assert torch.equal(sol_p, sol[perm]) and torch.equal(gains_p, gains[perm]), "factor + solve depend on the order"
    assert torch.equal(sol_cols_p, sol_cols[:, perm]), "solve_multi depends on the order"

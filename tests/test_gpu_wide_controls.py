"""The n = 32 matrix-core chain kernels for 12 and 16 controls (sip_lqr_plan_set_wide_controls;
BatchedChainLQR(..., wide_controls=True), BatchedNewtonKKT(..., chain_wide_controls=True)) on the GPU: the exact rows
(32, 12) and (32, 16) in fp64 and fp32, fp64 shapes with 9 <= m <= 16, n <= 32 embedded in them, the separate sweeps
on top, the Newton-KKT step on such a chain and the fused sweep under graph capture.

The reference is always the CPU oracle on the inputs as stored (tests/chain_guards.py); tolerances are the project's
own: 1e-9 in fp64 (statuses exact); in fp32 e_gpu <= F32_TOL + 3 e_general, e_general the error of the general fp32
engine on the same rounded inputs.  Every case asserts the kernel name it expects."""
import numpy as np
import pytest

import chain_guards as cg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
TAG = {F64: "f64", F32: "f32"}
SUFFIX = " + chain_factor_mt16 + chain_solve_mt16"
GENERAL = "tree_generic(chain layout)/"
# (n, m) -> M of the row that serves it
EXACT = {(32, 12): 12, (32, 16): 16}
EMBEDDED = {(17, 9): 12, (32, 9): 12, (24, 12): 12, (31, 13): 16, (16, 16): 16, (12, 12): 12, (5, 16): 16, (1, 9): 12}


def _name(dtype, n, m, separate=False):
    M = EXACT.get((n, m)) or EMBEDDED[(n, m)]
    name = f"chain_factor_solve_mt16<32,{M},mfma16x16x4>/{TAG[dtype]}"
    if (n, m) not in EXACT:
        name += f" embedding ({n},{m})"
    return name + (SUFFIX if separate else "")


def _solver(n, m, T, batch, dtype=F64, separate=False):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(n, m, T, batch, dtype=dtype, wide_controls=True, separate_sweeps=separate)
    assert s.has_wide_controls and s.has_separate_sweeps == separate
    assert s.kernel_name == _name(dtype, n, m, separate), s.kernel_name
    return s


def _cols(num, batch, vecs_len, dtype, seed):
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randn(num, batch, vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(dtype)


# ---- fp64 against the oracle -------------------------------------------------------------------------------------
CASES_F64 = [(32, 12, 1, 5), (32, 12, 5, 5), (32, 16, 1, 5), (32, 16, 5, 5),
             (17, 9, 4, 5), (32, 9, 3, 3), (24, 12, 5, 4), (31, 13, 6, 3), (16, 16, 4, 7), (12, 12, 5, 6), (5, 16, 6, 5),
             (1, 9, 3, 7)]


@pytest.mark.parametrize("separate", [False, True], ids=["fused", "separate"])
@pytest.mark.parametrize("n,m,T,batch", CASES_F64)
def test_every_entry_point_on_guarded_buffers(oracle_lib, n, m, T, batch, separate):
    """factor_solve, factor, solve and solve_multi(3) against the oracle at 1e-9 on guarded buffers, from a workspace
    full of NaN, the inputs bitwise untouched (chain_guards.guarded_entry_points)."""
    solver = _solver(n, m, T, batch, separate=separate)
    mats, vecs = cg.make(n, m, T, batch, seed=1200 + 31 * n + m, dtype=F64)
    g, es, eg, ek = cg.guarded_entry_points(solver, mats, vecs, oracle_lib, cg.F64_TOL)
    assert g.broken() == []
    print(f"{solver.kernel_name} ({n},{m},T={T}) guarded: sol {es:.2e}, gains {eg:.2e}, K of factor {ek:.2e}")


@pytest.mark.parametrize("separate", [False, True], ids=["fused", "separate"])
@pytest.mark.parametrize("n,m", sorted(EXACT))
def test_a_chain_of_one_node(oracle_lib, n, m, separate):
    """T = 0: no edge, no gains; every entry point on guarded buffers."""
    T, batch = 0, 5
    solver = _solver(n, m, T, batch, separate=separate)
    mats, vecs = cg.make(n, m, T, batch, seed=5 + m, dtype=F64)
    ref_sol, _, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert (ref_status == 0).all()
    g = cg.Guarded(solver, num_rhs=3)
    g.reset_outputs(), g.poison_workspace()
    solver.factor_solve(mats, vecs, g.sol, g.gains)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(solver.status.cpu().numpy(), ref_status)
    cg.assert_close(cg.host(g.sol), ref_sol, cg.F64_TOL, "factor_solve")
    g.reset_outputs(), g.poison_workspace()
    solver.factor(mats, g.gains)
    solver.solve(mats, vecs, g.gains, g.sol)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(solver.status.cpu().numpy(), ref_status)
    cg.assert_close(cg.host(g.sol), ref_sol, cg.F64_TOL, "factor + solve")
    assert g.broken() == []


@pytest.mark.parametrize("n,m", [(32, 16), (17, 9)], ids=["exact", "embedded"])
def test_injected_failures_report_the_reference_status(oracle_lib, n, m):
    """FactorStatus with injected failures (G, invalid delta, F), the precedence at a node and "first failing node in
    postorder", exact against the oracle: through the fused sweep and through the factor sweep, whose solve leaves
    the sol of every failed problem untouched (through the embedding too)."""
    T, batch = 12, 10
    mats, vecs = cg.make(n, m, T, batch, seed=78, dtype=F64)
    expected = cg.inject_ten_failures(n, m, T, mats)
    ref_sol, _, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert list(ref_status) == expected == [0, 3, 1, 1, 2, 2, 3, 1, 1, 3]
    _, _, status = _solver(n, m, T, batch).factor_solve(mats, vecs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    solver = _solver(n, m, T, batch, separate=True)
    gains, status = solver.factor(mats)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    sol = solver.empty_sol().fill_(cg.F_SENTINEL)
    solver.solve(mats, vecs, gains, sol)
    torch.cuda.synchronize()
    cg.assert_close(cg.host(sol[:1]), ref_sol[:1], cg.F64_TOL, "the good problem next to nine failing ones")
    assert bool((sol[1:] == cg.F_SENTINEL).all()), "solve wrote the sol of a failed problem"


# ---- the separate sweeps -------------------------------------------------------------------------------------------
def _errors_f32(oracle_lib, n, m, T, mats, vecs_list):
    """Per right-hand side: (oracle's sol, gains, status; e_general of sol, of gains, of the K blocks alone) -- the
    general fp32 engine on the same rounded inputs, each error the worst rel_err over the problems against the oracle."""
    import os
    from sip_optimal_control_amd import BatchedChainLQR
    old = os.environ.get("SIP_LQR_VARIANT")
    os.environ["SIP_LQR_VARIANT"] = "general"
    try:
        general = BatchedChainLQR(n, m, T, mats.shape[0], dtype=F32)
    finally:
        if old is None:
            del os.environ["SIP_LQR_VARIANT"]
        else:
            os.environ["SIP_LQR_VARIANT"] = old
    assert general.kernel_name == GENERAL + "f32", general.kernel_name
    out = []
    for vecs in vecs_list:
        ref = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
        sol, gains, status = general.factor_solve(mats, vecs)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(status.cpu().numpy(), ref[2])
        e_k = cg.rel_err(cg.gains_K(cg.host(gains), n, m, T), cg.gains_K(ref[1], n, m, T)).max() if T else 0.0
        out.append((ref, float(cg.rel_err(cg.host(sol), ref[0]).max()), float(cg.rel_err(cg.host(gains), ref[1]).max()),
                    float(e_k)))
    return out


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,m", sorted(EXACT))
def test_factor_then_two_solves(oracle_lib, dtype, n, m):
    """One factor (the oracle's statuses and K), then two solves with different right-hand sides on it."""
    T, batch = 5, 3
    solver = _solver(n, m, T, batch, dtype, separate=True)
    mats, vecs = cg.make(n, m, T, batch, seed=310 + n + m, dtype=dtype)
    _, vecs2 = cg.make(n, m, T, batch, seed=911 + n + m, dtype=dtype)
    if dtype == F64:
        refs = [(cg.oracle_of(oracle_lib, n, m, T, mats, v), 0.0, 0.0, 0.0) for v in (vecs, vecs2)]
        tol = cg.F64_TOL
    else:
        refs = _errors_f32(oracle_lib, n, m, T, mats, (vecs, vecs2))
        tol = cg.F32_TOL
    assert (refs[0][0][2] == 0).all()
    gains = solver.empty_gains().fill_(cg.F_SENTINEL)
    solver.status.fill_(cg.I_SENTINEL)
    _, status = solver.factor(mats, gains)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), refs[0][0][2])
    cg.assert_close(cg.gains_K(cg.host(gains), n, m, T), cg.gains_K(refs[0][0][1], n, m, T), tol + 3 * refs[0][3],
                    "K of factor")
    for v, ((ref_sol, ref_gains, _), e_sol, e_gains, _) in zip((vecs, vecs2), refs):
        sol = solver.empty_sol().fill_(cg.F_SENTINEL)
        solver.solve(mats, v, gains, sol)
        torch.cuda.synchronize()
        es = cg.assert_close(cg.host(sol), ref_sol, tol + 3 * e_sol, "solve: x, u, y")
        eg = cg.assert_close(cg.host(gains), ref_gains, tol + 3 * e_gains, "solve: K, k")
        print(f"{solver.kernel_name} solve: sol {es:.2e} (general {e_sol:.2e}), gains {eg:.2e} (general {e_gains:.2e})")


@pytest.mark.parametrize("cols", [1, 3, 16, 17])
@pytest.mark.parametrize("dtype,n,m", [(F64, 32, 12), (F64, 32, 16), (F32, 32, 12), (F32, 32, 16)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_solve_multi_every_column_against_the_oracle(oracle_lib, dtype, n, m, cols):
    """Every column against the oracle's solve of that column; 17 columns take a second sweep.  In the 16-column case
    problem 2 fails (R_1 = -1e4 I): status 3, all its solution columns stay at the sentinel, the others are exact."""
    from sip_optimal_control_amd import ChainShape
    T, batch = 4, 3
    solver = _solver(n, m, T, batch, dtype, separate=True)
    shape = ChainShape(n, m, T)
    mats, _ = cg.make(n, m, T, batch, seed=700 + m + cols, dtype=dtype)
    failing = cols == 16
    if failing:
        off = shape.mats_off(1)["R"]
        mats[2, off:off + m * m] = -1e4 * torch.eye(m, dtype=dtype, device="cuda:0").reshape(-1)
    vecs_cols = _cols(cols, batch, shape.vecs_len, dtype, seed=5)
    esize = 8 if dtype == F64 else 4
    assert solver.solve_multi_workspace_bytes(cols) == batch * (T + 1) * min(cols, 16) * (32 + m) * esize
    gains, status = solver.factor(mats)
    sol_cols = torch.full((cols, batch, shape.vecs_len), cg.F_SENTINEL, dtype=dtype, device="cuda:0")
    solver.solve_multi(mats, vecs_cols, gains, sol_cols)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st.tolist() == ([0, 0, 3] if failing else [0] * batch)
    ok = st == 0
    refs = [cg.oracle_of(oracle_lib, n, m, T, mats, vecs_cols[c]) for c in range(cols)]
    e_general = [0.0] * cols
    if dtype == F32 and not failing:      # (a failed problem has no solution to measure the general engine on)
        e_general = [e for _, e, _, _ in _errors_f32(oracle_lib, n, m, T, mats, [vecs_cols[c].contiguous() for c in range(cols)])]
    tol = cg.F64_TOL if dtype == F64 else cg.F32_TOL
    worst = 0.0
    for col, (ref_sol, _, ref_status) in enumerate(refs):
        np.testing.assert_array_equal(st, ref_status)
        worst = max(worst, cg.assert_close(cg.host(sol_cols[col])[ok], ref_sol[ok], tol + 3 * e_general[col],
                                           ("solve_multi", col)))
    if failing:
        assert bool((sol_cols[:, 2] == cg.F_SENTINEL).all()), "a column of the failed problem was written"
    print(f"{solver.kernel_name} solve_multi, {cols} columns: {worst:.2e}")


def test_solve_multi_on_an_embedded_shape_loops_the_columns(oracle_lib):
    from sip_optimal_control_amd import ChainShape
    n, m, T, batch, cols = 17, 9, 4, 3, 3
    solver = _solver(n, m, T, batch, separate=True)
    assert solver.solve_multi_workspace_bytes(cols) == 0
    mats, _ = cg.make(n, m, T, batch, seed=41, dtype=F64)
    vecs_cols = _cols(cols, batch, ChainShape(n, m, T).vecs_len, F64, seed=6)
    gains, status = solver.factor(mats)
    sol_cols = solver.solve_multi(mats, vecs_cols, gains)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * batch
    for col in range(cols):
        ref_sol, _, _ = cg.oracle_of(oracle_lib, n, m, T, mats, vecs_cols[col])
        cg.assert_close(cg.host(sol_cols[col]), ref_sol, cg.F64_TOL, ("solve_multi", col))


# ---- fp32, the fused sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", sorted(EXACT))
def test_fp32_fused_sweep(oracle_lib, n, m):
    """Statuses exact; e_gpu <= F32_TOL + 3 e_general on sol and gains, against the oracle on the rounded inputs."""
    T, batch = 5, 4
    solver = _solver(n, m, T, batch, F32)
    mats, vecs = cg.make(n, m, T, batch, seed=60 + m, dtype=F32)
    ((ref_sol, ref_gains, ref_status), e_sol, e_gains, _), = _errors_f32(oracle_lib, n, m, T, mats, (vecs,))
    assert (ref_status == 0).all()
    sol, gains, status = solver.factor_solve(mats, vecs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    es = float(cg.rel_err(cg.host(sol), ref_sol).max())
    eg = float(cg.rel_err(cg.host(gains), ref_gains).max())
    print(f"{solver.kernel_name}: sol {es:.2e} (general {e_sol:.2e}), gains {eg:.2e} (general {e_gains:.2e})")
    assert es <= cg.F32_TOL + 3 * e_sol and eg <= cg.F32_TOL + 3 * e_gains
    # the split calls re-run the sweep
    g2, st2 = solver.factor(mats)
    sol2 = solver.solve(mats, vecs, g2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(st2.cpu().numpy(), ref_status)
    assert float(cg.rel_err(cg.host(sol2), ref_sol).max()) <= cg.F32_TOL + 3 * e_sol


# ---- Newton-KKT --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("separate", [False, True], ids=["fused", "separate"])
@pytest.mark.parametrize("n,m", [(32, 12), (17, 9)])
def test_newton_kkt_step(n, m, separate):
    """BatchedNewtonKKT(chain_wide_controls=True) against kkt_oracle at the 1e-9 of tests/test_gpu_kkt.py's chain
    shapes: sip_kkt_factor_solve, and sip_kkt_factor followed by two sip_kkt_solve."""
    from oracle.kkt import KKTOracle
    from sip_optimal_control_amd import BatchedNewtonKKT
    from tests import reference_kkt_problems as rk
    T, batch = 4, 4
    dims = rk.newton_kkt_dims(n, m, T)
    arrays = rk.newton_kkt_problem(dims, seed=100 * n + m, batch=batch, r2_max=1e2)
    plain = BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                             batch=batch, root=dims.root)
    assert plain.kernel_name.startswith("chain:" + GENERAL + "f64"), plain.kernel_name
    kkt = BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                           batch=batch, root=dims.root, chain_wide_controls=True, chain_separate_sweeps=separate)
    assert kkt.kernel_name.startswith("chain:" + _name(F64, n, m, separate) + " + "), kkt.kernel_name
    assert kkt.kernel_name[len("chain:" + _name(F64, n, m, separate)):] == plain.kernel_name[len("chain:" + GENERAL + "f64"):]
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]
    o = KKTOracle(dims)
    ref, ref_status = o.batch(*arrays, threads=4)
    assert ref_status.tolist() == [0] * batch
    scale = np.abs(ref).max(axis=1, keepdims=True)
    sol, status = kkt.factor_solve(*d)
    assert status.cpu().tolist() == [0] * batch
    assert (np.abs(sol.cpu().numpy() - ref) / scale).max() <= 1e-9
    status = kkt.factor(*d[:5])
    assert status.cpu().tolist() == [0] * batch
    rhs2 = np.cos(np.arange(batch * dims.kkt_dim, dtype=np.float64)).reshape(batch, -1)
    ref2, _ = o.batch(*arrays[:5], rhs2, threads=4)
    for rhs, want in ((d[5], ref), (torch.from_numpy(rhs2).cuda(), ref2)):
        got = kkt.solve(d[0], rhs).cpu().numpy()
        assert (np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True)).max() <= 1e-9


# ---- graph capture -------------------------------------------------------------------------------------------------
def test_the_fused_sweep_of_an_embedded_plan_is_graph_capturable(oracle_lib):
    """The compute entry points only enqueue kernels: factor_solve of an embedded opt-in plan (repack, sweep, unpack:
    a linear chain on one stream) captured in a graph and replayed twice gives the bits of the eager run."""
    n, m, T, batch = 17, 9, 5, 6
    mats, vecs = cg.make(n, m, T, batch, seed=92, dtype=F64)
    solver = _solver(n, m, T, batch)
    eager_sol, eager_gains, status = solver.factor_solve(mats, vecs)
    torch.cuda.synchronize()
    eager_sol, eager_gains, eager_status = eager_sol.clone(), eager_gains.clone(), status.clone()
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    np.testing.assert_array_equal(eager_status.cpu().numpy(), ref_status)
    cg.assert_close(cg.host(eager_sol), ref_sol, cg.F64_TOL, "eager")
    sol, gains = solver.empty_sol().zero_(), solver.empty_gains().zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        solver.factor_solve(mats, vecs, sol, gains)
    torch.cuda.synchronize()
    assert float(sol.abs().max()) == 0.0               # captured, not executed
    for _ in range(2):
        sol.zero_(), gains.zero_(), solver.status.fill_(cg.I_SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sol, eager_sol) and torch.equal(gains, eager_gains)
        assert torch.equal(solver.status, eager_status)

"""Every problem of full-size batches against the CPU oracle, for the kernels that serve real batches but were
compared with the oracle on a handful of problems only: the fused tree sweep (csrc/tree_qw16.hpp, plain and with
workspace export), the tree multi-rhs solve (csrc/tree_mrhs_qw16.hpp), the theta Schur complement on trees, the
fp32 and fp64 C4 chain kernels and the Newton-KKT step.

A per-problem addressing bug (a wrong problem stride, a wavefront reading its neighbour's rows, a grid.y column
group landing on the wrong slot, a clamped tail wavefront that stores) shows only with more than two wavefronts of
DISTINCT problems, so every batch here is 4096 (or 4093: a partial last wavefront) distinct problems, and every
comparison first asserts that it can tell neighbouring problems apart (full_batch_problems.assert_discriminates).
Guard rows past the end of every output arena must come back bitwise unchanged.

Tolerances are those of the existing tests of each kernel: 1e-10 relative to the block max for the tree kernels
(test_gpu_tree.py), 1e-9 for fp64 chains and Newton-KKT (test_gpu_mt16_f64.py, test_gpu_kkt.py), 1e-8 for theta
(test_gpu_kkt_tree_theta.py), 1e-4 for fp32 against the oracle on the fp32-rounded problem
(test_gpu_mf32_parity.py).  The worst measured error of every comparison is printed."""
import functools
import zlib

import numpy as np
import pytest

import full_batch_problems as fb
from oracle import oracle
from oracle.kkt import KKTDims, KKTOracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

THREADS = fb.oracle_threads()
BATCHES = [4096, 4093]
TREE_TOL = 1e-10
F_SENTINEL = -3.0e33
I_SENTINEL = 0x5EED5EED
GUARD = 4            # rows past the end of every arena: one whole wavefront of the tree kernels

# the three variable-benchmark shapes (T = 63) and one random tree in each size class of tree_qw16 (every one
# with two zero-dimensional nodes)
TOPOLOGIES = ["vb0", "vb1", "vb2", "r4_2", "r6_3", "r8_4", "r9_3", "r10_4", "r12_4", "r15_4", "r15_8"]


@functools.lru_cache(maxsize=None)
def _topology(name):
    if name.startswith("vb"):
        return fb.variable_benchmark_topology(int(name[2:]))
    max_n, max_m = (int(v) for v in name[1:].split("_"))
    return fb.random_topology(np.random.default_rng(1000 + 17 * max_n + max_m), 12, max_n, max_m)


def _family(name):
    return "variable_benchmark" if name.startswith("vb") else "random"


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _inject_failures(topo, blocks, batch):
    """Statuses 1 (delta), 2 (F), 3 (G) and G-before-delta at one node at problems 0, 3 (last row of wavefront 0),
    4, 2049 and the last one.  Returns the statuses the construction implies."""
    live = [i for i, n in enumerate(topo.sd) if n > 0]
    j = live[-1]                                             # a node with a state
    e = next(e for e in range(topo.E) if topo.sd[topo.parents[e]] > 0)
    P = topo.parents[e]
    expect = np.zeros(batch, dtype=np.int32)
    cases = {0: 1, 3: 2, 4: 3, 2049: 33, batch - 1: 1 if batch % 2 else 2}
    for b, kind in cases.items():
        if kind == 1:
            blocks["delta"][j][b, 0] = 0.0
        elif kind == 2:
            blocks["Q"][j][b] = -1e6 * np.eye(topo.sd[j])
        elif kind == 3:
            blocks["R"][e][b] = -1e4 * np.eye(topo.cd[e])
        else:                                                # same node: the child edge's G before its delta
            blocks["R"][e][b] = -1e4 * np.eye(topo.cd[e])
            blocks["delta"][P][b, 0] = 0.0
        expect[b] = 3 if kind == 33 else kind
    return expect


def _problem_set(name, batch):
    """(topology, oracle nodes, oracle edges, oracle sol, gains, status) of a batch of distinct problems with
    failures injected (_inject_failures)."""
    topo = _topology(name)
    rng = np.random.default_rng(_seed(name, batch))
    blocks = fb.make_blocks(topo, batch, rng, _family(name))
    expect = _inject_failures(topo, blocks, batch)
    nodes, edges = fb.to_oracle(topo, blocks)
    sol, gains, st = oracle.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, nodes, edges, threads=THREADS)
    np.testing.assert_array_equal(st, expect)               # the oracle agrees with the construction
    return topo, nodes, edges, sol, gains, st


def _plan(topo, batch):
    """A plan whose output, work and status are views of arenas GUARD rows longer, filled with a sentinel."""
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    assert "tree_factor_solve_qw16" in s.kernel_name, s.kernel_name
    s._guarded = {}
    for name in ("output", "work", "status"):
        t = getattr(s, name)
        full = torch.empty((batch + GUARD,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        full.fill_(I_SENTINEL if t.dtype == torch.int32 else F_SENTINEL)
        setattr(s, name, full[:batch])
        s._guarded[name] = full
    return s


def _check_guards(s):
    for name, full in s._guarded.items():
        tail = full[s.batch:]
        want = I_SENTINEL if full.dtype == torch.int32 else F_SENTINEL
        assert bool((tail == want).all()), f"{name}: a row past the batch was written"


def _load(s, nodes, edges, maps):
    s.input.copy_(torch.from_numpy(maps.pack_input(s, nodes, edges)))


# ---- fused tree sweep: x, u, y, K, k, statuses of every problem -------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_tree_factor_solve_every_problem(name, batch):
    topo, nodes, edges, ref_sol, ref_gains, ref_st = _problem_set(name, batch)
    ok = np.flatnonzero(ref_st == 0)
    fb.assert_discriminates(ref_sol, TREE_TOL, rows=ok, what="sol")
    fb.assert_discriminates(ref_gains, TREE_TOL, rows=ok, what="gains")
    s = _plan(topo, batch)
    maps = fb.PlanMaps(s, topo)
    _load(s, nodes, edges, maps)
    out, st = s.factor_solve()
    torch.cuda.synchronize()
    _check_guards(s)
    np.testing.assert_array_equal(st.cpu().numpy(), ref_st)
    got_sol = out.cpu().numpy()[:, maps.sol_idx]
    got_gains = s.work.cpu().numpy()[:, maps.gains_idx]
    es = fb.block_rel_err(got_sol[ok], ref_sol[ok], maps.sol_blocks)
    eg = fb.block_rel_err(got_gains[ok], ref_gains[ok], maps.gains_blocks)
    print(f"tree_qw16 {name} batch {batch}: worst sol {es.max():.2e} (problem {ok[es.argmax()]}), "
          f"gains {eg.max():.2e}")
    assert es.max() <= TREE_TOL and eg.max() <= TREE_TOL, (ok[es.argmax()], ok[eg.argmax()])


# ---- fused sweep with workspace export: every LQR::Workspace field against the general engine --------------------
def _workspace_fields(s, topo):
    """Index vector into one problem's work arena of every LQR::Workspace field the export writes, and the
    start of each field in it (G_factor / F_factor: lower triangles only, as test_gpu_tree compares them)."""
    max_n = max(topo.sd)
    parts = []
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        o = s.offset(1, 1, e)
        low_m = np.flatnonzero(np.tril(np.ones((m, m), dtype=bool)).T.reshape(-1))
        parts += [o + np.arange(nc * nc), o + max_n * max_n + np.arange(m * np_),
                  o + max_n * max_n + m * np_ + low_m, o + max_n * max_n + m * np_ + m * m + np.arange(m)]
    for j, n in enumerate(topo.sd):
        o = s.offset(1, 0, j)
        low_n = np.flatnonzero(np.tril(np.ones((n, n), dtype=bool)).T.reshape(-1))
        parts += [o + np.arange(n * n), o + n * n + low_n, o + 2 * n * n + np.arange(3 * n)]
    parts = [p for p in parts if p.size]
    starts = np.cumsum([0] + [p.size for p in parts[:-1]])
    return np.concatenate(parts).astype(np.int64), starts


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", ["vb2", "r4_2", "r9_3", "r15_4", "r15_8"])
def test_tree_workspace_export_every_problem(name, batch):
    """sip_lqr_tree_factor_solve_workspace against sip_lqr_tree_factor + sip_lqr_tree_solve of the general
    engine, the comparison of test_gpu_tree.test_fused_sweep_writes_every_workspace_field at full batch (the
    15-state classes: the export instantiation spills)."""
    topo, nodes, edges, ref_sol, _, ref_st = _problem_set(name, batch)
    ok = np.flatnonzero(ref_st == 0)
    s = _plan(topo, batch)
    maps = fb.PlanMaps(s, topo)
    _load(s, nodes, edges, maps)
    idx, starts = _workspace_fields(s, topo)
    s.factor(); s.solve()
    torch.cuda.synchronize()
    want, want_out = s.work.cpu().numpy()[:, idx], s.output.cpu().numpy()
    fb.assert_discriminates(want, TREE_TOL, rows=ok, what="workspace")
    s.work.fill_(F_SENTINEL); s.output.fill_(F_SENTINEL); s.status.fill_(I_SENTINEL)
    s.factor_solve(workspace=True)
    torch.cuda.synchronize()
    _check_guards(s)
    np.testing.assert_array_equal(s.status.cpu().numpy(), ref_st)
    got = s.work.cpu().numpy()[:, idx]
    ew = fb.block_rel_err(got[ok], want[ok], starts)
    eo = fb.block_rel_err(s.output.cpu().numpy()[ok][:, maps.sol_idx], want_out[ok][:, maps.sol_idx],
                          maps.sol_blocks)
    print(f"tree_qw16 export {name} batch {batch}: worst workspace field {ew.max():.2e} "
          f"(problem {ok[ew.argmax()]}), output {eo.max():.2e}")
    assert ew.max() <= TREE_TOL and eo.max() <= TREE_TOL


# ---- tree multi-rhs solve: every column of every problem -----------------------------------------------------
COLUMNS = [1, 8, 11, 17]


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", ["vb2", "r4_2", "r9_3", "r12_4", "r15_8"])
def test_tree_solve_multi_every_column(name, batch):
    """1, 8, 11 and 17 columns (8 columns per wavefront up to 10 states, 4 above: the last grid.y group is partial
    for 11 and 17), each column against the oracle on its own right-hand side; failed problems keep their output
    columns (include/sip_lqr_amd.h); the column-batch past the last column stays untouched."""
    topo, nodes, edges, _, _, ref_st = _problem_set(name, batch)
    ok, bad = np.flatnonzero(ref_st == 0), np.flatnonzero(ref_st != 0)
    rng = np.random.default_rng(_seed(name, batch, "rhs"))
    rhs = [fb.make_rhs(topo, batch, rng) for _ in range(max(COLUMNS))]
    refs = []
    for r in rhs:
        n2, e2 = fb.with_rhs(topo, nodes, edges, r)
        sol, _, st = oracle.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, n2, e2, threads=THREADS,
                                       want_gains=False)
        np.testing.assert_array_equal(st, ref_st)
        refs.append(sol)
    for r in refs:
        fb.assert_discriminates(r, TREE_TOL, rows=ok, what="column")
    s = _plan(topo, batch)
    maps = fb.PlanMaps(s, topo)
    _load(s, nodes, edges, maps)
    s.factor()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(s.status.cpu().numpy(), ref_st)
    rhs_dev = torch.from_numpy(np.stack([maps.pack_rhs(s, r) for r in rhs])).to(s.device)
    worst = 0.0
    for ncols in COLUMNS:
        full = torch.full((ncols + 1, batch, s.output.shape[1]), F_SENTINEL, dtype=torch.float64, device=s.device)
        out = s.solve_multi(rhs_dev[:ncols].contiguous(), out_cols=full[:ncols])
        torch.cuda.synchronize()
        assert s.multi_kernel_name.startswith("tree_solve_mrhs_qw16"), s.multi_kernel_name
        full_h = full.cpu().numpy()
        assert (full_h[ncols] == F_SENTINEL).all(), "the column-batch past the last column was written"
        assert (full_h[:ncols, bad] == F_SENTINEL).all(), "a failed problem's output column was written"
        for col in range(ncols):
            e = fb.block_rel_err(full_h[col][ok][:, maps.sol_idx], refs[col][ok], maps.sol_blocks)
            assert e.max() <= TREE_TOL, (ncols, col, int(ok[e.argmax()]), float(e.max()))
            worst = max(worst, float(e.max()))
        _check_guards(s)
    print(f"{s.multi_kernel_name} {name} batch {batch}: worst column error {worst:.2e}")


# ---- theta Schur complement on tree plans ----------------------------------------------------------------------
def _theta_dims(topology, p):
    if topology == "nonuniform_chain":
        sd, cd = [4, 6, 5, 3, 6, 4, 5], [2, 3, 1, 2, 3, 2]
        return KKTDims(list(range(6)), list(range(1, 7)), sd, cd, node_c=[1, 0, 2, 0, 1, 0, 2],
                       node_g=[0, 2, 0, 1, 0, 0, 3], edge_c=[1, 2, 0, 1, 1, 0], edge_g=[2, 0, 1, 1, 0, 2], theta_dim=p)
    sd, cd = [5, 4, 6, 3, 5, 4, 6], [2, 3, 1, 2, 2, 3]
    return KKTDims([0, 0, 1, 1, 2, 4], [1, 2, 3, 4, 5, 6], sd, cd, node_c=[0, 1, 0, 2, 0, 1, 1],
                   node_g=[1, 0, 2, 0, 1, 0, 2], edge_c=[1, 0, 2, 1, 0, 1], edge_g=[0, 2, 1, 0, 1, 1], theta_dim=p)


def _kkt_plan(dims, batch):
    from sip_optimal_control_amd import BatchedNewtonKKT
    return BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                            batch=batch, root=dims.root, theta_dim=dims.p)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


@pytest.mark.parametrize("topology", ["nonuniform_chain", "branching_tree"])
def test_tree_theta_every_problem(monkeypatch, topology):
    from tests import reference_kkt_problems as rk
    dims, batch, p = _theta_dims(topology, 8), 4096, 8
    model, w, r1, r2, r3, rhs, theta_model = rk.newton_kkt_problem(dims, seed=31, batch=batch, r2_max=1e2)
    bad = [3, 2050]
    for q in bad:                                            # an indefinite Schur complement: status 7
        theta_model[q] = rk.initialize_theta_model(dims, -50.0)
    o = KKTOracle(dims)
    ref = np.zeros((batch, dims.full_dim))
    for q in range(batch):
        st = o.factor_theta(model[q], theta_model[q], w[q], r1[q], r2[q], r3[q])
        assert st == (7 if q in bad else 0), (q, st)
        if st == 0:
            ref[q] = o.solve_theta(model[q], theta_model[q], rhs[q])
    ok = np.setdiff1d(np.arange(batch), bad)
    fb.assert_discriminates(ref, 1e-8, rows=ok, what="theta")
    d = _dev(model, theta_model, w, r1, r2, r3, rhs)
    for multi in ("1", "0"):
        monkeypatch.setenv("SIP_KKT_THETA_TREE_MULTI", multi)
        kkt = _kkt_plan(dims, batch)
        assert kkt.kernel_name.startswith("tree:general")
        assert ("tree multi-rhs" in kkt.kernel_name) == (multi == "1")
        status = kkt.factor_theta(*d[:6]).cpu().numpy()
        expect = np.zeros(batch, dtype=status.dtype)
        expect[bad] = 7
        np.testing.assert_array_equal(status, expect)
        full = torch.full((batch + 1, dims.full_dim), F_SENTINEL, dtype=torch.float64, device="cuda")
        got = kkt.solve_theta(d[0], d[1], d[6], sol=full[:batch]).cpu().numpy()
        torch.cuda.synchronize()
        assert (full[batch] == F_SENTINEL).all() and (got[bad] == F_SENTINEL).all()
        err = (np.abs(got[ok] - ref[ok]).max(axis=1) / np.abs(ref[ok]).max(axis=1)).max()
        print(f"theta {topology} p={p} multi={multi} batch {batch}: worst {err:.2e}")
        assert err <= 1e-8


# ---- fp32 and fp64 C4 chains (n 32, m 8, T 100) ----------------------------------------------------------------
C4 = (32, 8, 100)
FP32_TOL, FP64_TOL = 1e-4, 1e-9


def _rel_rows(a, b):
    scale = np.abs(b).max(axis=1)
    scale[scale == 0] = 1.0
    return np.abs(a - b).max(axis=1) / scale


@functools.lru_cache(maxsize=None)
def _c4_problem(dtype_name):
    from sip_optimal_control_amd import ChainShape, synthetic
    dtype = getattr(torch, dtype_name)
    mats, vecs = synthetic.make_chain_batch(ChainShape(*C4), 4096, seed=4096 + len(dtype_name), device="cuda:0",
                                            dtype=dtype, cross_term=0.01)
    ref = oracle.chain_batch(*C4, mats.double().cpu().numpy(), vecs.double().cpu().numpy(), threads=THREADS)
    return mats, vecs, ref


@pytest.mark.parametrize("dtype_name,variant", [("float32", "mt16"), ("float32", "mf32"), ("float64", "mt16")])
def test_c4_every_problem(monkeypatch, dtype_name, variant):
    """Every one of the 4096 C4 problems against oracle.chain_batch (fp32: on the fp32-rounded problem)."""
    from sip_optimal_control_amd import BatchedChainLQR
    if variant != "mt16":
        monkeypatch.setenv("SIP_LQR_VARIANT", variant)
    mats, vecs, (ref_sol, ref_gains, ref_st) = _c4_problem(dtype_name)
    tol = FP32_TOL if dtype_name == "float32" else FP64_TOL
    assert (ref_st == 0).all()
    fb.assert_discriminates(ref_sol, tol, what="sol")
    fb.assert_discriminates(ref_gains, tol, what="gains")
    solver = BatchedChainLQR(*C4, 4096, dtype=mats.dtype)
    assert variant in solver.kernel_name, solver.kernel_name
    sol, gains, status = solver.factor_solve(mats, vecs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_st)
    es = _rel_rows(sol.double().cpu().numpy(), ref_sol)
    eg = _rel_rows(gains.double().cpu().numpy(), ref_gains)
    print(f"{solver.kernel_name} C4 batch 4096: worst sol {es.max():.2e} (problem {es.argmax()}), "
          f"gains {eg.max():.2e} (problem {eg.argmax()})")
    assert es.max() < tol and eg.max() < tol


# ---- Newton-KKT step ---------------------------------------------------------------------------------------------
def _kkt_every_problem(dims, batch, seed):
    from sip_optimal_control_amd import BatchedNewtonKKT, synthetic
    dd = dict(parents=dims.parents, children=dims.children, state_dims=dims.sd, control_dims=dims.cd,
              node_c_dims=dims.ncd, node_g_dims=dims.ngd, edge_c_dims=dims.ecd, edge_g_dims=dims.egd)
    kkt = BatchedNewtonKKT(batch=batch, root=dims.root, **dd)
    data = synthetic.make_newton_kkt_batch(kkt, seed=seed, r2_max=1e2, **dd)
    full = torch.full((batch + 1, dims.kkt_dim), F_SENTINEL, dtype=torch.float64, device=kkt.device)
    sol, status = kkt.factor_solve(*data, sol=full[:batch])
    torch.cuda.synchronize()
    assert (full[batch] == F_SENTINEL).all()
    model, w, r1, r2, r3, rhs = [a.cpu().numpy() for a in data]
    o = KKTOracle(dims)
    ref, ref_st = o.batch(model, w, r1, r2, r3, rhs, threads=THREADS)
    assert (ref_st == 0).all()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_st)
    fb.assert_discriminates(ref, 1e-9, what="kkt")
    got = sol.cpu().numpy()
    err = _rel_rows(got, ref)
    res = np.array([np.linalg.norm(o.add_Kx_to_y(model[q], w[q], r1[q], r2[q], r3[q], got[q]) - rhs[q]) /
                    np.linalg.norm(rhs[q]) for q in range(batch)])
    print(f"newton-kkt {kkt.kernel_name} batch {batch}: worst sol {err.max():.2e} (problem {err.argmax()}), "
          f"worst residual {res.max():.2e} (oracle operator)")
    assert err.max() <= 1e-9 and res.max() < 1e-9


def test_newton_kkt_f1_every_problem():
    """The f1 benchmark shape (n 12, m 4, T 50, c 6, g 8), all 4096 problems; K * sol - rhs through the oracle's
    operator, not the GPU one under test."""
    from tests import reference_kkt_problems as rk
    _kkt_every_problem(rk.newton_kkt_dims(12, 4, 50), 4096, seed=5)


def test_newton_kkt_tree_every_problem():
    _kkt_every_problem(_theta_dims("branching_tree", 0), 4093, seed=6)

"""The factorization and the single-right-hand-side solve of trees as separate sweeps on the size-class kernels
(sip_lqr_tree_factor_fused / sip_lqr_tree_solve_fused: the FACTOR_ONLY instantiation of csrc/tree_qw16.hpp and the
SINGLE one of csrc/tree_mrhs_qw16.hpp), at full batch against the CPU oracle and the general engine.

Every batch is 4096 (or 4093: a partial last wavefront) distinct problems with failures injected (statuses 1-3 and
G-before-delta, tests/test_gpu_full_batch._inject_failures), every comparison first asserts that it can tell
neighbouring problems apart, and rows past the end of every arena must come back bitwise unchanged.  The tolerance
is that of the tree kernels, 1e-10 relative to the block max.  The worst measured error of every comparison is
printed."""
import functools

import numpy as np
import pytest

import full_batch_problems as fb
from oracle import oracle
from test_gpu_full_batch import (BATCHES, F_SENTINEL, I_SENTINEL, THREADS, TOPOLOGIES, TREE_TOL, _check_guards,
                                 _load, _plan, _problem_set, _seed, _topology)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def _cached_problem_set(name, batch):
    return _problem_set(name, batch)


def _setup(name, batch):
    topo, nodes, edges, sol, gains, st = _cached_problem_set(name, batch)
    s = _plan(topo, batch)
    maps = fb.PlanMaps(s, topo)
    _load(s, nodes, edges, maps)
    return topo, nodes, edges, sol, gains, st, s, maps


def _compare(s, maps, ref_sol, ref_gains, ok, what):
    """x, y, u of the output arena and K, k of the work arena against the oracle: worst (sol, gains) error."""
    es = fb.block_rel_err(s.output.cpu().numpy()[ok][:, maps.sol_idx], ref_sol[ok], maps.sol_blocks)
    eg = fb.block_rel_err(s.work.cpu().numpy()[ok][:, maps.gains_idx], ref_gains[ok], maps.gains_blocks)
    assert es.max() <= TREE_TOL, (what, "sol", int(ok[es.argmax()]), float(es.max()))
    assert eg.max() <= TREE_TOL, (what, "gains", int(ok[eg.argmax()]), float(eg.max()))
    return float(es.max()), float(eg.max())


def _factor_fields(s, topo):
    """Index vector into one problem's work arena of the fields sip_lqr_tree_factor writes (W, K, G_factor per
    edge; V, F_factor, sqrt_delta, sqrt_delta_inv per node; G_factor / F_factor: lower triangles), and the start
    of each field in it."""
    max_n = max(topo.sd)
    parts = []
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        o = s.offset(1, 1, e)
        low_m = np.flatnonzero(np.tril(np.ones((m, m), dtype=bool)).T.reshape(-1))
        parts += [o + np.arange(nc * nc), o + max_n * max_n + np.arange(m * np_), o + max_n * max_n + m * np_ + low_m]
    for j, n in enumerate(topo.sd):
        o = s.offset(1, 0, j)
        low_n = np.flatnonzero(np.tril(np.ones((n, n), dtype=bool)).T.reshape(-1))
        parts += [o + np.arange(n * n), o + n * n + low_n, o + 2 * n * n + np.arange(2 * n)]
    parts = [p for p in parts if p.size]
    starts = np.cumsum([0] + [p.size for p in parts[:-1]])
    return np.concatenate(parts).astype(np.int64), starts


def _solve_slots(s, topo):
    """Index vector into one problem's work arena of v (per node) and k (per edge): what a solve writes there."""
    max_n = max(topo.sd)
    parts = [s.offset(1, 0, j) + 2 * n * n + 2 * n + np.arange(n) for j, n in enumerate(topo.sd)]
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        parts.append(s.offset(1, 1, e) + max_n * max_n + m * np_ + m * m + np.arange(m))
    return np.concatenate(parts).astype(np.int64)


def _rhs_slots(s, topo):
    """Index vector into one problem's input arena of q, c (per node) and r (per edge)."""
    parts = [s.offset(0, 0, j) + n * n + np.arange(2 * n) for j, n in enumerate(topo.sd)]
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        parts.append(s.offset(0, 1, e) + nc * np_ + nc * m + np_ * m + m * m + np.arange(m))
    return np.concatenate(parts).astype(np.int64)


def _oracle_with_rhs(topo, nodes, edges, rhs, ref_st):
    n2, e2 = fb.with_rhs(topo, nodes, edges, rhs)
    sol, gains, st = oracle.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, n2, e2, threads=THREADS)
    np.testing.assert_array_equal(st, ref_st)
    return n2, e2, sol, gains


# ---- 1 + 7: factor_fused then solve_fused, every problem against the oracle; failed problems keep their outputs --
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_split_every_problem(name, batch):
    topo, nodes, edges, ref_sol, ref_gains, ref_st, s, maps = _setup(name, batch)
    ok, bad = np.flatnonzero(ref_st == 0), np.flatnonzero(ref_st != 0)
    fb.assert_discriminates(ref_sol, TREE_TOL, rows=ok, what="sol")
    fb.assert_discriminates(ref_gains, TREE_TOL, rows=ok, what="gains")
    assert s.split_kernel_name == "tree_factor_qw16<{0}>/f64 + tree_solve_qw16<{0}>/f64".format(
        s.kernel_name[s.kernel_name.index("<") + 1:s.kernel_name.index(">")]), s.split_kernel_name
    s.factor_fused()
    s.solve_fused()
    torch.cuda.synchronize()
    _check_guards(s)
    np.testing.assert_array_equal(s.status.cpu().numpy(), ref_st)
    assert (s.output.cpu().numpy()[bad] == F_SENTINEL).all(), "a failed problem's output was written"
    es, eg = _compare(s, maps, ref_sol, ref_gains, ok, name)
    print(f"{s.split_kernel_name} {name} batch {batch}: worst sol {es:.2e}, gains {eg:.2e}")


# ---- 2 + 3: the factor state against the general engine; the factor reads only the matrices -----------------------
@pytest.mark.parametrize("name", ["vb0", "vb2", "r4_2", "r9_3", "r15_4", "r15_8"])
def test_factor_state_and_inputs_read(name):
    batch = 4096
    topo, nodes, edges, _, _, ref_st, s, maps = _setup(name, batch)
    ok = np.flatnonzero(ref_st == 0)
    idx, starts = _factor_fields(s, topo)
    s.factor()
    torch.cuda.synchronize()
    want = s.work.cpu().numpy()[:, idx]
    fb.assert_discriminates(want[:, :], TREE_TOL, rows=ok, what="factor state")
    s.work.fill_(F_SENTINEL); s.status.fill_(I_SENTINEL)
    s.factor_fused()
    torch.cuda.synchronize()
    _check_guards(s)
    assert (s.output == F_SENTINEL).all(), "the factor wrote the output arena"
    np.testing.assert_array_equal(s.status.cpu().numpy(), ref_st)
    work1 = s._guarded["work"].cpu().numpy().copy()
    ew = fb.block_rel_err(work1[:batch][ok][:, idx], want[ok], starts)
    assert ew.max() <= TREE_TOL, (int(ok[ew.argmax()]), float(ew.max()))
    # the same factor with q, c and r poisoned: the work arena and the statuses are bitwise the same
    rhs = torch.from_numpy(_rhs_slots(s, topo)).to(s.device)
    s.input[:, rhs] = float("nan")
    s.work.fill_(F_SENTINEL); s.status.fill_(I_SENTINEL)
    s.factor_fused()
    torch.cuda.synchronize()
    assert np.array_equal(s._guarded["work"].cpu().numpy().view(np.uint64), work1.view(np.uint64))
    np.testing.assert_array_equal(s.status.cpu().numpy(), ref_st)
    assert (s.output == F_SENTINEL).all()
    print(f"{s.split_kernel_name} factor state {name}: worst field {ew.max():.2e} (problem {ok[ew.argmax()]})")


# ---- 4 + 5: the solve writes only v, k and the outputs; one factor, several right-hand sides ----------------------
@pytest.mark.parametrize("name", ["vb1", "r6_3", "r12_4", "r15_8"])
def test_repeated_solves_write_only_v_k(name):
    batch = 4093
    topo, nodes, edges, _, _, ref_st, s, maps = _setup(name, batch)
    ok, bad = np.flatnonzero(ref_st == 0), np.flatnonzero(ref_st != 0)
    s.factor_fused()
    torch.cuda.synchronize()
    slots = _solve_slots(s, topo)
    rng = np.random.default_rng(_seed(name, batch, "split rhs"))
    worst = [0.0, 0.0]
    for rep in range(3):
        rhs = fb.make_rhs(topo, batch, rng)
        n2, e2, sol, gains = _oracle_with_rhs(topo, nodes, edges, rhs, ref_st)
        fb.assert_discriminates(sol, TREE_TOL, rows=ok, what="sol")
        _load(s, n2, e2, maps)
        before = s._guarded["work"].cpu().numpy().copy()
        s.solve_fused()
        torch.cuda.synchronize()
        _check_guards(s)
        after = s._guarded["work"].cpu().numpy()
        keep = np.ones(before.shape[1], dtype=bool)
        keep[slots] = False
        assert np.array_equal(after[:, keep].view(np.uint64), before[:, keep].view(np.uint64)), \
            "the solve wrote the work arena outside v and k"
        assert np.array_equal(after[bad].view(np.uint64), before[bad].view(np.uint64)), \
            "the solve wrote a failed problem's work arena"
        assert (s.output.cpu().numpy()[bad] == F_SENTINEL).all()
        es, eg = _compare(s, maps, sol, gains, ok, (name, rep))
        worst = [max(worst[0], es), max(worst[1], eg)]
    print(f"{s.split_kernel_name} {name} batch {batch}, 3 solves after one factor: worst sol {worst[0]:.2e}, "
          f"gains {worst[1]:.2e}")


# ---- 6: every producer of the factor state serves every solve --------------------------------------------------
@pytest.mark.parametrize("name", ["vb2", "r10_4"])
def test_factor_producers_and_solvers_interchange(name):
    batch = 4096
    topo, nodes, edges, ref_sol, ref_gains, ref_st, s, maps = _setup(name, batch)
    ok = np.flatnonzero(ref_st == 0)
    worst = {}

    def fresh():
        s.work.fill_(F_SENTINEL); s.output.fill_(F_SENTINEL); s.status.fill_(I_SENTINEL)

    def check(what):
        torch.cuda.synchronize()
        _check_guards(s)
        np.testing.assert_array_equal(s.status.cpu().numpy(), ref_st)
        worst[what] = _compare(s, maps, ref_sol, ref_gains, ok, what)

    fresh(); s.factor(); s.solve_fused(); check("factor -> solve_fused")
    fresh(); s.factor_fused(); s.solve(); check("factor_fused -> solve")
    fresh(); s.factor_solve(workspace=True); s.output.fill_(F_SENTINEL); s.solve_fused()
    check("factor_solve_workspace -> solve_fused")
    # factor_fused -> solve_multi, 8 columns, each against the oracle on its own right-hand side
    fresh(); s.factor_fused()
    rng = np.random.default_rng(_seed(name, batch, "split multi"))
    rhs = [fb.make_rhs(topo, batch, rng) for _ in range(8)]
    out = s.solve_multi(torch.from_numpy(np.stack([maps.pack_rhs(s, r) for r in rhs])).to(s.device))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(s.status.cpu().numpy(), ref_st)
    out = out.cpu().numpy()
    em = 0.0
    for col, r in enumerate(rhs):
        _, _, sol, _ = _oracle_with_rhs(topo, nodes, edges, r, ref_st)
        e = fb.block_rel_err(out[col][ok][:, maps.sol_idx], sol[ok], maps.sol_blocks)
        assert e.max() <= TREE_TOL, (col, int(ok[e.argmax()]), float(e.max()))
        em = max(em, float(e.max()))
    worst["factor_fused -> solve_multi(8)"] = (em, 0.0)
    for k, (es, eg) in worst.items():
        print(f"{name}: {k}: worst sol {es:.2e}, gains {eg:.2e}")


# ---- 8: fallback and names -------------------------------------------------------------------------------------
def _small_problem(topo, batch, seed):
    blocks = fb.make_blocks(topo, batch, np.random.default_rng(seed), "random")
    return fb.to_oracle(topo, blocks)


def _bitwise_against_general(s, maps, nodes, edges):
    _load(s, nodes, edges, maps)
    s.factor(); s.solve()
    torch.cuda.synchronize()
    want = [t.cpu().numpy().copy() for t in (s.work, s.output, s.status)]
    s.work.zero_(); s.output.zero_(); s.status.fill_(-1)
    s.factor_fused(); s.solve_fused()
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (s.work, s.output, s.status)]
    for w, g in zip(want, got):
        assert np.array_equal(w.view(np.uint8), g.view(np.uint8))
    assert (want[2] == 0).all()


def test_fallback_beyond_size_classes_is_the_general_engine():
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    topo = fb.random_topology(np.random.default_rng(5), 6, 16, 3)  # a 16-state node: no size class
    batch = 37
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    assert s.split_kernel_name == "tree_generic/f64" and s.kernel_name == "tree_generic/f64"
    assert s._lib.sip_lqr_tree_fused_scratch_bytes(s._plan) == 0
    nodes, edges = _small_problem(topo, batch, 6)
    _bitwise_against_general(s, fb.PlanMaps(s, topo), nodes, edges)


def test_fallback_with_general_variant(monkeypatch):
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    topo = _topology("r9_3")
    batch = 64
    monkeypatch.setenv("SIP_LQR_TREE", "general")
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    monkeypatch.delenv("SIP_LQR_TREE")
    assert s.split_kernel_name == "tree_generic/f64"
    nodes, edges = _small_problem(topo, batch, 7)
    _bitwise_against_general(s, fb.PlanMaps(s, topo), nodes, edges)
    fitting = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    assert fitting.split_kernel_name == "tree_factor_qw16<9,3>/f64 + tree_solve_qw16<9,3>/f64"


# ---- 9: graph capture ------------------------------------------------------------------------------------------
def test_graph_capture_matches_eager():
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    topo = _topology("r8_4")
    batch = 1031
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    maps = fb.PlanMaps(s, topo)
    eager = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    nodes, edges = _small_problem(topo, batch, 8)
    _load(s, nodes, edges, maps)
    s.factor_fused(); s.solve_fused()                 # scratch allocated outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        s.factor_fused()
        s.solve_fused()
    torch.cuda.synchronize()
    for seed in (9, 10):
        nodes, edges = _small_problem(topo, batch, seed)
        _load(s, nodes, edges, maps)
        _load(eager, nodes, edges, maps)
        s.output.zero_(); s.status.fill_(-1)
        graph.replay()
        eager.factor_fused(); eager.solve_fused()
        torch.cuda.synchronize()
        for a, b in ((s.work, eager.work), (s.output, eager.output), (s.status, eager.status)):
            assert torch.equal(a.view(torch.uint8) if a.dtype != torch.int32 else a,
                               b.view(torch.uint8) if b.dtype != torch.int32 else b)
        sol, _, st = oracle.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, nodes, edges, threads=THREADS)
        np.testing.assert_array_equal(s.status.cpu().numpy(), st)
        ok = np.flatnonzero(st == 0)
        e = fb.block_rel_err(s.output.cpu().numpy()[ok][:, maps.sol_idx], sol[ok], maps.sol_blocks)
        assert e.max() <= TREE_TOL

"""sip_lqr_tree_solve_multi: several right-hand sides against ONE tree factorization (the LQR part of the
reference's solve_stagewise_kkt_matrix, helpers.cpp:521-665), on the size-class kernel
(csrc/tree_mrhs_qw16.hpp) and on the general engine.  Every column against the oracle run with that
column's q, r, c patched into the problem: x, u, y to 1e-10 relative, KKT residual to 1e-12 relative."""
import copy

import numpy as np
import pytest

import reference_problems as rp
from oracle import dense_kkt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _solver(prob, batch=1):
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    return BatchedTreeLQR(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"], batch=batch)


def _random_tree(rng, N, max_n, max_m, zero_nodes=True):
    """A random tree whose largest state / control dimensions are max_n / max_m, two nodes of dimension 0."""
    parents = [int(rng.integers(0, e + 1)) for e in range(N - 1)]
    children = list(range(1, N))
    sd = [int(rng.integers(1, max_n + 1)) for _ in range(N)]
    cd = [int(rng.integers(1, max_m + 1)) for _ in range(N - 1)]
    sd[0] = max_n
    cd[int(rng.integers(0, N - 1))] = max_m
    if zero_nodes:
        for i in rng.choice(np.arange(1, N), size=2, replace=False):
            sd[int(i)] = 0
    return parents, children, sd, cd


def _random_blocks(rng, parents, children, sd, cd):
    blocks = {k: [] for k in ("Q", "M", "R", "q", "r", "A", "B", "c", "delta")}
    for n in sd:
        S = rng.normal(size=(n, n))
        blocks["Q"].append(S.T @ S + 1e-3 * np.eye(n))
        blocks["q"].append(rng.normal(size=n))
        blocks["c"].append(rng.normal(size=n))
        blocks["delta"].append(1e-3 + 0.1 * rng.random(n))
    for e, m in enumerate(cd):
        np_, nc = sd[parents[e]], sd[children[e]]
        G = rng.normal(size=(m, m))
        blocks["A"].append(0.3 * rng.normal(size=(nc, np_)))
        blocks["B"].append(0.3 * rng.normal(size=(nc, m)))
        blocks["M"].append(0.05 * rng.normal(size=(np_, m)))
        blocks["R"].append(G.T @ G + np.eye(m))
        blocks["r"].append(rng.normal(size=m))
    return blocks


def _random_rhs(rng, sd, cd):
    return {"q": [rng.normal(size=n) for n in sd], "c": [rng.normal(size=n) for n in sd],
            "r": [rng.normal(size=m) for m in cd]}


def _check_columns(oracle_lib, s, probs, cols, out_cols, tol=1e-10, res_tol=1e-12, skip=()):
    """Returns the worst (error of x, u, y; KKT residual), both relative as they are asserted."""
    worst, worst_res = 0.0, 0.0
    for col, rhs in enumerate(cols):
        for b, blocks in enumerate(probs):
            if b in skip:
                continue
            patched = dict(blocks)
            patched.update({k: rhs[b][k] for k in ("q", "c", "r")})
            lqr = oracle_lib.TreeLQR(s.parents, s.children, s.state_dims, s.control_dims, patched)
            assert lqr.factor() == 0
            xo, uo, yo = lqr.solve()
            x, u, y = s.unpack_solution(b, output=out_cols[col])
            for a, bb in list(zip(x, xo)) + list(zip(u, uo)) + list(zip(y, yo)):
                np.testing.assert_allclose(a, bb, rtol=0, atol=tol * max(1.0, np.abs(bb).max(initial=0.0)))
                worst = max(worst, float(np.abs(a - bb).max(initial=0.0) / max(1.0, np.abs(bb).max(initial=0.0))))
            scale = max(1.0, np.sqrt(sum(float(v @ v) for k in ("q", "c", "r") for v in rhs[b][k])))
            res = dense_kkt.residual_norm(s.parents, s.children, s.state_dims, s.control_dims, patched, x, u, y)
            assert res / scale < res_tol, (col, b, res)
            worst_res = max(worst_res, res / scale)
    return worst, worst_res


# (largest state dim, largest control dim) -> the size class the tree lands in: all of kClasses (csrc/tree_qw16.hip),
# each at its own largest dimensions, which no cheaper class holds (tests/test_tree_plan.py keeps the lists equal)
CLASSES = [(4, 2, "<4,2>"), (6, 3, "<6,3>"), (8, 4, "<8,4>"), (9, 3, "<9,3>"), (10, 4, "<10,4>"), (12, 4, "<12,4>"),
           (15, 4, "<15,4>"), (15, 8, "<15,8>")]


@pytest.mark.parametrize("max_n,max_m,cls", CLASSES)
@pytest.mark.parametrize("num_rhs", [1, 3, 8, 11, 17])
def test_every_column_matches_the_oracle(oracle_lib, max_n, max_m, cls, num_rhs):
    rng = np.random.default_rng(100 * max_n + num_rhs)
    parents, children, sd, cd = _random_tree(rng, 9, max_n, max_m)
    batch = 5
    probs = [_random_blocks(rng, parents, children, sd, cd) for _ in range(batch)]
    s = _solver(dict(parents=parents, children=children, state_dims=sd, control_dims=cd), batch=batch)
    assert s.multi_kernel_name == "tree_solve_mrhs_qw16" + cls + "/f64"
    s.pack(probs)
    assert (s.factor().cpu().numpy() == 0).all()
    cols = [[_random_rhs(rng, sd, cd) for _ in range(batch)] for _ in range(num_rhs)]
    out = s.solve_multi(s.pack_rhs(cols))
    torch.cuda.synchronize()
    err, res = _check_columns(oracle_lib, s, probs, cols, out)
    print(f"tree multi-rhs {cls}, {num_rhs} columns: worst error {err:.2e} (bound 1e-10), residual {res:.2e} (bound 1e-12)")


@pytest.mark.parametrize("name", ["nonuniform_diagonal_delta", "branch_tree", "variable_dimension_branch",
                                  "five_node_variable_tree_eigen"])
def test_reference_fixtures(oracle_lib, name):
    prob = getattr(rp, name)()
    rng = np.random.default_rng(7)
    s = _solver(prob)
    s.pack([prob["blocks"]])
    assert int(s.factor()[0]) == 0
    cols = [[{k: prob["blocks"][k] for k in ("q", "c", "r")}]] + \
           [[_random_rhs(rng, prob["state_dims"], prob["control_dims"])] for _ in range(8)]
    out = s.solve_multi(s.pack_rhs(cols))
    torch.cuda.synchronize()
    _check_columns(oracle_lib, s, [prob["blocks"]], cols, out)


def _variable_tree(batch, seed):
    rng = np.random.default_rng(seed)
    return [rp.variable_benchmark_problem(2, 20, 8, 2, rng) for _ in range(batch)], rng


def test_one_column_equals_the_single_column_solve():
    probs, rng = _variable_tree(6, 3)
    s = _solver(probs[0], batch=len(probs))
    s.pack([p["blocks"] for p in probs])
    s.factor()
    out = s.solve_multi(s.pack_rhs([[{k: p["blocks"][k] for k in ("q", "c", "r")} for p in probs]]))
    single = s.solve().clone()
    torch.cuda.synchronize()
    a, b = out[0].cpu().numpy(), single.cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-13 * np.abs(b).max())


def test_factor_state_from_both_producers_and_work_untouched():
    probs, rng = _variable_tree(7, 4)
    p0 = probs[0]
    s = _solver(p0, batch=len(probs))
    s.pack([p["blocks"] for p in probs])
    rhs = s.pack_rhs([[_random_rhs(rng, p0["state_dims"], p0["control_dims"]) for _ in probs] for _ in range(5)])
    results = []
    for producer in ("factor", "factor_solve_workspace"):
        s.work.zero_()
        if producer == "factor":
            s.factor()
        else:
            s.factor_solve(workspace=True)
        torch.cuda.synchronize()
        before = s.work.clone()
        results.append(s.solve_multi(rhs).clone())
        torch.cuda.synchronize()
        assert torch.equal(before.view(torch.int64), s.work.view(torch.int64)), producer
    a, b = results[0].cpu().numpy(), results[1].cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.abs(a).max())


def test_failed_problems_keep_their_output_columns(oracle_lib):
    base = rp.default_chain(2, 1, 2)
    bad = copy.deepcopy(base)
    bad["blocks"]["delta"][2][0] = 0.0  # INVALID_DELTA (lqr_test.cpp:188-227)
    probs = [base["blocks"], bad["blocks"], base["blocks"]]
    s = _solver(base, batch=3)
    s.pack(probs)
    assert list(s.factor().cpu().numpy()) == [0, 1, 0]
    rng = np.random.default_rng(9)
    cols = [[_random_rhs(rng, base["state_dims"], base["control_dims"]) for _ in probs] for _ in range(3)]
    sentinel = torch.full((3, 3, s.out_len), 12345.0, dtype=torch.float64, device=s.device)
    out = s.solve_multi(s.pack_rhs(cols), out_cols=sentinel)
    torch.cuda.synchronize()
    assert (out[:, 1].cpu().numpy() == 12345.0).all()
    _check_columns(oracle_lib, s, probs, cols, out, skip=(1,))


@pytest.mark.parametrize("how", ["beyond_classes", "env"])
def test_general_fallback(oracle_lib, monkeypatch, how):
    rng = np.random.default_rng(11)
    if how == "env":
        monkeypatch.setenv("SIP_LQR_TREE", "general")
        parents, children, sd, cd = _random_tree(rng, 7, 6, 3)
    else:
        parents, children, sd, cd = _random_tree(rng, 7, 17, 3)
    batch = 3
    probs = [_random_blocks(rng, parents, children, sd, cd) for _ in range(batch)]
    s = _solver(dict(parents=parents, children=children, state_dims=sd, control_dims=cd), batch=batch)
    assert s.multi_kernel_name == "tree_generic/f64 column by column"
    s.pack(probs)
    assert (s.factor().cpu().numpy() == 0).all()
    cols = [[_random_rhs(rng, sd, cd) for _ in range(batch)] for _ in range(4)]
    before = s.work.clone()
    out = s.solve_multi(s.pack_rhs(cols))
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int64), s.work.view(torch.int64))
    _check_columns(oracle_lib, s, probs, cols, out)

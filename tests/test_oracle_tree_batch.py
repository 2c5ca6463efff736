"""oracle.tree_batch (lqr_oracle_tree_batch: many problems of one tree, OpenMP over problems) agrees bitwise with
the per-problem oracle.TreeLQR it batches: the reference's tree fixtures, random trees with zero-dimensional nodes,
every failure status, any thread count.  CPU only."""
import numpy as np
import pytest

import full_batch_problems as fb
import reference_problems as rp


def _stack(probs):
    """Per-problem blocks dicts -> blocks with a leading batch axis."""
    return {k: [np.stack([np.asarray(p[k][j], dtype=np.float64) for p in probs]) for j in range(len(probs[0][k]))]
            for k in probs[0]}


def _per_problem(oracle_lib, topo, blk, root=0):
    """(sol, gains, status) of TreeLQR, laid out as tree_batch lays them out."""
    lay = topo.layout
    lqr = oracle_lib.TreeLQR(topo.parents, topo.children, topo.sd, topo.cd, blk, root=root)
    sol, gains = np.zeros(lay.sol_len), np.zeros(lay.gains_len)
    st = lqr.factor()
    if st == 0:
        x, u, y = lqr.solve()
        for i, n in enumerate(topo.sd):
            sol[lay.x_off[i]:lay.x_off[i] + 2 * n] = np.concatenate([x[i], y[i]])
        for e, m in enumerate(topo.cd):
            sol[lay.u_off[e]:lay.u_off[e] + m] = u[e]
        K, k = lqr.gains()
        for e in range(topo.E):
            o, nk = lay.gains_off[e], K[e].size
            gains[o:o + nk] = K[e].reshape(-1, order="F")
            gains[o + nk:o + nk + k[e].size] = k[e]
    return sol, gains, st


def _agree(oracle_lib, topo, probs, threads, root=0):
    blocks = _stack(probs)
    nodes, edges = fb.to_oracle(topo, blocks)
    sol, gains, status = oracle_lib.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, nodes, edges,
                                               threads=threads, root=root)
    for b, blk in enumerate(probs):
        rsol, rgains, rst = _per_problem(oracle_lib, topo, blk, root)
        assert status[b] == rst, (b, status[b], rst)
        assert np.array_equal(sol[b], rsol) and np.array_equal(gains[b], rgains), b
    return status


@pytest.mark.parametrize("name", ["nonuniform_diagonal_delta", "branch_tree", "variable_dimension_branch",
                                  "five_node_variable_tree_eigen"])
def test_reference_fixtures(oracle_lib, name):
    prob = getattr(rp, name)()
    topo = fb.Topology(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"])
    assert _agree(oracle_lib, topo, [prob["blocks"]] * 3, threads=2).tolist() == [0, 0, 0]


@pytest.mark.parametrize("threads", [1, 3])
def test_random_trees_with_zero_dimensional_nodes(oracle_lib, threads):
    rng = np.random.default_rng(404)
    for N, max_n, max_m in [(7, 4, 2), (12, 9, 3), (9, 15, 8)]:
        topo = fb.random_topology(rng, N, max_n, max_m)
        assert 0 in topo.sd
        blocks = fb.make_blocks(topo, 11, rng)
        st = _agree(oracle_lib, topo, [fb.problem(blocks, b) for b in range(11)], threads)
        assert (st == 0).all()
    topo = fb.variable_benchmark_topology(2, T=20)
    blocks = fb.make_blocks(topo, 5, rng, family="variable_benchmark")
    assert (_agree(oracle_lib, topo, [fb.problem(blocks, b) for b in range(5)], threads) == 0).all()


def test_every_failure_status(oracle_lib):
    """Statuses 1, 2, 3 and G-before-delta at one node, between successful problems; INVALID_TOPOLOGY for the
    whole batch of a rejected topology."""
    p0 = rp.five_node_variable_tree_eigen()
    topo = fb.Topology(p0["parents"], p0["children"], p0["state_dims"], p0["control_dims"])
    probs = [rp.five_node_variable_tree_eigen()["blocks"] for _ in range(6)]
    probs[1]["delta"][3][0] = 0.0
    probs[2]["Q"][2] = -1e6 * np.eye(topo.sd[2])
    probs[3]["R"][0] = -1e4 * np.eye(topo.cd[0])
    probs[4]["R"][2] = -1e4 * np.eye(topo.cd[2])
    probs[4]["delta"][1][0] = 0.0                        # node 1: its child edge 2 (G) before its own delta
    probs[5]["q"][0] = probs[5]["q"][0] + 1.0
    assert _agree(oracle_lib, topo, probs, threads=3).tolist() == [0, 1, 2, 3, 3, 0]
    bad = fb.Topology([0, 0, 1, 1], [1, 1, 3, 4], topo.sd, topo.cd)     # node 1 twice, node 2 unreachable
    assert _agree(oracle_lib, bad, probs[:2], threads=2).tolist() == [4, 4]
    with pytest.raises(ValueError):
        oracle_lib.tree_batch([0, 7], [1, 2], [1, 1, 1], [1, 1], np.zeros((1, 12)), np.zeros((1, 10)))


def test_empty_batch_and_threads_beyond_the_batch(oracle_lib):
    rng = np.random.default_rng(3)
    topo = fb.random_topology(rng, 6, 5, 2)
    blocks = fb.make_blocks(topo, 2, rng)
    nodes, edges = fb.to_oracle(topo, blocks)
    sol, gains, st = oracle_lib.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, nodes[:0], edges[:0])
    assert sol.shape == (0, topo.layout.sol_len) and st.size == 0
    assert (_agree(oracle_lib, topo, [fb.problem(blocks, b) for b in range(2)], threads=8) == 0).all()

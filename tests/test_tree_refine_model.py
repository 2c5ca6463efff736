"""The residual of sip_lqr_tree_residual and the scheme of sip_lqr_tree_refine restated in numpy
(tests/tree_refine_cases.py), without a GPU: the numpy residual is tied to the oracle's dense KKT system, and the scheme
-- float64 residual, the CPU oracle's recursion as the correction solve -- meets the GPU test's cap
e <= 1e-9 + 3 e_ref on every cell tests/test_gpu_tree_refine.py runs, in the same number of rounds.  The cells on which
the model's error falls by at least 100x from round 1 to round 2 are recorded (tree_refine_cases.cells_with_a_drop):
there the GPU test asks for a drop of at least 10x.

Every model test prints "MODEL | tree <n,m> | axis | e by round | e_ref | norms by round (worst problem)", and where a
problem's residual norm rises from round 1 to round 2 (cost[1,1e4]: with a residual summed in plain float64, as this
model's is, both norms are below the residual's own rounding there; the kernel sums in head + tail pairs and does not
show it) the norms of that cell by problem."""
import numpy as np
import pytest

import extended_reference as xr
import full_batch_problems as fb
import hard_inputs as hi
import tree_refine_cases as tc
from oracle import dense_kkt


@pytest.mark.parametrize("name", list(tc.reference_trees()))
def test_the_numpy_residual_is_the_dense_kkt_system(name):
    """rho = Kmat z + b of dense_kkt.assemble (b = -rhs), reordered into the rhs layout, at a random z: signs and
    layout tied to the oracle's system, on the reference's four small trees."""
    prob = tc.reference_trees()[name]
    topo, blocks = tc.batched(prob, 3, seed=7)
    lay = topo.layout
    rng = np.random.default_rng(11)
    sol = rng.normal(size=(3, lay.sol_len))
    rho, mag = tc.residual(topo, blocks, None, sol, dt=np.float64)
    for b in range(3):
        one = fb.problem(blocks, b)
        Kmat, rhs, (xo, uo, yo) = dense_kkt.assemble(topo.parents, topo.children, topo.sd, topo.cd, one)
        z = np.zeros(Kmat.shape[0])
        for i, n in enumerate(topo.sd):
            z[xo[i]:xo[i] + n] = sol[b, lay.x_off[i]:lay.x_off[i] + n]
            z[yo[i]:yo[i] + n] = sol[b, lay.x_off[i] + n:lay.x_off[i] + 2 * n]
        for e, m in enumerate(topo.cd):
            z[uo[e]:uo[e] + m] = sol[b, lay.u_off[e]:lay.u_off[e] + m]
        dense = Kmat @ z - rhs
        # rows of assemble: stationarity per node, per edge, then the root's and every edge's dynamics row
        want = np.zeros(lay.sol_len)
        row = 0
        for i, n in enumerate(topo.sd):
            want[lay.x_off[i]:lay.x_off[i] + n] = dense[row:row + n]
            row += n
        for e, m in enumerate(topo.cd):
            want[lay.u_off[e]:lay.u_off[e] + m] = dense[row:row + m]
            row += m
        for node in [0] + [topo.children[e] for e in range(topo.E)]:
            n = topo.sd[node]
            want[lay.x_off[node] + n:lay.x_off[node] + 2 * n] = dense[row:row + n]
            row += n
        assert row == dense.size
        assert np.abs(rho[b] - want).max() <= 1e-12 * np.abs(want).max(), name
    assert (mag >= np.abs(rho)).all()


def test_term_counts_of_the_five_node_tree():
    """k by hand on one tree: node 1 (n = 1, children over edges 2 and 3 with m = 3, 1 and nc = 4, 2)."""
    prob = tc.reference_trees()["five_node"]
    topo = fb.Topology(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"])
    k, lay = tc.k(topo), topo.layout
    assert k[lay.x_off[1]] == 1 + 2 + (3 + 4) + (1 + 2)          # Q x, y and q, then M u + A^T y per child edge
    assert k[lay.x_off[0] + 3] == 3                               # the root's rho_c: x, delta y, c
    assert k[lay.x_off[3] + 4] == 1 + 3 + 3                       # rho_c of node 3 (edge 2): A x (np = 1), B u, x, dy, c
    assert k[lay.u_off[2]] == 1 + 3 + 4 + 1                       # rho_r of edge 2: M^T x, R u, B^T y, r


@pytest.mark.parametrize("axis", hi.AXES_TREE)
@pytest.mark.parametrize("dims", hi.TREES, ids=lambda d: "<%d,%d>" % d)
def test_model_meets_the_cap_on_the_tree_cells(dims, axis):
    cell = hi.tree_cell(*dims, axis)
    iterates, norms = tc.model_refine(cell, tc.ITERATIONS_F64)
    errs = [xr.err(z, cell.ext) for z in iterates]
    print("MODEL | tree <%d,%d> | %s | " % (dims + (axis,)) + " ".join(f"{e:.1e}" for e in errs) + f" | {cell.e_ref:.1e} | " +
          " ".join(f"{v:.2e}" for v in norms.max(axis=1)) +
          ("" if (norms[2] <= norms[1]).all() else " | norms not monotone after round 1: " +
           " ".join(f"{a:.2e}->{b:.2e}" for a, b in zip(norms[1], norms[2]))))
    assert (cell.ref_status == 0).all()
    assert errs[-1] <= tc.CAP + 3 * cell.e_ref, (dims, axis, errs, cell.e_ref)
    assert norms.shape == (tc.ITERATIONS_F64 + 1, hi.BATCH)
    # round 1 of the model is the oracle's own solve
    np.testing.assert_allclose(iterates[0], cell.ref_sol, rtol=0, atol=1e-12 * np.abs(cell.ref_sol).max())


def test_the_cells_with_a_drop_are_recorded():
    """The set the GPU test imports: computed from the model, a subset of the cells, and not empty -- the small-delta
    axes lose digits in the recursion and one round recovers them."""
    marked = tc.cells_with_a_drop()
    assert marked <= {(d, a) for d in hi.TREES for a in hi.AXES_TREE}
    print("DROP | " + " ".join("<%d,%d>/%s" % (d + (a,)) for d, a in sorted(marked)))
    assert any(a == "delta[1e-9,1e-7]" for _, a in marked), marked


def test_the_numpy_residual_vanishes_at_the_extended_solution():
    cell = hi.tree_cell(*hi.TREES[0], hi.BENIGN)
    rho, mag = tc.residual(cell.topo, cell.blocks, None, cell.ext)
    assert (np.abs(rho) <= 4 * tc.U * mag).all(), float((np.abs(rho) / np.where(mag > 0, mag, 1)).max())

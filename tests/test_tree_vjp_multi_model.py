"""The gradient formulas of include/sip_lqr_amd.h (sip_lqr_tree_vjp_multi), as tests/tree_vjp_multi_cases.py restates
them, against central differences of oracle/dense_kkt.solve on the reference's four small trees, 3 columns with
independent right-hand sides.  No GPU.

Loss L = sum_c w_c . z_c with fixed random w_c in the output arena's layout and z_c the dense solve of the ONE set of
blocks with (q, c, r) <- the right-hand side of column c; dL/dz_c = w_c and the adjoint of column c is the dense solve
with (q, c, r) <- w_c.  Every entry of every block of the input arena is perturbed in turn, as in
tests/test_tree_vjp_model.py: A, B, M, delta, q, c and r entry by entry, Q and R in symmetric directions.  The arena's
own q, c, r do not enter any column (the columns bring their right-hand sides), so there the quotient and the formula
must both be EXACTLY 0.

Tolerance: the one tests/test_tree_vjp_model.py derives from the scheme (truncation h^2 |K^-1|^3 |w| |z| plus rounding
N eps cond(K) |w| |z| / h per quotient), for every column with its own |w_c| |z_c|, summed over the columns -- at most
the number of columns times the worst column's."""
import numpy as np
import pytest

import full_batch_problems as fb
import tree_refine_cases as tc
import tree_vjp_cases as tv
import tree_vjp_multi_cases as tm
from oracle import dense_kkt

H = 1e-6
EPS = 2.0 ** -53
BATCH = 2
COLS = 3


def _row(topo, x, u, y):
    out = np.zeros(topo.layout.sol_len)
    vx, vy, vu = tv.views(topo, out[None])
    for dst, src in zip(vx + vy + vu, list(x) + list(y) + list(u)):
        dst[0, :] = src
    return out


def _solve(topo, blocks, rhs_row):
    """z of the blocks' matrices with the right-hand side rhs_row [sol_len] in place of the blocks' q, c, r."""
    gx, gy, gu = tv.views(topo, rhs_row[None])
    prob = dict(blocks, q=[v[0] for v in gx], c=[v[0] for v in gy], r=[v[0] for v in gu])
    return _row(topo, *dense_kkt.solve(topo.parents, topo.children, topo.sd, topo.cd, prob))


@pytest.mark.parametrize("name", list(tc.reference_trees()))
def test_formulas_against_central_differences(name):
    topo, blocks = tc.batched(tc.reference_trees()[name], BATCH, seed=17)
    for key in ("Q", "R"):                                   # exactly symmetric, as the library takes them
        blocks[key] = [tc._sym(a) for a in blocks[key]]
    L = topo.layout.sol_len
    rng = np.random.default_rng(41)
    w, rhs = rng.normal(size=(COLS, BATCH, L)), rng.normal(size=(COLS, BATCH, L))
    sol, adj, tol = np.zeros((COLS, BATCH, L)), np.zeros((COLS, BATCH, L)), np.zeros(BATCH)
    problems = [fb.problem(blocks, b) for b in range(BATCH)]
    for b, prob in enumerate(problems):
        K = dense_kkt.assemble(topo.parents, topo.children, topo.sd, topo.cd, prob)[0]
        sv = np.linalg.svd(K, compute_uv=False)
        inv, cond, N = 1.0 / sv[-1], sv[0] / sv[-1], K.shape[0]
        for c in range(COLS):
            sol[c, b] = _solve(topo, prob, rhs[c, b])
            adj[c, b] = _solve(topo, prob, w[c, b])
            scale = np.linalg.norm(w[c, b]) * np.linalg.norm(sol[c, b])
            tol[b] += H ** 2 * inv ** 3 * scale + N * EPS * cond * scale / H
    grad, mag, copy = tm.grad_input_multi(topo, sol, adj, dt=np.float64)
    assert grad.shape == (BATCH, tv.input_len(topo)) and (mag >= np.abs(grad)).all() and (grad[:, copy] == 0).all()
    # independent columns: the sum is not a multiple of one column's gradient
    one = tv.grad_input(topo, sol[0], adj[0], dt=np.float64)[0]
    assert np.abs(grad - COLS * one)[:, ~copy].max() > 1e-3

    def quotient(b, key, i, r, c, symmetric_direction):
        vals = []
        blk = problems[b][key][i]
        for sign in (+1, -1):
            where = [(r,)] if blk.ndim == 1 else [(r, c)] + ([(c, r)] if symmetric_direction and r != c else [])
            for at in where:
                blk[at] += sign * H
            vals.append(sum(float(w[col, b] @ _solve(topo, problems[b], rhs[col, b])) for col in range(COLS)))
            for at in where:
                blk[at] -= sign * H
        return (vals[0] - vals[1]) / (2 * H)

    lay = topo.layout
    worst, checked, zeros = 0.0, 0, 0
    for b in range(BATCH):
        top = np.abs(grad[b]).max()
        items = []                                           # (key, index, rows, cols, symmetric, offset in the arena)
        for i, n in enumerate(topo.sd):
            o = lay.node_off[i]
            items += [("Q", i, n, n, True, o), ("q", i, n, 1, False, o + n * n), ("c", i, n, 1, False, o + n * n + n),
                      ("delta", i, n, 1, False, o + n * n + 2 * n)]
        for e in range(topo.E):
            np_, nc, m = topo.edge_dims(e)
            o = lay.nodes_len + lay.edge_off[e]
            items += [("A", e, nc, np_, False, o), ("B", e, nc, m, False, o + nc * np_),
                      ("M", e, np_, m, False, o + nc * np_ + nc * m), ("R", e, m, m, True, o + nc * np_ + nc * m + np_ * m),
                      ("r", e, m, 1, False, o + nc * np_ + nc * m + np_ * m + m * m)]
        for key, i, rows, cols, sym, o in items:
            for c in range(cols):
                for r in range(c if sym else 0, rows):
                    fd = quotient(b, key, i, r, c, sym)
                    want = grad[b, o + r + rows * c]
                    if sym and r != c:
                        want = want + grad[b, o + c + rows * r]
                    if key in ("q", "c", "r"):
                        assert copy[o + r] and fd == 0.0 and want == 0.0, (key, i, r, fd, want)
                        zeros += 1
                    else:
                        assert not copy[o + r + rows * c]
                        assert abs(fd - want) <= tol[b], (key, i, r, c, fd, want, tol[b])
                        worst = max(worst, abs(fd - want) / top)
                    checked += 1
    print(f"TREE VJP MULTI MODEL | {name} | {COLS} columns, {checked} entries ({zeros} exact zeros), worst "
          f"|fd - formula| / max |grad| = {worst:.1e}, "
          f"tolerance / max |grad| = {float((tol / np.abs(grad).max(axis=1)).max()):.1e}")
    want_checked = sum(n * (n + 1) // 2 + 3 * n for n in topo.sd)
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        want_checked += nc * np_ + nc * m + np_ * m + m * (m + 1) // 2 + m
    assert checked == BATCH * want_checked
    assert zeros == BATCH * (2 * sum(topo.sd) + sum(topo.cd)) == BATCH * int(copy.sum())


def test_one_column_is_the_single_table_off_the_copies_and_the_bound_at_one_column():
    topo, _ = tc.batched(tc.reference_trees()["five_node"], 1, seed=1)
    rng = np.random.default_rng(5)
    L = topo.layout.sol_len
    z, lam = rng.normal(size=(4, 3, L)), rng.normal(size=(4, 3, L))
    g1, a1, copy1 = tv.grad_input(topo, z[0], lam[0])
    gm, am, copy = tm.grad_input_multi(topo, z[:1], lam[:1])
    assert np.array_equal(copy, copy1) and np.array_equal(gm[:, ~copy], g1[:, ~copy]) and np.array_equal(am, a1)
    assert (gm[:, copy] == 0).all() and (am[:, copy] == 0).all()
    assert np.array_equal(tm.kernel_bound(am, 1), tv.kernel_bound(a1)) and tm.roundings(4) == 9
    g4, a4, _ = tm.grad_input_multi(topo, z, lam)
    want = sum(tv.grad_input(topo, z[c], lam[c])[0] for c in range(4))
    assert np.abs(g4 - want)[:, ~copy].max() <= 4 * 2.0 ** -63 * a4.max() and (a4 >= np.abs(g4)).all()

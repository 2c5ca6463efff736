"""The gradient formulas of include/sip_lqr_amd.h (sip_lqr_tree_vjp), as tests/tree_vjp_cases.py restates them, against
central differences of oracle/dense_kkt.solve on the reference's four small trees.  No GPU.

Loss L = w . z with a fixed random w in the output arena's layout, so dL/dz = w and the adjoint is the dense solve with
(q, c, r) <- w.  Every entry of every block is perturbed in turn: A, B, M, delta, q, c and r entry by entry, Q and R in
symmetric directions E_rc + E_cr (E_rr on the diagonal), and the difference quotient is held against G[r, c] + G[c, r]
(G[r, r] on the diagonal): <G, dQ> for that direction.

Tolerance, from the scheme and not from the outcome (as in tests/test_vjp_model.py).  h = 1e-6.  z(theta) = -K(theta)^-1 b
along a direction E with |E|_2 = 1 has d^3 z / dtheta^3 = -6 (K^-1 E)^3 z, so the truncation of the central difference
is at most h^2 |K^-1|^3 |w| |z| (a perturbation of b alone has none).  Each of the two solves is an LU solve of N
unknowns whose error is at most about N eps cond(K) |z| (Higham, Accuracy and Stability, Theorem 9.4 with a modest
growth factor), so the rounding of the quotient is at most N eps cond(K) |w| |z| / h.  The sum of the two is the
absolute tolerance, per problem."""
import numpy as np
import pytest

import full_batch_problems as fb
import tree_refine_cases as tc
import tree_vjp_cases as tv
from oracle import dense_kkt

H = 1e-6
EPS = 2.0 ** -53
BATCH = 2


def _row(topo, x, u, y):
    out = np.zeros(topo.layout.sol_len)
    vx, vy, vu = tv.views(topo, out[None])
    for dst, src in zip(vx + vy + vu, list(x) + list(y) + list(u)):
        dst[0, :] = src
    return out


def _solve(topo, blocks):
    return _row(topo, *dense_kkt.solve(topo.parents, topo.children, topo.sd, topo.cd, blocks))


@pytest.mark.parametrize("name", list(tc.reference_trees()))
def test_formulas_against_central_differences(name):
    topo, blocks = tc.batched(tc.reference_trees()[name], BATCH, seed=17)
    for key in ("Q", "R"):                                   # exactly symmetric, as the library takes them
        blocks[key] = [tc._sym(a) for a in blocks[key]]
    L = topo.layout.sol_len
    w = np.random.default_rng(31).normal(size=(BATCH, L))
    sol, adj, tol = np.zeros((BATCH, L)), np.zeros((BATCH, L)), np.zeros(BATCH)
    problems = [fb.problem(blocks, b) for b in range(BATCH)]
    for b, prob in enumerate(problems):
        sol[b] = _solve(topo, prob)
        gx, gy, gu = tv.views(topo, w[b:b + 1])
        adj[b] = _solve(topo, dict(prob, q=[v[0] for v in gx], c=[v[0] for v in gy], r=[v[0] for v in gu]))
        K = dense_kkt.assemble(topo.parents, topo.children, topo.sd, topo.cd, prob)[0]
        sv = np.linalg.svd(K, compute_uv=False)
        inv, cond, N = 1.0 / sv[-1], sv[0] / sv[-1], K.shape[0]
        scale = np.linalg.norm(w[b]) * np.linalg.norm(sol[b])
        tol[b] = H ** 2 * inv ** 3 * scale + N * EPS * cond * scale / H
    grad, mag, copy = tv.grad_input(topo, sol, adj, dt=np.float64)
    assert grad.shape == (BATCH, tv.input_len(topo)) and (mag >= np.abs(grad) * (~copy)).all()

    def quotient(b, key, i, r, c, symmetric_direction):
        vals = []
        blk = problems[b][key][i]
        for sign in (+1, -1):
            where = [(r,)] if blk.ndim == 1 else [(r, c)] + ([(c, r)] if symmetric_direction and r != c else [])
            for at in where:
                blk[at] += sign * H
            vals.append(float(w[b] @ _solve(topo, problems[b])))
            for at in where:
                blk[at] -= sign * H
        return (vals[0] - vals[1]) / (2 * H)

    lay = topo.layout
    worst, checked = 0.0, 0
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
                    assert abs(fd - want) <= tol[b], (key, i, r, c, fd, want, tol[b])
                    worst = max(worst, abs(fd - want) / top)
                    checked += 1
    print(f"TREE VJP MODEL | {name} | {checked} entries, worst |fd - formula| / max |grad| = {worst:.1e}, "
          f"tolerance / max |grad| = {float((tol / np.abs(grad).max(axis=1)).max()):.1e}")
    want_checked = sum(n * (n + 1) // 2 + 3 * n for n in topo.sd)
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        want_checked += nc * np_ + nc * m + np_ * m + m * (m + 1) // 2 + m
    assert checked == BATCH * want_checked


def test_magnitudes_and_the_propagated_bound():
    """a >= |grad| off the copies, and moving z and l by e_z, e_l moves no entry by more than the propagated bound plus
    the second-order term e_l e_z per product."""
    topo, _ = tc.batched(tc.reference_trees()["five_node"], 1, seed=1)
    rng = np.random.default_rng(8)
    L = topo.layout.sol_len
    z, lam = rng.normal(size=(3, L)), rng.normal(size=(3, L))
    ez, el = np.array([1e-7, 1e-9, 0.0]), np.array([1e-8, 0.0, 1e-6])
    dz, dl = ez[:, None] * rng.uniform(-1, 1, size=z.shape), el[:, None] * rng.uniform(-1, 1, size=z.shape)
    g0, a0, copy = tv.grad_input(topo, z, lam)
    g1, _, _ = tv.grad_input(topo, z + dz, lam + dl)
    assert (a0[:, ~copy] >= np.abs(g0[:, ~copy])).all() and (a0[:, copy] == 0).all()
    bound = tv.propagated_bound(topo, z, lam, ez, el) + 2 * (ez * el)[:, None] + 8 * tv.U * (a0 + np.abs(g0))
    assert (np.abs(g1 - g0) <= bound).all()

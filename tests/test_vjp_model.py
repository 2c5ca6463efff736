"""The gradient formulas of include/sip_lqr_amd.h (sip_lqr_vjp_mats), as tests/vjp_cases.py restates them, against
central differences of oracle/dense_kkt.solve.  No GPU.

Loss L = w . z with a fixed random w in the sol layout, so dL/dz = w and the adjoint is the dense solve with
(q, c, r) <- w.  Every entry of every block is perturbed in turn: A, B, M and delta entry by entry, Q and R in symmetric
directions E_rc + E_cr (E_rr on the diagonal), which is also the direction of the packed parameter (r, c) of the
SYMMETRIC layout.  The difference quotient is held against
  FULL       G[r, c] + G[c, r]  (G[r, r] on the diagonal): <G, dQ> for that direction
  SYMMETRIC  the packed entry itself.

Tolerance, from the scheme and not from the outcome.  h = 1e-6.  z(theta) = -K(theta)^-1 b along a direction E with
|E|_2 = 1 has d^3 z / dtheta^3 = -6 (K^-1 E)^3 z, so the truncation of the central difference is at most
h^2 |K^-1|^3 |w| |z|.  Each of the two solves is an LU solve of N unknowns whose error is at most about
N eps cond(K) |z| (Higham, Accuracy and Stability, Theorem 9.4 with a modest growth factor), so the rounding of
the quotient is at most N eps cond(K) |w| |z| / h.  The sum of the two is the absolute tolerance, per problem.  (These
formulas came out at 4e-9 relative to the largest gradient entry at this h.)"""
import numpy as np
import pytest

import vjp_cases as vc
from oracle import dense_kkt

H = 1e-6
EPS = 2.0 ** -53


def _problem(n, m, T, batch, seed):
    from sip_optimal_control_amd import ChainShape, synthetic
    import hard_inputs as hi
    mats, vecs = synthetic.make_chain_batch(ChainShape(n, m, T), batch, seed=seed, cross_term=0.05)
    mats, vecs = mats.numpy().copy(), vecs.numpy().copy()
    views = hi.chain_views(n, m, T, mats)
    for blk in views["Q"] + views["R"]:                     # exactly symmetric, as the library takes them
        low = np.tril(blk)
        blk[...] = low + np.tril(blk, -1).transpose(0, 2, 1)
    return mats, vecs


def _pack_sol(n, m, T, x, u, y):
    out = []
    for i in range(T + 1):
        out += [x[i], y[i]] + ([u[i]] if i < T else [])
    return np.concatenate(out)


def _solve(n, m, T, blocks):
    par, ch = list(range(T)), list(range(1, T + 1))
    return _pack_sol(n, m, T, *dense_kkt.solve(par, ch, [n] * (T + 1), [m] * T, blocks))


@pytest.mark.parametrize("n,m,T", [(3, 2, 4), (1, 1, 1)])
def test_formulas_against_central_differences(n, m, T):
    from sip_optimal_control_amd import ChainShape
    batch = 2
    mats, vecs = _problem(n, m, T, batch, seed=11 + n)
    full, packed = ChainShape(n, m, T), ChainShape(n, m, T, symmetric=True)
    w = np.random.default_rng(5 + n).normal(size=vecs.shape)
    sol, adj, tol = np.zeros_like(vecs), np.zeros_like(vecs), np.zeros(batch)
    problems = []
    par, ch = list(range(T)), list(range(1, T + 1))
    for b in range(batch):
        blocks = dense_kkt.chain_blocks_from_packed(n, m, T, mats[b].copy(), vecs[b].copy())
        problems.append(blocks)
        sol[b] = _solve(n, m, T, blocks)
        gx, gy, gu = (list(t) for t in vc.slots(n, m, T, w[b:b + 1]))
        adjoint = dict(blocks, q=[v[0] for v in gx], c=[v[0] for v in gy], r=[v[0] for v in gu])
        adj[b] = _solve(n, m, T, adjoint)
        K = dense_kkt.assemble(par, ch, [n] * (T + 1), [m] * T, blocks)[0]
        sv = np.linalg.svd(K, compute_uv=False)
        inv, cond, N = 1.0 / sv[-1], sv[0] / sv[-1], K.shape[0]
        scale = np.linalg.norm(w[b]) * np.linalg.norm(sol[b])
        tol[b] = H ** 2 * inv ** 3 * scale + N * EPS * cond * scale / H
    g_full = vc.grad_mats(n, m, T, sol, adj, symmetric=False, dt=np.float64)[0]
    g_sym = vc.grad_mats(n, m, T, sol, adj, symmetric=True, dt=np.float64)[0]
    assert g_full.shape == (batch, full.mats_len) and g_sym.shape == (batch, packed.mats_len)

    def quotient(b, key, i, r, c, symmetric_direction):
        vals = []
        blk = problems[b][key][i]
        for sign in (+1, -1):
            where = [(r,)] if blk.ndim == 1 else [(r, c)] + ([(c, r)] if symmetric_direction and r != c else [])
            for at in where:
                blk[at] += sign * H
            vals.append(float(w[b] @ _solve(n, m, T, problems[b])))
            for at in where:
                blk[at] -= sign * H
        return (vals[0] - vals[1]) / (2 * H)

    worst, checked = 0.0, 0
    for b in range(batch):
        top = np.abs(g_full[b]).max()
        for i in range(T + 1):
            fo, so = full.mats_off(i), packed.mats_off(i)
            cases = [("Q", n, n, True), ("delta", n, 1, False)]
            if i < T:
                cases += [("A", n, n, False), ("B", n, m, False), ("M", n, m, False), ("R", m, m, True)]
            for key, rows, cols, sym in cases:
                k_packed = 0
                for c in range(cols):
                    for r in range(c if sym else 0, rows):
                        fd = quotient(b, key, i, r, c, sym)
                        at = fo[key] + r + rows * c
                        if sym:
                            want = g_full[b, at] + (g_full[b, fo[key] + c + rows * r] if r != c else 0.0)
                            got_sym = g_sym[b, so[key] + k_packed]
                            k_packed += 1
                        else:
                            want = g_full[b, at]
                            got_sym = g_sym[b, so[key] + r + rows * c]
                        assert abs(fd - want) <= tol[b], (key, i, r, c, fd, want, tol[b])
                        assert abs(fd - got_sym) <= tol[b], ("packed", key, i, r, c, fd, got_sym, tol[b])
                        worst = max(worst, abs(fd - want) / top, abs(fd - got_sym) / top)
                        checked += 1
    print(f"VJP MODEL | ({n},{m},{T}) | {checked} entries per layout, worst |fd - formula| / max |grad| = {worst:.1e}, "
          f"tolerance / max |grad| = {float((tol / np.abs(g_full).max(axis=1)).max()):.1e}")
    assert checked == batch * ((T + 1) * (n * (n + 1) // 2 + n) + T * (n * n + 2 * n * m + m * (m + 1) // 2))


def test_the_two_layouts_agree():
    """<G_full, dQ> = sum over the packed entries of g_rc dQ_rc for a symmetric dQ, on random vectors."""
    n, m, T, batch = 4, 3, 2, 2
    from sip_optimal_control_amd import ChainShape
    full, packed = ChainShape(n, m, T), ChainShape(n, m, T, symmetric=True)
    rng = np.random.default_rng(3)
    sol, adj = rng.normal(size=(batch, full.vecs_len)), rng.normal(size=(batch, full.vecs_len))
    g_full, a_full = vc.grad_mats(n, m, T, sol, adj, symmetric=False)
    g_sym, a_sym = vc.grad_mats(n, m, T, sol, adj, symmetric=True)
    d_full = rng.normal(size=(batch, full.mats_len))
    for i in range(T + 1):                                   # a symmetric direction in Q and R
        for key, dim in (("Q", n),) + ((("R", m),) if i < T else ()):
            o = full.mats_off(i)[key]
            blk = d_full[:, o:o + dim * dim].reshape(batch, dim, dim)
            blk[...] = blk + blk.transpose(0, 2, 1)
    d_sym = d_full[:, packed.pack_index()]
    lhs = (g_full * d_full).sum(axis=1)
    rhs = (g_sym * d_sym).sum(axis=1)
    slack = 2.0 ** -50 * (a_full * np.abs(d_full)).sum(axis=1)
    assert (np.abs(lhs - rhs) <= slack).all(), (lhs, rhs)
    assert (a_sym >= np.abs(g_sym)).all() and (a_full >= np.abs(g_full)).all()

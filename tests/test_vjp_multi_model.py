"""The gradient of a loss that reads several solutions against one `mats` (sip_lqr_vjp_mats_multi): the sum over the
columns of the formulas of tests/vjp_cases.py, against central differences of oracle/dense_kkt.solve.  No GPU.

Three right-hand sides b_c against one K(mats) at (n, m, T) = (3, 2, 2); loss L(mats) = sum_c w_c . z_c(mats) with
fixed random w_c in the sol layout, so dL/dz_c = w_c and adjoint c is the dense solve with (q, c, r) <- w_c.  The
scheme is that of tests/test_vjp_model.py: every entry of every block perturbed in turn, Q and R in symmetric
directions, the quotient held against G[r, c] + G[c, r] of the FULL layout and against the packed entry of the
SYMMETRIC one.

Tolerance, from the scheme and not from the outcome: that of tests/test_vjp_model.py per column, summed over the
columns (the loss is a sum, and so are its truncation and rounding errors): with h = 1e-6, per problem
  sum_c  h^2 |K^-1|^3 |w_c| |z_c|  +  N eps cond(K) |w_c| |z_c| / h."""
import numpy as np

import vjp_cases as vc
from oracle import dense_kkt

from test_vjp_model import EPS, H, _problem, _solve

N_, M_, T_, COLS, BATCH = 3, 2, 2, 3, 2


def test_summed_formulas_against_central_differences():
    from sip_optimal_control_amd import ChainShape
    n, m, T = N_, M_, T_
    mats, vecs0 = _problem(n, m, T, BATCH, seed=23)
    rng = np.random.default_rng(41)
    vecs = [vecs0] + [rng.normal(size=vecs0.shape) for _ in range(COLS - 1)]      # the right-hand sides b_c
    w = [rng.normal(size=vecs0.shape) for _ in range(COLS)]
    full, packed = ChainShape(n, m, T), ChainShape(n, m, T, symmetric=True)
    par, ch = list(range(T)), list(range(1, T + 1))
    sol = [np.zeros_like(vecs0) for _ in range(COLS)]
    adj = [np.zeros_like(vecs0) for _ in range(COLS)]
    tol = np.zeros(BATCH)
    problems = []                                                # [b][c]: blocks sharing the matrices of problem b
    for b in range(BATCH):
        base = dense_kkt.chain_blocks_from_packed(n, m, T, mats[b].copy(), vecs[0][b].copy())
        K = dense_kkt.assemble(par, ch, [n] * (T + 1), [m] * T, base)[0]
        sv = np.linalg.svd(K, compute_uv=False)
        inv, cond, N = 1.0 / sv[-1], sv[0] / sv[-1], K.shape[0]
        cols = []
        for c in range(COLS):
            rhs = dense_kkt.chain_blocks_from_packed(n, m, T, mats[b].copy(), vecs[c][b].copy())
            blocks = dict(base, q=rhs["q"], c=rhs["c"], r=rhs["r"])      # the matrices are base's own arrays
            cols.append(blocks)
            sol[c][b] = _solve(n, m, T, blocks)
            gx, gy, gu = (list(t) for t in vc.slots(n, m, T, w[c][b:b + 1]))
            adj[c][b] = _solve(n, m, T, dict(base, q=[v[0] for v in gx], c=[v[0] for v in gy], r=[v[0] for v in gu]))
            scale = np.linalg.norm(w[c][b]) * np.linalg.norm(sol[c][b])
            tol[b] += H ** 2 * inv ** 3 * scale + N * EPS * cond * scale / H
        problems.append((base, cols))
    g_full = sum(vc.grad_mats(n, m, T, sol[c], adj[c], symmetric=False, dt=np.float64)[0] for c in range(COLS))
    g_sym = sum(vc.grad_mats(n, m, T, sol[c], adj[c], symmetric=True, dt=np.float64)[0] for c in range(COLS))
    assert g_full.shape == (BATCH, full.mats_len) and g_sym.shape == (BATCH, packed.mats_len)

    def loss(b):
        return sum(float(w[c][b] @ _solve(n, m, T, problems[b][1][c])) for c in range(COLS))

    def quotient(b, key, i, r, c, symmetric_direction):
        vals = []
        blk = problems[b][0][key][i]
        for sign in (+1, -1):
            where = [(r,)] if blk.ndim == 1 else [(r, c)] + ([(c, r)] if symmetric_direction and r != c else [])
            for at in where:
                blk[at] += sign * H
            vals.append(loss(b))
            for at in where:
                blk[at] -= sign * H
        return (vals[0] - vals[1]) / (2 * H)

    # a perturbation of base's block is seen by every column: they share the arrays
    assert all(problems[0][1][c]["A"][0] is problems[0][0]["A"][0] for c in range(COLS))
    worst, checked = 0.0, 0
    for b in range(BATCH):
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
    print(f"VJP MULTI MODEL | ({n},{m},{T}) x {COLS} columns | {checked} entries per layout, worst |fd - formula| / "
          f"max |grad| = {worst:.1e}, tolerance / max |grad| = {float((tol / np.abs(g_full).max(axis=1)).max()):.1e}")
    assert checked == BATCH * ((T + 1) * (n * (n + 1) // 2 + n) + T * (n * n + 2 * n * m + m * (m + 1) // 2))
    # and the sum is not one column's gradient in disguise
    one = vc.grad_mats(n, m, T, sol[0], adj[0], symmetric=False, dt=np.float64)[0]
    assert np.abs(g_full - one).max() > 1e3 * tol.max()

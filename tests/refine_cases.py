"""TEST INFRASTRUCTURE ONLY: what tests/test_refine_model.py (no GPU) and tests/test_gpu_refine.py share -- the cells the
refinement is run on, the residual of the chain KKT system in numpy, its derived error bound, and a numpy restatement of
the refinement scheme.

Residual (the system oracle/dense_kkt.py states, in the vecs layout: slot q_i, slot c_i, slot r_i):
  rho_q[i] = Q_i x_i - y_i + q_i  (+ M_i u_i + A_i^T y_{i+1}           if i < T)
  rho_c[0] = -x_0 - delta_0 o y_0 + c_0
  rho_c[i] = A_{i-1} x_{i-1} + B_{i-1} u_{i-1} - x_i - delta_i o y_i + c_i     (i >= 1)
  rho_r[i] = M_i^T x_i + R_i u_i + B_i^T y_{i+1} + r_i                  (i < T)
Bound: an entry is a sum of at most 2 n + m + 3 terms (2 n + m products and three vector entries), every product and
partial sum rounded once in fp64 at the worst, so |got - ref| <= (2 n + m + 3) 2^-53 a, `a` the same expression on the
absolute values of the blocks and of z (Higham, Accuracy and Stability, (3.5), any summation order).  Derived, not
measured."""
import numpy as np

import hard_inputs as hi

LD = np.longdouble
CAP = 1e-9                      # the project's fp64 criterion e <= CAP + 3 e_ref (tests/test_gpu_hard_inputs.py)
ITERATIONS_F32, ITERATIONS_F64, ITERATIONS_OPEN = 4, 2, 8

# (n, m) of the cells the refinement runs on, all axes of hard_inputs.AXES_F32 / AXES_F64
CELLS_F32 = [(12, 4), (5, 3), (32, 8)]
CELLS_F64 = [(12, 4), (8, 4), (32, 8), (17, 9)]


def bound_factor(n, m):
    return (2 * n + m + 3) * 2.0 ** -53


def _slots(n, m, T, v):
    """q-, c- and r-slot views of a [B, vecs_len] array (sol: x, y, u), per stage."""
    vs = 2 * n + m
    a = [v[:, i * vs:i * vs + n] for i in range(T + 1)]
    b = [v[:, i * vs + n:i * vs + 2 * n] for i in range(T + 1)]
    c = [v[:, i * vs + 2 * n:i * vs + 2 * n + m] for i in range(T)]
    return a, b, c


def residual(n, m, T, mats, vecs, sol, dt=LD):
    """(rho, a) [B, vecs_len] in `dt`: the residual above from FULL-layout float64 mats, vecs, sol, and the same
    expression on absolute values."""
    blocks = {k: [np.asarray(b, dtype=dt) for b in v] for k, v in hi.chain_views(n, m, T, np.asarray(mats)).items()}
    q, c, r = _slots(n, m, T, np.asarray(vecs, dtype=dt))
    x, y, u = _slots(n, m, T, np.asarray(sol, dtype=dt))
    rho = np.zeros(vecs.shape, dtype=dt)
    mag = np.zeros(vecs.shape, dtype=dt)
    oq, oc, orr = _slots(n, m, T, rho)
    aq, ac, ar = _slots(n, m, T, mag)
    mv = lambda M, v: np.einsum("brc,bc->br", M, v)
    tv = lambda M, v: np.einsum("brc,br->bc", M, v)
    for signed, (dq, dc, dr) in ((True, (oq, oc, orr)), (False, (aq, ac, ar))):
        f = (lambda t: t) if signed else np.abs
        sgn = 1 if signed else -1       # the subtracted terms add in the magnitude
        Q, A, B, M, R, delta = (list(map(f, blocks[k])) for k in ("Q", "A", "B", "M", "R", "delta"))
        qq, cc, rr, xx, yy, uu = (list(map(f, t)) for t in (q, c, r, x, y, u))
        for i in range(T + 1):
            dq[i][...] = mv(Q[i], xx[i]) - sgn * yy[i] + qq[i]
            dc[i][...] = -sgn * xx[i] - sgn * delta[i] * yy[i] + cc[i]
            if i < T:
                dq[i][...] += mv(M[i], uu[i]) + tv(A[i], yy[i + 1])
                dr[i][...] = tv(M[i], xx[i]) + mv(R[i], uu[i]) + tv(B[i], yy[i + 1]) + rr[i]
            if i >= 1:
                dc[i][...] += mv(A[i - 1], xx[i - 1]) + mv(B[i - 1], uu[i - 1])
    return rho, mag


def scale_of(norm):
    """s: the power of two with s <= norm < 2 s; 1 for a norm that is 0 or not finite."""
    norm = np.asarray(norm, dtype=np.float64)
    ok = np.isfinite(norm) & (norm > 0)
    return np.where(ok, 2.0 ** np.floor(np.log2(np.where(ok, norm, 1.0))), 1.0)


# ---- the scheme in numpy ---------------------------------------------------------------------------------------------
def riccati_solve(n, m, T, blocks, q, c, r, dt):
    """One problem: the Riccati recursion and rollout in `dt` with W = (I + V Delta)^-1 V (oracle/numpy_riccati.py's
    form: nothing cancels at a tiny delta).  blocks: per-stage [rows, cols] arrays; q, c, r: per-stage vectors.
    -> packed sol row (x_i | y_i | u_i) in `dt`."""
    cast = lambda t: [np.asarray(a, dtype=dt) for a in t]
    Q, A, B, M, R, delta = (cast(blocks[k]) for k in ("Q", "A", "B", "M", "R", "delta"))
    q, c, r = cast(q), cast(c), cast(r)
    eye = np.eye(n, dtype=dt)
    V, v = [None] * (T + 1), [None] * (T + 1)
    K, k = [None] * T, [None] * T
    V[T], v[T] = Q[T], q[T]
    for i in range(T - 1, -1, -1):
        d = delta[i + 1]
        W = np.linalg.solve(eye + V[i + 1] * d[None, :], V[i + 1]).astype(dt)
        g = v[i + 1] + W @ (c[i + 1] - d * v[i + 1])
        G, H, h = R[i] + B[i].T @ W @ B[i], M[i].T + B[i].T @ W @ A[i], r[i] + B[i].T @ g
        X = -np.linalg.solve(G, np.concatenate([H, h[:, None]], axis=1)).astype(dt)
        K[i], k[i] = X[:, :-1], X[:, -1]
        V[i] = Q[i] + A[i].T @ W @ A[i] + K[i].T @ H
        v[i] = q[i] + A[i].T @ g + K[i].T @ h
    out = []
    x = np.linalg.solve(eye + delta[0][:, None] * V[0], c[0] - delta[0] * v[0]).astype(dt)
    for i in range(T + 1):
        out += [x, V[i] @ x + v[i]]
        if i < T:
            u = K[i] @ x + k[i]
            out.append(u)
            d = delta[i + 1]
            x = np.linalg.solve(eye + d[:, None] * V[i + 1], A[i] @ x + B[i] @ u + c[i + 1] - d * v[i + 1]).astype(dt)
    return np.concatenate(out).astype(dt)


def model_refine(cell, iterations, dt):
    """The scheme on a cell: recursion in `dt`, residual and iterate in float64, starting from zero.  -> per round the
    iterate [B, vecs_len] (float64) and the residual norms [iterations + 1, B]."""
    n, m, T = cell.shape
    views = hi.chain_views(n, m, T, cell.mats)
    B = cell.mats.shape[0]
    z = np.zeros(cell.vecs.shape)
    iterates, norms = [], []
    for _ in range(iterations):
        rho = residual(n, m, T, cell.mats, cell.vecs, z, dt=np.float64)[0]
        nrm = np.abs(rho).max(axis=1)
        norms.append(nrm)
        s = scale_of(nrm)
        rhs = (rho / s[:, None]).astype(dt)
        q, c, r = _slots(n, m, T, rhs)
        for b in range(B):
            blocks = {k: [a[b] for a in v] for k, v in views.items()}
            d = riccati_solve(n, m, T, blocks, [t[b] for t in q], [t[b] for t in c], [t[b] for t in r], dt)
            z[b] += s[b] * d.astype(np.float64)
        iterates.append(z.copy())
    norms.append(np.abs(residual(n, m, T, cell.mats, cell.vecs, z, dt=np.float64)[0]).max(axis=1))
    return iterates, np.stack(norms)

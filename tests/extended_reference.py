"""TEST INFRASTRUCTURE ONLY: an extended-precision solve of the dense KKT system of a tree-LQR problem, the yardstick
of the hard-input tests (tests/hard_inputs.py, tests/test_gpu_hard_inputs.py).

The matrix is the one oracle.dense_kkt.assemble builds (fp64 inputs, exactly representable), cast to np.longdouble
(x87 extended, eps 1.08e-19 on the x86 hosts -- asserted, not skipped), factorised by LU with partial pivoting and
solved; two steps of iterative refinement follow, residuals in long double.  solve() returns x, u, y and the size of
the last correction relative to the solution: what the reference itself still moved by.

cached(key, make) keeps what a (shape, axis, seed) cell needs for the whole session: several kernel families share
a shape and must share inputs and reference."""
import numpy as np

from oracle import dense_kkt

LD = np.longdouble
assert np.finfo(LD).eps <= 1.1e-19, "np.longdouble is not the 80-bit extended type: no extended reference here"
REFINEMENTS = 2
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def lu_factor(A):
    """LU with partial pivoting of a square long-double matrix, in place: (LU, row order).  The rank-1 update of a
    step touches only the rows and columns whose multiplier / pivot-row entry is not zero (the KKT matrix is sparse;
    leaving out exact zeros changes nothing)."""
    n = A.shape[0]
    order = np.arange(n)
    for k in range(n - 1):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        assert A[p, k] != 0, "singular KKT matrix"
        if p != k:
            A[[k, p]] = A[[p, k]]
            order[[k, p]] = order[[p, k]]
        A[k + 1:, k] /= A[k, k]
        rows = k + 1 + np.flatnonzero(A[k + 1:, k])
        cols = k + 1 + np.flatnonzero(A[k, k + 1:])
        if rows.size and cols.size:
            A[np.ix_(rows, cols)] -= np.outer(A[rows, k], A[k, cols])
    return A, order


def lu_solve(LU, order, B):
    """Solve with the factors of lu_factor for the columns of B [n, k]."""
    X = B[order].copy()
    n = LU.shape[0]
    for k in range(n - 1):                       # L y = P b, unit diagonal
        X[k + 1:] -= np.outer(LU[k + 1:, k], X[k])
    for k in range(n - 1, -1, -1):               # U x = y
        X[k] /= LU[k, k]
        X[:k] -= np.outer(LU[:k, k], X[k])
    return X


class Factored:
    """The KKT matrix of one problem, factorised once in long double; solve() takes any number of right-hand sides
    (each a dict with the problem's "q", "c" per node and "r" per edge; None: the problem's own)."""

    def __init__(self, parents, children, state_dims, control_dims, blocks, root=0):
        self.topology = (list(parents), list(children), list(state_dims), list(control_dims))
        self.blocks, self.root = blocks, root
        Kmat, self.rhs, self.offsets = dense_kkt.assemble(*self.topology, blocks, root)
        self.K = Kmat.astype(LD)
        self.LU, self.order = lu_factor(self.K.copy())

    def _rhs(self, column):
        if column is None:
            return self.rhs
        patched = dict(self.blocks)
        patched.update({k: column[k] for k in ("q", "c", "r")})
        return dense_kkt.assemble(*self.topology, patched, self.root)[1]

    def solve(self, columns=(None,)):
        """-> (list of (x, u, y) in fp64, one per column, worst relative size of the last correction)."""
        B = np.stack([self._rhs(c) for c in columns], axis=1).astype(LD)
        Z = lu_solve(self.LU, self.order, B)
        last = 0.0
        for _ in range(REFINEMENTS):
            D = lu_solve(self.LU, self.order, B - self.K @ Z)
            Z += D
            last = float((np.abs(D).max(axis=0) / np.abs(Z).max(axis=0)).max())
        xo, uo, yo = self.offsets
        _, _, sd, cd = self.topology
        out = []
        for j in range(len(columns)):
            z = Z[:, j].astype(np.float64)
            out.append(([z[xo[i]:xo[i] + d] for i, d in enumerate(sd)], [z[uo[e]:uo[e] + d] for e, d in enumerate(cd)],
                        [z[yo[i]:yo[i] + d] for i, d in enumerate(sd)]))
        return out, last


def solve(parents, children, state_dims, control_dims, blocks, root=0):
    """-> ((x, u, y), relative size of the last refinement correction)."""
    sols, last = Factored(parents, children, state_dims, control_dims, blocks, root).solve()
    return sols[0], last


def riccati_gains(parents, children, state_dims, control_dims, blocks):
    """K_e, k_e (fp64) of every edge by the textbook recursion in long double, with W = (I + V Delta)^-1 V formed by a
    solve: no D^1/2 scaling and no I - F^-1, so nothing cancels at a tiny delta (oracle/numpy_riccati.py, on trees).
    A second reference next to the dense solve, which has no gains: u_e = K_e x_parent(e) + k_e ties the two."""
    E = len(control_dims)
    assert all(children[e] == e + 1 and parents[e] <= e for e in range(E)), "edges in reverse are not a postorder"
    solve_ld = lambda A, B: lu_solve(*lu_factor(A.copy()), B)
    V = [np.array(Q, dtype=LD) for Q in blocks["Q"]]
    v = [np.array(q, dtype=LD) for q in blocks["q"]]
    Ks, ks = [None] * E, [None] * E
    for e in reversed(range(E)):
        p, c = parents[e], children[e]
        A, B, M, R, r = (np.asarray(blocks[k][e], dtype=LD) for k in ("A", "B", "M", "R", "r"))
        d, cc = np.asarray(blocks["delta"][c], dtype=LD), np.asarray(blocks["c"][c], dtype=LD)
        W = solve_ld(np.eye(state_dims[c], dtype=LD) + V[c] * d[None, :], V[c])
        g = v[c] + W @ (cc - d * v[c])
        H, h = M.T + B.T @ W @ A, r + B.T @ g
        X = -solve_ld(R + B.T @ W @ B, np.concatenate([H, h[:, None]], axis=1))
        K, k = X[:, :-1], X[:, -1]
        V[p] += A.T @ W @ A + K.T @ H
        v[p] += A.T @ g + K.T @ h
        Ks[e], ks[e] = K.astype(np.float64), k.astype(np.float64)
    return Ks, ks


def gains_row(Ks, ks):
    """K_e (column-major) | k_e per edge: the packed gains of a chain and the oracle's gains layout of a tree."""
    return np.concatenate([np.concatenate([K.reshape(-1, order="F"), k]) for K, k in zip(Ks, ks)] + [np.zeros(0)])


def chain_row(x, u, y):
    """x, u, y of a chain in the packed sol layout (x_i | y_i | u_i per stage)."""
    T = len(u)
    return np.concatenate([np.concatenate([x[i], y[i]] + ([u[i]] if i < T else [])) for i in range(T + 1)])


def tree_row(x, u, y):
    """x, u, y of a tree in the oracle's sol layout (x_i | y_i per node, then u_e per edge)."""
    return np.concatenate([np.concatenate([x[i], y[i]]) for i in range(len(x))] + list(u) + [np.zeros(0)])


def err(got, ext):
    """e(v) of the hard-input criterion: max over the problems (rows) of max |v - ext| / max |ext|."""
    got, ext = np.asarray(got, dtype=np.float64), np.asarray(ext, dtype=np.float64)
    return float((np.abs(got - ext).max(axis=-1) / np.abs(ext).max(axis=-1)).max())

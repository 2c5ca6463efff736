"""TEST INFRASTRUCTURE ONLY: what tests/test_vjp_model.py (no GPU) and the tests/test_gpu_vjp*.py share -- the gradient of
a loss with respect to `mats` through the chain KKT solve, restated in numpy block by block, and its derived bound.

With z = (x_i, y_i, u_i) the solution and l = (lx_i, ly_i, lu_i) the adjoint (K l + dL/dz = 0), both in the sol layout:
  Q_i, FULL       1/2 (lx_i x_i^T + x_i lx_i^T), the whole square
  Q_i, SYMMETRIC  packed entry (r, c): lx_r x_c + lx_c x_r for r > c, lx_r x_r for r = c
  R_i             the same two rules with lu_i, u_i
  delta_i         -ly_i o y_i
  A_i             ly_{i+1} x_i^T + y_{i+1} lx_i^T
  B_i             ly_{i+1} u_i^T + y_{i+1} lu_i^T
  M_i             lx_i u_i^T + x_i lu_i^T
Next to every entry its magnitude a = sum of |terms| (a FULL entry of Q: 1/2 |lx_r x_c| + 1/2 |x_r lx_c|).

Bound of the kernel (csrc/chain_vjp.hpp): an entry is fma(l[ia], z[ib], z[ia] * l[ib]) -- the product rounded, then the
fused sum rounded: |err| <= u |t1| + u |t1 + t2| (1 + u) <= (2 u + u^2) a with u = 2^-53 -- times 1, 1/2 or -1/2, which
is exact.  c = 3 covers the two roundings with their second-order term and the 2^-64 of the long-double reference.  The
all-float form rounds the result once more: + 2^-24 |ref|.  Derived, not measured."""
import numpy as np

LD = np.longdouble
C_ROUNDINGS = 3


def slots(n, m, T, v):
    """x-, y- and u-slot views of a [B, vecs_len] array, per stage."""
    vs = 2 * n + m
    x = [v[:, i * vs:i * vs + n] for i in range(T + 1)]
    y = [v[:, i * vs + n:i * vs + 2 * n] for i in range(T + 1)]
    u = [v[:, i * vs + 2 * n:i * vs + 2 * n + m] for i in range(T)]
    return x, y, u


def _outer(a, b):
    return np.einsum("br,bc->brc", a, b)


def _flat(block):
    """[B, rows, cols] -> [B, rows * cols], column-major."""
    return block.transpose(0, 2, 1).reshape(block.shape[0], -1)


def _pair(la, za, lb, zb):
    """(l_a z_b^T + z_a l_b^T, the same on absolute values) [B, rows, cols]."""
    t1, t2 = _outer(la, zb), _outer(za, lb)
    return t1 + t2, np.abs(t1) + np.abs(t2)


def _symmetric_block(l, z, symmetric):
    """Gradient and magnitude of Q (or R) from its vectors, flattened in the FULL or the SYMMETRIC layout."""
    dim = z.shape[1]
    g, a = _pair(l, z, l, z)
    if not symmetric:
        return _flat(g / 2), _flat(a / 2)
    diag = np.einsum("br,br->br", l, z)
    rows = [(r, c) for c in range(dim) for r in range(c, dim)]       # lower triangle packed by columns
    pick = lambda full, d: np.stack([d[:, r] if r == c else full[:, r, c] for r, c in rows], axis=1) \
        if rows else np.zeros((z.shape[0], 0), dtype=z.dtype)
    return pick(g, diag), pick(a, np.abs(diag))


def grad_mats(n, m, T, sol, adj, symmetric=False, dt=LD):
    """(grad, a) [B, mats_len] in `dt`, in the FULL or SYMMETRIC layout of `mats`, from float64 sol and adj."""
    x, y, u = slots(n, m, T, np.asarray(sol, dtype=dt))
    lx, ly, lu = slots(n, m, T, np.asarray(adj, dtype=dt))
    grad, mag = [], []

    def put(g, a):
        grad.append(g), mag.append(a)

    for i in range(T + 1):
        put(*_symmetric_block(lx[i], x[i], symmetric))
        put(-ly[i] * y[i], np.abs(ly[i] * y[i]))
        if i < T:
            for g, a in (_pair(ly[i + 1], y[i + 1], lx[i], x[i]),     # A_i
                         _pair(ly[i + 1], y[i + 1], lu[i], u[i]),     # B_i
                         _pair(lx[i], x[i], lu[i], u[i])):            # M_i
                put(_flat(g), _flat(a))
            put(*_symmetric_block(lu[i], u[i], symmetric))
    return np.concatenate(grad, axis=1), np.concatenate(mag, axis=1)


def kernel_bound(mag, ref, f32_out):
    """The bound of the module docstring per entry."""
    return C_ROUNDINGS * 2.0 ** -53 * mag + (2.0 ** -24 * np.abs(ref) if f32_out else 0)


def propagated_bound(n, m, T, z, lam, e_z, e_lam, symmetric=False):
    """First-order propagation of errors |dz| <= e_z, |dl| <= e_lam (scalars per problem, [B]) through every entry:
    each term l_a z_b moves by at most e_lam |z_b| + |l_a| e_z, summed over the entry's terms with their weights --
    which is grad_mats' magnitude with (|l|, |z|) replaced by (e_lam, |z|) plus (|l|, e_z).  [B, mats_len]."""
    z, lam = np.abs(np.asarray(z, dtype=LD)), np.abs(np.asarray(lam, dtype=LD))
    ez = np.broadcast_to(np.asarray(e_z, dtype=LD)[:, None], z.shape)
    el = np.broadcast_to(np.asarray(e_lam, dtype=LD)[:, None], z.shape)
    return grad_mats(n, m, T, z, el, symmetric)[1] + grad_mats(n, m, T, ez, lam, symmetric)[1]

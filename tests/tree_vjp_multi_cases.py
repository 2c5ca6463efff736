"""TEST INFRASTRUCTURE ONLY: what tests/test_tree_vjp_multi_model.py (no GPU) and the tests/test_gpu_tree_vjp_multi*.py
share -- the gradient of a loss that reads several columns z_c of sip_lqr_tree_solve_multi with respect to the ONE input
arena, restated in numpy on top of tests/tree_vjp_cases.py, and its derived bound.

grad = sum over c, in ascending order, of the one-column table of tree_vjp_cases.grad_input on (z_c, l_c), EXCEPT the
copies: solve_multi does not read the arena's q, c, r (its right-hand sides are the columns), so those slots are 0 and
dL/db_c is l_c, the adjoint column.  Next to every entry its magnitude a = sum over c of the one-column magnitudes
|s| (|l_c[ia] z_c[ib]| + |z_c[ia] l_c[ib]|); a copy has a = 0.

Bound of the kernel (csrc/tree_vjp_cols.hpp), k columns: column 0 is fma(l[ia], z[ib], z[ia] * l[ib]) -- two roundings --
and every further column acc = fma(l[ia], z[ib], fma(z[ia], l[ib], acc)) -- two more, each of a partial sum whose
magnitude is at most the sum of the |terms| so far (1 + u)^j: after 2 k roundings |err| <= ((1 + u)^(2k) - 1) sum|terms|
= (2 k u + O(u^2)) sum|terms|, u = 2^-53; the factor s is exact, and so is undoing it between two launches, so the
grouping does not enter.  (2 k + 1) u covers the second-order terms (k <= 17 here) and the 2^-64 of the long-double
reference.  At k = 1 this is tree_vjp_cases.C_ROUNDINGS = 3.  A copy is exactly +0.0: bound 0.  Derived, not measured."""
import numpy as np

import tree_vjp_cases as tv

LD = tv.LD
U = tv.U


def grad_input_multi(topo, sol_cols, adj_cols, dt=LD):
    """(grad, a, copy) -- grad and a [B, input_len] in `dt`, copy [input_len] bool -- from sol_cols and adj_cols
    [num_rhs, B, sol_len]: the columns summed in ascending order, the copies 0."""
    sol_cols, adj_cols = np.asarray(sol_cols), np.asarray(adj_cols)
    assert sol_cols.shape == adj_cols.shape and sol_cols.ndim == 3
    B = sol_cols.shape[1]
    grad, mag = np.zeros((B, tv.input_len(topo)), dtype=dt), np.zeros((B, tv.input_len(topo)), dtype=dt)
    _, _, copy = tv.grad_input(topo, np.zeros((1, topo.layout.sol_len)), np.zeros((1, topo.layout.sol_len)), dt=dt)
    for c in range(sol_cols.shape[0]):
        g, a, _ = tv.grad_input(topo, sol_cols[c], adj_cols[c], dt=dt)
        grad, mag = grad + np.where(copy[None, :], 0, g), mag + a
    return grad, mag, copy


def roundings(num_rhs):
    """c of the bound c * 2^-53 * a for num_rhs columns."""
    return 2 * max(int(num_rhs), 1) + 1


def kernel_bound(mag, num_rhs):
    """The bound of the module docstring per entry (0 on a copy, whose a is 0)."""
    return roundings(num_rhs) * U * mag


assert roundings(1) == tv.C_ROUNDINGS

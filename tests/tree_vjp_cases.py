"""TEST INFRASTRUCTURE ONLY: what tests/test_tree_vjp_model.py, tests/test_tree_vjp_table.py (no GPU) and the
tests/test_gpu_tree_vjp*.py share -- the gradient of a loss with respect to the input arena through the tree KKT solve,
restated in numpy block by block, and its derived bounds.

With z = (x_i, y_i per node; u_e per edge) the solution and l = (lx_i, ly_i; lu_e) the adjoint (K l + dL/dz = 0), both
in the output arena's layout (the oracle's sol layout: x_i | y_i per node, then u_e per edge), for node i and for edge e
with parent p and child c:
  Q_i      1/2 (lx_i x_i^T + x_i lx_i^T), the whole square
  q_i, c_i lx_i, ly_i
  delta_i  -ly_i o y_i
  A_e      ly_c x_p^T + y_c lx_p^T
  B_e      ly_c u_e^T + y_c lu_e^T
  M_e      lx_p u_e^T + x_p lu_e^T
  R_e      1/2 (lu_e u_e^T + u_e lu_e^T)
  r_e      lu_e
in the order of the input arena: node blocks Q | q | c | delta, then edge blocks A | B | M | R | r, matrices
column-major (the oracle's [nodes | edges]).  Next to every entry its magnitude a = |s| (|l[ia] z[ib]| + |z[ia] l[ib]|),
s the entry's exact factor 1, 1/2 or -1/2; a copy has a = 0.

Bound of the kernel (csrc/tree_vjp.hpp): an entry is fma(l[ia], z[ib], z[ia] * l[ib]) -- the product rounded, then the
fused sum rounded: |err| <= u |t2| + u |t1 + t2| (1 + u) <= (2 u + u^2) (|t1| + |t2|) with u = 2^-53 -- times s, which
is exact.  c = 3 covers the two roundings with their second-order term and the 2^-64 of the long-double reference.  A
copy is exact: bound 0.  Derived, not measured."""
import numpy as np

LD = np.longdouble
C_ROUNDINGS = 3
U = 2.0 ** -53


def views(topo, v):
    """x-, y- and u-slot views of a [B, sol_len] array."""
    lay = topo.layout
    x = [v[:, lay.x_off[i]:lay.x_off[i] + n] for i, n in enumerate(topo.sd)]
    y = [v[:, lay.x_off[i] + n:lay.x_off[i] + 2 * n] for i, n in enumerate(topo.sd)]
    u = [v[:, lay.u_off[e]:lay.u_off[e] + m] for e, m in enumerate(topo.cd)]
    return x, y, u


def input_len(topo):
    return topo.layout.nodes_len + topo.layout.edges_len


def _outer(a, b):
    # (stated, not left to einsum: on long double it returns unset memory for a dimension of 0)
    return a[:, :, None] * b[:, None, :]


def _flat(block):
    """[B, rows, cols] -> [B, rows * cols], column-major."""
    return block.transpose(0, 2, 1).reshape(block.shape[0], -1)


def _pair(la, za, lb, zb, s):
    """s (l_a z_b^T + z_a l_b^T) and |s| times the same on absolute values, flattened."""
    t1, t2 = _outer(la, zb), _outer(za, lb)
    return _flat(s * (t1 + t2)), _flat(abs(s) * (np.abs(t1) + np.abs(t2)))


def grad_input(topo, sol, adj, dt=LD):
    """(grad, a, copy) -- grad and a [B, input_len] in `dt`, copy [input_len] bool (the q, c, r slots) -- from sol and
    adj [B, sol_len]."""
    x, y, u = views(topo, np.asarray(sol, dtype=dt))
    lx, ly, lu = views(topo, np.asarray(adj, dtype=dt))
    grad, mag, copy = [], [], []

    def put(g, a, is_copy=False):
        grad.append(g), mag.append(a), copy.append(np.full(g.shape[1], is_copy))

    half, one = dt(0.5), dt(1.0)
    for i in range(topo.N):
        put(*_pair(lx[i], x[i], lx[i], x[i], half))                     # Q_i
        put(lx[i], np.zeros_like(lx[i]), True)                          # q_i
        put(ly[i], np.zeros_like(ly[i]), True)                          # c_i
        put(-ly[i] * y[i], np.abs(ly[i] * y[i]))                        # delta_i
    for e in range(topo.E):
        p, c = topo.parents[e], topo.children[e]
        put(*_pair(ly[c], y[c], lx[p], x[p], one))                      # A_e
        put(*_pair(ly[c], y[c], lu[e], u[e], one))                      # B_e
        put(*_pair(lx[p], x[p], lu[e], u[e], one))                      # M_e
        put(*_pair(lu[e], u[e], lu[e], u[e], half))                     # R_e
        put(lu[e], np.zeros_like(lu[e]), True)                          # r_e
    B = np.asarray(sol).shape[0]
    g = np.concatenate(grad, axis=1) if grad else np.zeros((B, 0), dtype=dt)
    a = np.concatenate(mag, axis=1) if mag else np.zeros((B, 0), dtype=dt)
    c = np.concatenate(copy) if copy else np.zeros(0, dtype=bool)
    assert g.shape == (B, input_len(topo))
    return g, a, c


def kernel_bound(mag):
    """The bound of the module docstring per entry (0 on a copy)."""
    return C_ROUNDINGS * U * mag


def propagated_bound(topo, z, lam, e_z, e_lam):
    """First-order propagation of errors |dz| <= e_z, |dl| <= e_lam (scalars per problem, [B]) through every entry: each
    term l_a z_b moves by at most e_lam |z_b| + |l_a| e_z, summed over the entry's terms with their weights -- which is
    grad_input's magnitude with (|l|, |z|) replaced by (e_lam, |z|) plus (|l|, e_z); a copy moves by e_lam.
    [B, input_len]."""
    z, lam = np.abs(np.asarray(z, dtype=LD)), np.abs(np.asarray(lam, dtype=LD))
    ez = np.broadcast_to(np.asarray(e_z, dtype=LD)[:, None], z.shape)
    el = np.broadcast_to(np.asarray(e_lam, dtype=LD)[:, None], z.shape)
    _, a1, copy = grad_input(topo, z, el)
    _, a2, _ = grad_input(topo, ez, lam)
    return a1 + a2 + np.where(copy[None, :], np.asarray(e_lam, dtype=LD)[:, None], 0)


# ---- the trees the GPU tests run on ------------------------------------------------------------------------------------
STAGED, DIRECT = "tree_vjp<staged>/f64", "tree_vjp<direct>/f64"


def topologies():
    """name -> (Topology, the gradient kernel's name, the solve kernel's name starts with): the reference's four small
    trees, a single node, dimensions of 0, the random trees of hard_inputs, a tree of the general engine, a star, and a
    chain whose z and lambda pairs (16 * 4476 bytes) exceed the LDS budget."""
    import full_batch_problems as fb
    import hard_inputs as hi
    import reference_problems as rp
    T = fb.Topology
    out = {}
    for name, prob in (("nonuniform_delta_chain", rp.nonuniform_diagonal_delta()), ("branch", rp.branch_tree()),
                       ("variable_branch", rp.variable_dimension_branch()),
                       ("five_node", rp.five_node_variable_tree_eigen())):
        out[name] = (T(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"], name), STAGED,
                     "tree_factor_solve_qw16")
    out["single_node"] = (T([], [], [5], [], "single_node"), STAGED, "tree_factor_solve_qw16")
    out["node_n0"] = (T([0, 1, 1], [1, 2, 3], [3, 0, 4, 3], [2, 1, 1], "node_n0"), STAGED, "tree_")
    out["edge_m0"] = (T([0, 1, 1], [1, 2, 3], [3, 2, 4, 3], [2, 0, 1], "edge_m0"), STAGED, "tree_")
    for dims in hi.TREES:
        rng = np.random.default_rng(hi._seed("tree", *dims))
        topo = fb.random_topology(rng, hi.TREE_NODES, *dims)
        out[topo.name] = (topo, STAGED, "tree_factor_solve_qw16<%d,%d>" % dims)
    out["general<17,9>"] = (T([0, 0, 1], [1, 2, 3], [5, 17, 3, 4], [9, 2, 3], "general<17,9>"), STAGED, "tree_generic")
    out["star_of_12"] = (T([0] * 12, list(range(1, 13)), [6, 3, 4, 5] * 3 + [2], [2, 1, 3] * 4, "star_of_12"), STAGED,
                         "tree_factor_solve_qw16")
    out["chain_30x70"] = (T(list(range(69)), list(range(1, 70)), [30] * 70, [4] * 69, "chain_30x70"), DIRECT, "tree_generic")
    return out

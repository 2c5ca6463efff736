"""TEST INFRASTRUCTURE ONLY: what tests/test_tree_refine_model.py (no GPU) and tests/test_gpu_tree_refine.py share -- the
residual of the tree KKT system in numpy, its derived error bound, the trees the residual is run on and a numpy
restatement of the refinement scheme of sip_lqr_tree_refine.

Residual (the system oracle/dense_kkt.py states), in the layout of a right-hand side of sip_lqr_tree_solve_multi, which
is the oracle's sol layout (q | c where x | y are per node, then r where u is per edge):
  rho_q[i]        = Q_i x_i - y_i + q_i + sum over the child edges e of i of (M_e u_e + A_e^T y_child(e))
  rho_c[root]     = -x_root - delta_root o y_root + c_root
  rho_c[child(e)] = A_e x_parent(e) + B_e u_e - x_child - delta_child o y_child + c_child
  rho_r[e]        = M_e^T x_parent(e) + R_e u_e + B_e^T y_child + r_e
Q and R are taken symmetric from their lower triangles.

Bound: an entry is a sum of k terms -- its products plus its vector entries, the expression evaluated on all-ones --
every product and partial sum rounded once in fp64 at the worst, so |got - ref| <= k 2^-53 a, `a` the same expression
on the absolute values of the blocks and of z (Higham, Accuracy and Stability, (3.5), any summation order; the chain
tests' (2 n + m + 3) rule with the terms counted per entry).  Derived, not measured."""
import numpy as np

import full_batch_problems as fb
import hard_inputs as hi
import reference_problems as rp
from oracle import oracle
from refine_cases import CAP, ITERATIONS_F64, LD, scale_of  # noqa: F401  (one scale rule, one cap)

U = 2.0 ** -53


def _sym(S):
    """[B, n, n] -> symmetric from the lower triangle (selfadjointView<Lower>)."""
    return np.tril(S) + np.tril(S, -1).transpose(0, 2, 1)


def _views(topo, v):
    """q-, c- and r-slot views of a [B, sol_len] array (sol: x, y, u)."""
    lay = topo.layout
    a = [v[:, lay.x_off[i]:lay.x_off[i] + n] for i, n in enumerate(topo.sd)]
    b = [v[:, lay.x_off[i] + n:lay.x_off[i] + 2 * n] for i, n in enumerate(topo.sd)]
    c = [v[:, lay.u_off[e]:lay.u_off[e] + m] for e, m in enumerate(topo.cd)]
    return a, b, c


def rhs_row(topo, rhs):
    """A right-hand side {"q", "c", "r"} of arrays with a leading batch axis -> [B, sol_len] in the rhs layout."""
    B = (rhs["q"] + rhs["r"])[0].shape[0]
    out = np.zeros((B, topo.layout.sol_len))
    q, c, r = _views(topo, out)
    for dst, src in zip(q + c + r, list(rhs["q"]) + list(rhs["c"]) + list(rhs["r"])):
        dst[...] = src
    return out


def residual(topo, blocks, rhs, sol, dt=LD, root=0):
    """(rho, a) [B, sol_len] in `dt`.  blocks: arrays with a leading batch axis (full_batch_problems); rhs: None (q, c,
    r of blocks) or {"q", "c", "r"} likewise; sol: [B, sol_len] (x_i | y_i per node, then u_e per edge).  `a` is the
    same expression on absolute values."""
    cast = lambda t: [np.asarray(a, dtype=dt) for a in t]
    src = blocks if rhs is None else rhs
    Q, R = cast(_sym(np.asarray(a)) for a in blocks["Q"]), cast(_sym(np.asarray(a)) for a in blocks["R"])
    A, Bm, M, delta = (cast(blocks[k]) for k in ("A", "B", "M", "delta"))
    q, c, r = (cast(src[k]) for k in ("q", "c", "r"))
    x, y, u = _views(topo, np.asarray(sol, dtype=dt))
    rho, mag = np.zeros(sol.shape, dtype=dt), np.zeros(sol.shape, dtype=dt)
    # (an empty sum is stated, not left to einsum: on long double it returns unset memory for a dimension of 0)
    mv = lambda Mx, v: np.einsum("brc,bc->br", Mx, v) if Mx.size else np.zeros(Mx.shape[:2], dtype=dt)
    tv = lambda Mx, v: np.einsum("brc,br->bc", Mx, v) if Mx.size else np.zeros(Mx.shape[::2], dtype=dt)
    for signed, out in ((True, rho), (False, mag)):
        f = (lambda t: t) if signed else np.abs
        sgn = 1 if signed else -1               # the subtracted terms add in the magnitude
        fQ, fR, fA, fB, fM, fd, fq, fc, fr, fx, fy, fu = (list(map(f, t)) for t in (Q, R, A, Bm, M, delta, q, c, r, x, y, u))
        dq, dc, dr = _views(topo, out)
        for i in range(topo.N):
            dq[i][...] = mv(fQ[i], fx[i]) - sgn * fy[i] + fq[i]
        dc[root][...] = -sgn * fx[root] - sgn * fd[root] * fy[root] + fc[root]
        for e in range(topo.E):
            p, ch = topo.parents[e], topo.children[e]
            dq[p][...] += mv(fM[e], fu[e]) + tv(fA[e], fy[ch])
            dr[e][...] = tv(fM[e], fx[p]) + mv(fR[e], fu[e]) + tv(fB[e], fy[ch]) + fr[e]
            dc[ch][...] = mv(fA[e], fx[p]) + mv(fB[e], fu[e]) - sgn * fx[ch] - sgn * fd[ch] * fy[ch] + fc[ch]
    return rho, mag


def k(topo, root=0):
    """[sol_len]: the terms of every entry -- the magnitude expression on all-ones."""
    ones = {"Q": [np.ones((1, n, n)) for n in topo.sd]}
    ones.update({key: [np.ones((1, n)) for n in topo.sd] for key in ("q", "c", "delta")})
    dims = [topo.edge_dims(e) for e in range(topo.E)]                                  # (np, nc, m)
    ones.update({"A": [np.ones((1, nc, np_)) for np_, nc, m in dims], "B": [np.ones((1, nc, m)) for np_, nc, m in dims],
                 "M": [np.ones((1, np_, m)) for np_, nc, m in dims], "R": [np.ones((1, m, m)) for np_, nc, m in dims],
                 "r": [np.ones((1, m)) for np_, nc, m in dims]})
    return np.asarray(residual(topo, ones, None, np.ones((1, topo.layout.sol_len)), np.float64, root)[1][0])


def bound(topo, mag):
    """[B, sol_len]: k 2^-53 a."""
    return k(topo)[None, :] * U * mag


# ---- the trees the residual is run on -------------------------------------------------------------------------------
def batched(prob, B, seed):
    """A reference problem (reference_problems: per-problem blocks) -> (Topology, blocks with a leading batch axis):
    problem 0 is the reference's, the others its entries times (1 + 0.1 N(0,1)), Q and R kept symmetric."""
    topo = fb.Topology(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"])
    rng = np.random.default_rng(seed)
    blocks = {}
    for key, items in prob["blocks"].items():
        blocks[key] = []
        for a in items:
            a = np.asarray(a, dtype=np.float64)
            f = 1.0 + 0.1 * rng.normal(size=(B,) + a.shape)
            f[0] = 1.0
            if key in ("Q", "R"):
                f = _sym(f)
            blocks[key].append(a[None] * f)
    return topo, blocks


def reference_trees():
    """The four small trees of reference_problems.py: a chain with non-uniform delta, the star, the star with
    nc != np, the five-node variable tree."""
    return {"nonuniform_delta_chain": rp.nonuniform_diagonal_delta(), "branch": rp.branch_tree(),
            "variable_branch": rp.variable_dimension_branch(), "five_node": rp.five_node_variable_tree_eigen()}


def random_blocks(topo, B, seed):
    return fb.make_blocks(topo, B, np.random.default_rng(seed), "random")


# ---- the scheme in numpy ---------------------------------------------------------------------------------------------
def model_refine(cell, iterations):
    """The scheme on a tree cell (hard_inputs.tree_cell): the correction solve is the CPU oracle's recursion
    (oracle.tree_batch through full_batch_problems.with_rhs), residual and iterate in float64, starting from zero.
    -> per round the iterate [B, sol_len] and the residual norms [iterations + 1, B]."""
    topo = cell.topo
    z = np.zeros((hi.BATCH, topo.layout.sol_len))
    iterates, norms = [], []
    for _ in range(iterations):
        rho = residual(topo, cell.blocks, None, z, dt=np.float64)[0]
        nrm = np.abs(rho).max(axis=1)
        norms.append(nrm)
        s = scale_of(nrm)
        q, c, r = _views(topo, rho / s[:, None])
        nodes, edges = fb.with_rhs(topo, cell.nodes, cell.edges, {"q": q, "c": c, "r": r})
        d, _, status = oracle.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, nodes, edges, want_gains=False)
        ok = status == 0
        z[ok] += s[ok, None] * d[ok]
        iterates.append(z.copy())
    norms.append(np.abs(residual(topo, cell.blocks, None, z, dt=np.float64)[0]).max(axis=1))
    return iterates, np.stack(norms)


_DROPS = {}


def cells_with_a_drop(factor=100.0):
    """The (dims, axis) cells of hard_inputs.TREES x AXES_TREE on which the model's error falls by at least `factor`
    from round 1 to round 2 (computed once per session): where the GPU must show a drop too."""
    import extended_reference as xr
    if factor not in _DROPS:
        marked = set()
        for dims in hi.TREES:
            for axis in hi.AXES_TREE:
                cell = hi.tree_cell(*dims, axis)
                iterates, _ = model_refine(cell, 2)
                e1, e2 = (xr.err(zz, cell.ext) for zz in iterates)
                if e1 >= factor * e2:
                    marked.add((dims, axis))
        _DROPS[factor] = marked
    return _DROPS[factor]

"""TEST INFRASTRUCTURE ONLY: the hard-input axes of the kernel accuracy tests and the cells (shape x axis) they run on.

An axis modifies a benign draw in place, seeded; it works on `blocks` whose arrays carry a leading batch axis (the form
of tests/full_batch_problems.py), and on the packed chain layout through views of it (chain_views):

  delta[lo,hi]   every delta log-uniform in [lo, hi]
  delta_mixed    every delta log-uniform in [1e-9, 1e6]: fifteen decades inside one node
  cost[1,w]      Q_i += J^T diag(w) J, J ~ N(0,1) of ceil(n_i / 2) rows, w log-uniform in [1, w]: the condensed
                 Newton-KKT shape (V ~ J^T R2^-1 J), the diagonal of F = I + D^1/2 V D^1/2 far from 1
  cost_delta     cost[1,1e4] together with delta[1e-9,1e-7]
  expanding      A_e = 1.5 * (a random orthogonal matrix; its leading nc x np block where the dimensions differ): an
                 antisymmetric part of V would grow by |A|^2 per stage

A cell (chain_cell, tree_cell) is 3 problems with, per problem, the extended-precision solution
(tests/extended_reference.py) and the extended-precision gains, the CPU oracle's solution, gains and statuses, and
e_ref = e(oracle's x, u, y), e_ref_gains = e(oracle's K, k) against them; where a family
needs several right-hand sides, also columns of N(0,1) right-hand sides for the first 2 problems (3 on trees), each
with its own extended solve and oracle solve.  fp32 cells are rounded to fp32 before anything is solved.  Cells are
cached by (shape, axis, dtype): every kernel family at a shape sees the same inputs and the same reference.

The module imports and runs without a GPU."""
import zlib

import numpy as np

import extended_reference as xr
import full_batch_problems as fb
from oracle import oracle

BATCH = 3
AXES_F64 = ["delta[1e-9,1e-7]", "delta[1e-6,1e-4]", "delta[1e-3,1e-1]", "delta[1e2,1e6]", "delta_mixed", "cost[1,1e4]",
            "cost_delta", "expanding"]
AXES_F32 = ["delta[1e-3,1e-1]", "delta[1e-1,1e2]", "cost[1,1e2]", "expanding"]
BENIGN = "delta[1e-3,1e-1]"
# Trees: the stage cost of the random family (full_batch_problems.make_blocks: Q = S^T S + 1e-3 I next to M = 0.05 N on
# every outgoing edge) is not convex -- Q - sum_e M_e R_e^-1 M_e^T has eigenvalues down to -0.008 / -0.019 on the two
# draws used here -- so V has a negative eigenvalue and F = I + D^1/2 V D^1/2 is indefinite once delta exceeds about 50:
# with delta in [1e2, 1e6] the oracle reports F_FACTORIZATION_FAILURE, rightly.  The large-delta axis of the trees is
# therefore weakened to [1, 30], the range this family admits (F >= 1 - 30 * 0.019 > 0).
AXES_TREE = [a if a != "delta[1e2,1e6]" else "delta[1,30]" for a in AXES_F64]

# chain shapes of tests/test_gpu_hard_inputs.py: (n, m) -> columns of the multi-rhs family at that shape (0: none)
CHAINS_F64 = {(12, 4): 8, (5, 3): 0, (15, 8): 0, (16, 4): 0, (8, 4): 0, (10, 3): 0, (16, 8): 8, (32, 8): 9,
              (20, 3): 0, (17, 4): 0, (17, 9): 0}
CHAINS_F32 = {(32, 8): 0, (12, 4): 0, (5, 3): 0}
TREES = [(9, 3), (15, 8)]                      # largest state / control dimension of the random topology
TREE_NODES, TREE_COLS, COL_PROBLEMS = 10, 3, 2


def horizon(n):
    return 12 if n <= 16 else 6


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _logu(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=shape))


def _set_delta(blocks, rng, lo, hi):
    for d in blocks["delta"]:
        d[...] = _logu(rng, lo, hi, d.shape)


def _add_cost(blocks, rng, wmax):
    for Q in blocks["Q"]:
        B, n = Q.shape[0], Q.shape[1]
        if n == 0:
            continue
        rows = (n + 1) // 2
        J = rng.normal(size=(B, rows, n))
        w = _logu(rng, 1.0, wmax, (B, rows))
        Q += J.transpose(0, 2, 1) @ (w[:, :, None] * J)


def _expand(blocks, rng):
    for A in blocks["A"]:
        B, nc, np_ = A.shape
        k = max(nc, np_)
        if min(nc, np_) == 0:
            continue
        Qm = np.linalg.qr(rng.normal(size=(B, k, k)))[0]
        A[...] = 1.5 * Qm[:, :nc, :np_]


def apply(axis, blocks, seed):
    """Modify `blocks` (arrays with a leading batch axis, written in place) along `axis`."""
    rng = np.random.default_rng(_seed("axis", axis, seed))
    if axis.startswith("delta["):
        lo, hi = (float(v) for v in axis[6:-1].split(","))
        _set_delta(blocks, rng, lo, hi)
    elif axis == "delta_mixed":
        _set_delta(blocks, rng, 1e-9, 1e6)
    elif axis.startswith("cost["):
        _add_cost(blocks, rng, float(axis[5:-1].split(",")[1]))
    elif axis == "cost_delta":
        _add_cost(blocks, rng, 1e4)
        _set_delta(blocks, rng, 1e-9, 1e-7)
    elif axis == "expanding":
        _expand(blocks, rng)
    else:
        raise KeyError(axis)


def chain_views(n, m, T, mats):
    """Matrices and delta of packed `mats` [B, mats_len] (numpy) as blocks of views [B, rows, cols]: writing a block
    writes `mats`."""
    from sip_optimal_control_amd import ChainShape
    shape, B = ChainShape(n, m, T), mats.shape[0]
    assert mats.shape == (B, shape.mats_len)

    def mat(off, rows, cols):  # column-major in `mats`
        return mats[:, off:off + rows * cols].reshape(B, cols, rows).transpose(0, 2, 1)

    blocks = {k: [] for k in ("Q", "delta", "A", "B", "M", "R")}
    for i in range(T + 1):
        o = shape.mats_off(i)
        blocks["Q"].append(mat(o["Q"], n, n))
        blocks["delta"].append(mats[:, o["delta"]:o["delta"] + n])
        if i < T:
            blocks["A"].append(mat(o["A"], n, n))
            blocks["B"].append(mat(o["B"], n, m))
            blocks["M"].append(mat(o["M"], n, m))
            blocks["R"].append(mat(o["R"], m, m))
    return blocks


class Cell:
    """Inputs, extended reference and oracle results of one (shape, axis, dtype); see the module docstring."""


def _finish(cell, sd, cd, parents, children, problems, oracle_run, row, col_draw):
    """Extended solves and oracle runs of a cell.  problems: per-problem blocks; oracle_run(columns or None) -> (sol,
    gains, status) of the batch with those right-hand sides; col_draw(rng) -> one right-hand side per problem."""
    cell.ref_sol, cell.ref_gains, cell.ref_status = oracle_run(None)
    rng = np.random.default_rng(_seed("columns", cell.key))
    cell.columns = [col_draw(rng) for _ in range(cell.ncols)]                      # [col] -> batch-wide rhs
    cell.col_ref = [oracle_run(c)[0][:COL_PROBLEMS if cell.chain else BATCH] for c in cell.columns]
    ext, col_ext, ext_gains, cell.correction, cell.gains_tie = [], [], [], 0.0, 0.0
    for b, blocks in enumerate(problems):
        cols = [None]
        if cell.ncols and (not cell.chain or b < COL_PROBLEMS):
            cols += [{k: [a[b] for a in c[k]] for k in ("q", "c", "r")} for c in cell.columns]
        sols, last = xr.Factored(parents, children, sd, cd, blocks).solve(cols)
        cell.correction = max(cell.correction, last)
        ext.append(row(*sols[0]))
        Ks, ks = xr.riccati_gains(parents, children, sd, cd, blocks)
        ext_gains.append(xr.gains_row(Ks, ks))
        x, u, _ = sols[0]      # the dense solve and the recursion are independent: u_e = K_e x_parent(e) + k_e ties them
        cell.gains_tie = max([cell.gains_tie] + [np.abs(u[e] - (Ks[e] @ x[parents[e]] + ks[e])).max(initial=0.0)
                                                 for e in range(len(cd))])
        if len(cols) > 1:
            col_ext.append([row(*s) for s in sols[1:]])
    cell.ext = np.stack(ext)
    cell.col_ext = [np.stack([col_ext[b][c] for b in range(len(col_ext))]) for c in range(cell.ncols)]  # [col][b, len]
    cell.ext_gains = np.stack(ext_gains)
    cell.gains_tie /= np.abs(cell.ext).max()
    cell.e_ref = xr.err(cell.ref_sol, cell.ext)
    cell.e_ref_gains = xr.err(cell.ref_gains, cell.ext_gains)
    cell.e_ref_cols = max([xr.err(r, e) for r, e in zip(cell.col_ref, cell.col_ext)], default=0.0)
    return cell


def chain_cell(n, m, axis, dtype="f64"):
    """The cell of the uniform chain (n, m, T = horizon(n)).  mats, vecs: float64 numpy in the packed layout (fp32
    cells: rounded to fp32, stored as float64); columns[c]: vecs of column c for all problems; col_ext[c] /
    col_ref[c]: [COL_PROBLEMS, vecs_len]."""
    T = horizon(n)
    key = ("chain", n, m, T, axis, dtype)

    def make():
        import torch
        from oracle import dense_kkt
        from sip_optimal_control_amd import ChainShape, synthetic
        mats, vecs = synthetic.make_chain_batch(ChainShape(n, m, T), BATCH, seed=_seed(n, m, T) % 2**31, device="cpu",
                                                cross_term=0.01)
        mats, vecs = mats.numpy().copy(), vecs.numpy().copy()
        apply(axis, chain_views(n, m, T, mats), _seed(n, m, T))
        if dtype == "f32":
            mats, vecs = mats.astype(np.float32).astype(np.float64), vecs.astype(np.float32).astype(np.float64)
        cell = Cell()
        cell.key, cell.chain, cell.shape, cell.axis, cell.dtype = key, True, (n, m, T), axis, dtype
        cell.mats, cell.vecs = mats, vecs
        cell.ncols = (CHAINS_F64 if dtype == "f64" else CHAINS_F32)[(n, m)]
        problems = [dense_kkt.chain_blocks_from_packed(n, m, T, mats[b], vecs[b]) for b in range(BATCH)]

        def col_draw(rng):
            v = rng.normal(size=vecs.shape)
            per = [dense_kkt.chain_blocks_from_packed(n, m, T, mats[b], v[b]) for b in range(BATCH)]
            return {"vecs": v, **{k: [np.stack([p[k][i] for p in per]) for i in range(len(per[0][k]))]
                                  for k in ("q", "c", "r")}}

        def oracle_run(column):
            return oracle.chain_batch(n, m, T, mats, vecs if column is None else column["vecs"])

        return _finish(cell, [n] * (T + 1), [m] * T, list(range(T)), list(range(1, T + 1)), problems, oracle_run,
                       xr.chain_row, col_draw)

    return xr.cached(key, make)


def tree_cell(max_n, max_m, axis):
    """The cell of the random tree of TREE_NODES nodes with largest dimensions (max_n, max_m), two of its nodes of
    dimension 0.  topo: fb.Topology; blocks: arrays with a leading batch axis; nodes, edges: the oracle's packed
    layout; ext / ref_sol in the oracle's sol layout; columns[c]: fb.make_rhs-style right-hand sides."""
    key = ("tree", max_n, max_m, TREE_NODES, axis, "f64")

    def make():
        rng = np.random.default_rng(_seed("tree", max_n, max_m))
        topo = fb.random_topology(rng, TREE_NODES, max_n, max_m)
        blocks = fb.make_blocks(topo, BATCH, rng, "random")
        apply(axis, blocks, _seed(max_n, max_m, TREE_NODES))
        cell = Cell()
        cell.key, cell.chain, cell.axis, cell.dtype, cell.ncols = key, False, axis, "f64", TREE_COLS
        cell.topo, cell.blocks = topo, blocks
        cell.nodes, cell.edges = fb.to_oracle(topo, blocks)

        def oracle_run(column):
            nodes, edges = (cell.nodes, cell.edges) if column is None else fb.with_rhs(topo, cell.nodes, cell.edges, column)
            return oracle.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, nodes, edges)

        return _finish(cell, topo.sd, topo.cd, topo.parents, topo.children, [fb.problem(blocks, b) for b in range(BATCH)],
                       oracle_run, xr.tree_row, lambda r: fb.make_rhs(topo, BATCH, r))

    return xr.cached(key, make)


def cells():
    """Every (kind, shape, axis, dtype) the GPU tests use -- what the CPU test of the references walks."""
    out = [("chain", s, a, "f64") for s in CHAINS_F64 for a in AXES_F64]
    out += [("tree", s, a, "f64") for s in TREES for a in AXES_TREE]
    out += [("chain", s, a, "f32") for s in CHAINS_F32 for a in AXES_F32]
    return out


def cell_of(kind, shape, axis, dtype):
    return chain_cell(*shape, axis, dtype) if kind == "chain" else tree_cell(*shape, axis)

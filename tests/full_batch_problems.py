"""Batches of DISTINCT tree problems for the full-batch parity tests (tests/test_gpu_full_batch.py).

Every block is a numpy array with a leading batch axis (blocks["Q"][i] is [B, n_i, n_i], blocks["A"][e] is
[B, nc_e, np_e], ...), generated without a per-problem Python loop, and the packers move them with one fancy
index per arena: into the packed tree layout of the oracle (oracle.TreeBatchLayout / lqr_oracle_tree_batch) and
into the input arena of a BatchedTreeLQR plan (by its sip_lqr_tree_offset table).  Gathers map the plan's
output / work / multi-rhs arenas back onto the oracle's sol and gains layout.

newton_kkt_batch draws B distinct Newton-KKT problems (model and theta arenas, regularization, right-hand side) the
same way, one vectorised draw per block (tests/test_gpu_kkt_family.py).
"""
import math
import os

import numpy as np

from oracle.oracle import TreeBatchLayout

NODE_BLOCKS = ("Q", "q", "c", "delta")
EDGE_BLOCKS = ("A", "B", "M", "R", "r")


class Topology:
    def __init__(self, parents, children, state_dims, control_dims, name=""):
        self.parents, self.children = list(parents), list(children)
        self.sd, self.cd = list(state_dims), list(control_dims)
        self.E, self.N = len(self.cd), len(self.sd)
        self.name = name
        self.layout = TreeBatchLayout(self.parents, self.children, self.sd, self.cd)

    def edge_dims(self, e):
        """(np, nc, m) of edge e."""
        return self.sd[self.parents[e]], self.sd[self.children[e]], self.cd[e]


def variable_benchmark_topology(shape, T=63, base_n=8, base_m=2):
    """The topologies of tests/reference_problems.variable_benchmark_problem (BM_LQRVariableFactorSolve):
    shape 0 heterogeneous chain, 1 shallow wide tree, 2 binary tree."""
    sd = [max(1, base_n + (node % 3) - 1) for node in range(T + 1)]
    cd = [max(1, base_m + (edge % 3) - 1) for edge in range(T)]
    parents = [{0: e, 1: 0, 2: e // 2}[shape] for e in range(T)]
    return Topology(parents, list(range(1, T + 1)), sd, cd, name=f"variable_benchmark_{shape}")


def random_topology(rng, N, max_n, max_m, zero_nodes=2):
    """A random tree whose largest state / control dimensions are exactly max_n / max_m, with `zero_nodes`
    zero-dimensional non-root nodes."""
    parents = [int(rng.integers(0, e + 1)) for e in range(N - 1)]
    sd = [int(rng.integers(1, max_n + 1)) for _ in range(N)]
    cd = [int(rng.integers(1, max_m + 1)) for _ in range(N - 1)]
    sd[0] = max_n
    cd[int(rng.integers(0, N - 1))] = max_m
    for i in rng.choice(np.arange(1, N), size=zero_nodes, replace=False):
        sd[int(i)] = 0
    return Topology(parents, list(range(1, N)), sd, cd, name=f"random<{max_n},{max_m}>")


def _spd(rng, B, n, shift):
    S = rng.normal(size=(B, n, n))
    return S.transpose(0, 2, 1) @ S + shift * np.eye(n)


def make_blocks(topo, B, rng, family="random"):
    """B distinct problems on `topo`.  family "variable_benchmark": the value distributions of
    reference_problems.variable_benchmark_problem (A = 0.05 N, B = 0.1 N, M = 0); "random": those of the random
    trees of test_gpu_tree.py (A, B = 0.3 N, M = 0.05 N).  R = G^T G + I, Q = S^T S + 1e-3 I,
    delta = 1e-3 + 0.1 U(0, 1), q, r, c ~ N(0, 1) everywhere."""
    sa, sb, sm = (0.05, 0.1, 0.0) if family == "variable_benchmark" else (0.3, 0.3, 0.05)
    blocks = {k: [] for k in NODE_BLOCKS + EDGE_BLOCKS}
    for n in topo.sd:
        blocks["Q"].append(_spd(rng, B, n, 1e-3))
        blocks["q"].append(rng.normal(size=(B, n)))
        blocks["c"].append(rng.normal(size=(B, n)))
        blocks["delta"].append(1e-3 + 0.1 * rng.random((B, n)))
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        blocks["A"].append(sa * rng.normal(size=(B, nc, np_)))
        blocks["B"].append(sb * rng.normal(size=(B, nc, m)))
        blocks["M"].append(sm * rng.normal(size=(B, np_, m)))
        blocks["R"].append(_spd(rng, B, m, 1.0))
        blocks["r"].append(rng.normal(size=(B, m)))
    return blocks


def make_rhs(topo, B, rng):
    """One right-hand side (q, c per node, r per edge) for each of B problems."""
    return {"q": [rng.normal(size=(B, n)) for n in topo.sd], "c": [rng.normal(size=(B, n)) for n in topo.sd],
            "r": [rng.normal(size=(B, m)) for m in topo.cd]}


def problem(blocks, b):
    """Problem b as the per-problem blocks dict of oracle.TreeLQR / BatchedTreeLQR.pack."""
    return {k: [a[b] for a in v] for k, v in blocks.items()}


def _flat(a):
    """[B, rows, cols] -> [B, rows * cols] column-major; [B, n] unchanged."""
    return a.transpose(0, 2, 1).reshape(a.shape[0], -1) if a.ndim == 3 else a


def to_oracle(topo, blocks):
    """-> (nodes, edges) [B, len] in the packed tree layout of lqr_oracle_tree_batch."""
    lay = topo.layout
    B = blocks["Q"][0].shape[0]
    nodes, edges = np.zeros((B, lay.nodes_len)), np.zeros((B, lay.edges_len))
    for i in range(topo.N):
        row = np.concatenate([_flat(blocks[k][i]) for k in NODE_BLOCKS], axis=1)
        nodes[:, lay.node_off[i]:lay.node_off[i] + row.shape[1]] = row
    for e in range(topo.E):
        row = np.concatenate([_flat(blocks[k][e]) for k in EDGE_BLOCKS], axis=1)
        edges[:, lay.edge_off[e]:lay.edge_off[e] + row.shape[1]] = row
    return nodes, edges


def with_rhs(topo, nodes, edges, rhs):
    """Copies of the oracle arenas with q, c, r replaced by those of `rhs`."""
    lay = topo.layout
    nodes, edges = nodes.copy(), edges.copy()
    for i, n in enumerate(topo.sd):
        o = lay.node_off[i] + n * n
        nodes[:, o:o + n] = rhs["q"][i]
        nodes[:, o + n:o + 2 * n] = rhs["c"][i]
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        o = lay.edge_off[e] + nc * np_ + nc * m + np_ * m + m * m
        edges[:, o:o + m] = rhs["r"][e]
    return nodes, edges


class PlanMaps:
    """Index maps between a BatchedTreeLQR plan's arenas and the oracle's packed tree layout (one topology)."""

    def __init__(self, s, topo):
        lay = topo.layout
        max_n = max(topo.sd)
        # input arena <- [nodes | edges] of the oracle (the plan stores each node block Q|q|c|delta and each
        # edge block A|B|M|R|r contiguously, as BatchedTreeLQR.pack writes them)
        src = []
        for i, n in enumerate(topo.sd):
            src.append(s.offset(0, 0, i) + np.arange(n * n + 3 * n))
        for e in range(topo.E):
            np_, nc, m = topo.edge_dims(e)
            src.append(s.offset(0, 1, e) + np.arange(nc * np_ + nc * m + np_ * m + m * m + m))
        self.input_idx = np.concatenate(src).astype(np.int64)
        assert self.input_idx.size == lay.nodes_len + lay.edges_len
        # output arena -> oracle sol (x_i | y_i per node, then u_e per edge)
        sol = [s.offset(2, 0, i) + np.arange(2 * n) for i, n in enumerate(topo.sd)]
        sol += [s.offset(2, 1, e) + np.arange(m) for e, m in enumerate(topo.cd)]
        self.sol_idx = np.concatenate(sol).astype(np.int64)
        assert self.sol_idx.size == lay.sol_len
        # work arena -> oracle gains (K_e | k_e per edge): K at +max_n^2 (after W), k after K and G_factor
        g = []
        for e in range(topo.E):
            np_, nc, m = topo.edge_dims(e)
            o = s.offset(1, 1, e) + max_n * max_n
            g += [o + np.arange(m * np_), o + m * np_ + m * m + np.arange(m)]
        self.gains_idx = np.concatenate(g).astype(np.int64) if g else np.zeros(0, np.int64)
        # multi-rhs arena of one column <- q | c per node, r per edge (oracle problem order)
        r = [s._lib.sip_lqr_tree_rhs_offset(s._plan, 0, i) + np.arange(2 * n) for i, n in enumerate(topo.sd)]
        r += [s._lib.sip_lqr_tree_rhs_offset(s._plan, 1, e) + np.arange(m) for e, m in enumerate(topo.cd)]
        self.rhs_idx = np.concatenate(r).astype(np.int64)
        # blocks of the oracle sol / gains layouts (for the per-block scale): start offsets of non-empty blocks
        self.sol_blocks = _starts([n for n in topo.sd for _ in range(2)] + topo.cd)
        self.gains_blocks = _starts([x for e in range(topo.E) for x in (topo.cd[e] * topo.sd[topo.parents[e]],
                                                                          topo.cd[e])])

    def pack_input(self, s, nodes, edges):
        host = np.zeros((nodes.shape[0], s.input.shape[1]))
        host[:, self.input_idx] = np.concatenate([nodes, edges], axis=1)
        return host

    def pack_rhs(self, s, rhs):
        """One column's right-hand side -> [B, rhs_len]."""
        B = rhs["q"][0].shape[0]
        host = np.zeros((B, max(1, s.rhs_len)))
        vals = [a for i in range(len(rhs["q"])) for a in (rhs["q"][i], rhs["c"][i])] + list(rhs["r"])
        host[:, self.rhs_idx] = np.concatenate(vals, axis=1)
        return host


def _starts(sizes):
    """Start offsets of the non-empty blocks of a contiguous layout with these block sizes."""
    out, o = [], 0
    for k in sizes:
        if k > 0:
            out.append(o)
        o += k
    return np.array(out, dtype=np.int64)


def block_rel_err(got, ref, starts):
    """Worst |got - ref| per problem, each block relative to max(1, max |ref| of that block) (the scale of
    test_gpu_tree._check_against_oracle): [B]."""
    if starts.size == 0:
        return np.zeros(got.shape[0])
    err = np.maximum.reduceat(np.abs(got - ref), starts, axis=1)
    scale = np.maximum(1.0, np.maximum.reduceat(np.abs(ref), starts, axis=1))
    return (err / scale).max(axis=1)


def assert_discriminates(ref, tol, rows=None, what=""):
    """The comparison at `tol` can tell neighbouring problems apart: for every problem p (of `rows`, default
    all), max |ref[p] - ref[q]| relative to max(1, max |ref[p]|) is at least 1e3 * tol for q = p +- 1 (the
    neighbouring row of the wavefront) and q = p +- 4 (the same row of the neighbouring wavefront)."""
    B = ref.shape[0]
    rows = np.arange(B) if rows is None else np.asarray(rows)
    scale = np.maximum(1.0, np.abs(ref[rows]).max(axis=1))
    for d in (-4, -1, 1, 4):
        q = rows + d
        ok = (q >= 0) & (q < B)
        if not ok.any():                                         # a batch too small to have this neighbour
            continue
        gap =np.abs(ref[rows[ok]] - ref[q[ok]]).max(axis=1) / scale[ok]
        assert gap.min() >= 1e3 * tol, (what, d, float(gap.min()), int(rows[ok][gap.argmin()]))


def oracle_threads():
    """Threads for the CPU oracle: the smallest of OMP_NUM_THREADS (when set), the CPUs this process may run on,
    and 16 (os.cpu_count() reports the whole host, not what the process may use)."""
    n = min(16, len(os.sched_getaffinity(0)))
    try:
        n = min(n, int(os.environ.get("OMP_NUM_THREADS", "").split(",")[0]))
    except ValueError:
        pass
    return max(1, n)


# ---- Newton-KKT problems ------------------------------------------------------------------------------------------
def newton_kkt_batch(dims, B, seed, r2_max=1e2, device="cpu"):
    """B distinct Newton-KKT problems on `dims` (an oracle.kkt.KKTDims, any tree / dimensions, with or without
    theta), with the value distributions of reference_kkt_problems.newton_kkt_problem (newton_kkt_benchmark.cpp
    :170-262): dc / dg Jacobians 0.1 N(0,1), node d2L_dx2 = S^T S + 1e-3 I, ddyn_dx = I + 0.05 N(0,1), ddyn_du
    0.1 N(0,1), edge d2L_dx2 = 0, d2L_dxdu 0.01 N(0,1), d2L_du2 = S^T S + I; theta couplings 1e-3 N(0,1),
    d2L_dtheta2 = S^T S + 100 I on the last node and 0 elsewhere; r2 log-uniform [1e-3, r2_max], w [1e-2, 1e3],
    r3 [1e-3, 1e1], r1 = 1e-8, rhs N(0,1).  Every block is one draw with a leading batch axis, placed at the
    offsets of dims (the plan's model_offset / theta_offset tables).

    Returns float64 torch tensors on `device`, each [B, len]: (model, w, r1, r2, r3, rhs), and theta_model when
    dims.p > 0 (then r1 and rhs include the theta columns, as for BatchedNewtonKKT.factor_theta / solve_theta)."""
    import torch
    from oracle.kkt import EDGE_BLOCKS, NODE_BLOCKS, THETA_EDGE_BLOCKS, THETA_NODE_BLOCKS
    f64 = torch.float64
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)

    def randn(rows, cols, scale):
        return scale * torch.randn(B, rows, cols, generator=gen, device=device, dtype=f64)

    def spd(k, shift):
        S = randn(k, k, 1.0)
        return S.transpose(1, 2) @ S + shift * torch.eye(k, device=device, dtype=f64)

    def put(arena, off, mat):  # [B, rows, cols] -> column-major block at off
        if mat.shape[1] * mat.shape[2]:
            arena[:, off:off + mat.shape[1] * mat.shape[2]] = mat.transpose(1, 2).reshape(B, -1)

    def edge_eye(nc, np_):
        return torch.eye(nc, np_, device=device, dtype=f64).expand(B, nc, np_)

    model = torch.zeros(B, max(1, dims.model_len), dtype=f64, device=device)
    node_draw = {"d2L_dx2": lambda n, c, g: spd(n, 1e-3), "dc_dx": lambda n, c, g: randn(c, n, 0.1),
                 "dg_dx": lambda n, c, g: randn(g, n, 0.1)}
    for i in range(dims.N):
        for b in NODE_BLOCKS:
            put(model, dims.node_off[b][i], node_draw[b](dims.sd[i], dims.ncd[i], dims.ngd[i]))
    for e in range(dims.E):
        np_, nc, m = dims.sd[dims.parents[e]], dims.sd[dims.children[e]], dims.cd[e]
        for b, (r, c) in zip(EDGE_BLOCKS, dims.edge_shapes(e)):
            if b == "d2L_dx2":
                continue  # 0
            mat = spd(m, 1.0) if b == "d2L_du2" else \
                edge_eye(nc, np_) + randn(nc, np_, 0.05) if b == "ddyn_dx" else \
                randn(r, c, 0.01 if b == "d2L_dxdu" else 0.1)
            put(model, dims.edge_off[b][e], mat)

    def logu(lo, hi, length):
        u = torch.rand(B, length, generator=gen, device=device, dtype=f64)
        return torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * u)

    r2 = logu(1e-3, r2_max, dims.y_dim)
    w = logu(1e-2, 1e3, dims.z_dim)
    r3 = logu(1e-3, 1e1, dims.z_dim)
    r1 = torch.full((B, dims.x_dim + dims.p), 1e-8, dtype=f64, device=device)
    rhs = torch.randn(B, dims.full_dim, generator=gen, device=device, dtype=f64)
    out = [model, w, r1, r2, r3, rhs]
    if dims.p > 0:
        theta = torch.zeros(B, max(1, dims.theta_len), dtype=f64, device=device)
        for i in range(dims.N):
            for b, (r, c) in zip(THETA_NODE_BLOCKS, dims.theta_node_shapes(i)):
                if b != "d2L_dtheta2":
                    put(theta, dims.theta_node_off[b][i], randn(r, c, 1e-3))
                elif i == dims.E:
                    put(theta, dims.theta_node_off[b][i], spd(dims.p, 100.0))
        for e in range(dims.E):
            for b, (r, c) in zip(THETA_EDGE_BLOCKS, dims.theta_edge_shapes(e)):
                if b != "d2L_dtheta2":
                    put(theta, dims.theta_edge_off[b][e], randn(r, c, 1e-3))
        out.append(theta)
    return tuple(out)

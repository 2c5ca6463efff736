"""Every benchmark-family Newton-KKT chain kernel against the CPU oracle, at every problem of the batch.

A uniform chain whose dimensions are those of the reference's NewtonKKTProblem (n in {4, 6, 8, 12}, m in 1..4,
c = n/2 and g = 2m rows on every edge and on the last node, no interior-node constraints) runs the chain kernels as
the instantiation with every dimension but the horizon a constant (kkt_chain_kernels.hpp: family_dims; the plan's row
of the table of kkt_chain_launch.hpp, instantiated in kkt_chain_kernels.hip): unrolled loops, folded branches and other register caps than the generic
(FN = 0) kernels, so a bug can live in one (n, m) or one entry point alone.  Here all 16 shapes run every entry
point -- the step (fused and split, every condensation switch), y += K x, the five block operators and the theta
Schur complement -- on 1031 distinct problems at T = 13 (1031 x 14 stages is not a multiple of the 6 stages per
wavefront of the pipelined condensation), and the f2 / f4 benchmark configurations at batch 4096.

Conventions of test_gpu_full_batch.py: every problem is checked, each comparison first asserts that the reference
can tell neighbouring problems apart, and a sentinel row past the end of every output arena must come back bitwise
unchanged.  Residuals and operators are the oracle's, never the GPU's.  Tolerances are the existing ones
(test_gpu_kkt.py): 1e-9 relative to the row max for step solutions, 1e-9 x max(1, |ref|) for operators, 1e-8 for
theta solutions; 1e-12 between two GPU paths that differ only in rounding (the chain-vs-tables bound), 1e-11
between the fused and generic theta passes.  The worst error of every comparison is printed."""
import concurrent.futures
import functools
import zlib

import numpy as np
import pytest

import full_batch_problems as fb
from oracle.kkt import EDGE_BLOCKS, NODE_BLOCKS, THETA_EDGE_BLOCKS, THETA_NODE_BLOCKS, KKTDims, KKTOracle
from tests import reference_kkt_problems as rk

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(n, m) for n in (4, 6, 8, 12) for m in (1, 2, 3, 4)]
BATCH, T = 1031, 13
REL, THETA_TOL, PAIR_TOL, THETA_PAIR_TOL = 1e-9, 1e-8, 1e-12, 1e-11
F_SENTINEL = -3.0e33
I_SENTINEL = 0x5EED5EED
TAG = "[benchmark-family instantiation]"
PACKED = {(4, 4), (8, 4), (12, 4)}  # the family shapes whose sweep reads Q | R packed (SIP_KKT_SYM)
THREADS = fb.oracle_threads()
OPS = ("Hx", "Cx", "CTx", "Gx", "GTx")
SPACE = {"Hx": ("x", "x"), "Cx": ("x", "y"), "CTx": ("y", "x"), "Gx": ("x", "z"), "GTx": ("z", "x")}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _dims(n, m, T, p=0, **over):
    """NewtonKKTProblem(n, m, T) dimension tables, with some of them replaced (near misses)."""
    d = rk.newton_kkt_dims(n, m, T)
    kw = dict(node_c=d.ncd, node_g=d.ngd, edge_c=d.ecd, edge_g=d.egd)
    kw.update(over)
    return KKTDims(d.parents, d.children, d.sd, d.cd, theta_dim=p, **kw)


def _plan(dims, batch, env=None, monkeypatch=None):
    """A plan created under the environment `env`, whose status is a view of an arena one row longer (sentinel)."""
    from sip_optimal_control_amd import BatchedNewtonKKT
    with monkeypatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        kkt = BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd,
                               dims.egd, batch=batch, root=dims.root, theta_dim=dims.p)
    assert (kkt.x_dim, kkt.y_dim, kkt.z_dim, kkt.model_len) == (dims.x_dim, dims.y_dim, dims.z_dim, dims.model_len)
    full = torch.full((batch + 1,), I_SENTINEL, dtype=torch.int32, device=kkt.device)
    kkt.status, kkt.status_guarded = full[:batch], full
    return kkt


def _guarded(rows, width, init=None):
    """[rows + 1, width] on the GPU: the first rows `init` (or the sentinel), the last one the sentinel."""
    full = torch.full((rows + 1, width), F_SENTINEL, dtype=torch.float64, device="cuda")
    if init is not None:
        full[:rows] = torch.from_numpy(np.ascontiguousarray(init)).cuda()
    return full


def _host(full, rows, what):
    """Rows of a guarded arena; its sentinel row must be untouched."""
    torch.cuda.synchronize()
    h = full.cpu().numpy()
    assert (h[rows] == F_SENTINEL).all(), f"{what}: the row past the batch was written"
    return h[:rows]


def _status(kkt, what):
    torch.cuda.synchronize()
    s = kkt.status_guarded.cpu().numpy()
    assert s[kkt.batch] == I_SENTINEL, f"{what}: the status past the batch was written"
    return s[:kkt.batch]


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


def _rel_rows(got, ref):
    """max |got - ref| per row relative to max |ref| of the row."""
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


def _op_rows(got, ref):
    """max |got - ref| per row relative to max(1, max |ref| of the row) (the operator scale of test_gpu_kkt)."""
    return np.abs(got - ref).max(axis=1, initial=0.0) / np.maximum(1.0, np.abs(ref).max(axis=1, initial=0.0))


def _worst(err, rows, what, tol):
    rows = np.asarray(rows)
    i = int(np.argmax(err)) if err.size else 0
    worst = float(err[i]) if err.size else 0.0
    print(f"  {what}: worst {worst:.2e} (problem {int(rows[i]) if err.size else -1})")
    assert worst <= tol, (what, worst, int(rows[i]))
    return worst


def _pool(dims, fn, rows):
    """[fn(oracle, q) for q in rows] over THREADS threads with one KKTOracle each (ctypes drops the GIL)."""
    oracles = [KKTOracle(dims) for _ in range(THREADS)]
    chunks = np.array_split(np.asarray(rows, dtype=np.int64), THREADS)
    with concurrent.futures.ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(lambda a: [fn(a[0], int(q)) for q in a[1]], zip(oracles, chunks)))
    return [r for part in parts for r in part]


def _set_block(dims, model_row, name, e, mat):
    o = dims.edge_off[name][e]
    model_row[o:o + mat.size] = mat.reshape(-1, order="F")


@functools.lru_cache(maxsize=None)
def _step_problems(n, m, T, batch, inject):
    """(dims, (model, w, r1, r2, r3, rhs) numpy, expected statuses, oracle solution, oracle statuses).  With
    `inject`: r2 = 0 on an edge-constraint row of problem 0 (status 5), d2L_du2 = -5 I on a middle edge of problem
    515 (status 3), w + r3 = 0 on the last problem (status 5)."""
    dims = _dims(n, m, T)
    arrays = tuple(a.numpy() for a in fb.newton_kkt_batch(dims, batch, seed=_seed(n, m, T, batch)))
    model, w, r1, r2, r3, rhs = arrays
    expect = np.zeros(batch, dtype=np.int32)
    if inject:
        mid = dims.E // 2
        r2[0, dims.off["y_edge_c"][mid] + dims.ecd[mid] - 1] = 0.0
        _set_block(dims, model[515], "d2L_du2", mid, -5.0 * np.eye(m))
        z = dims.off["z_edge"][mid]
        w[batch - 1, z] = -r3[batch - 1, z]
        expect[[0, 515, batch - 1]] = [5, 3, 5]
    ref, ref_st = KKTOracle(dims).batch(*arrays, threads=THREADS)
    np.testing.assert_array_equal(ref_st, expect)          # the oracle agrees with the construction
    return dims, arrays, expect, ref, ref_st


# ---- a. dispatch --------------------------------------------------------------------------------------------------
def test_every_family_shape_dispatches_to_its_instantiation(monkeypatch):
    """All 16 shapes run their family instantiation (SIP_KKT_FAMILY=0: the generic kernels), and the plan's model
    and theta arenas are laid out as the dimension tables the generator writes by."""
    for n, m in SHAPES:
        dims = _dims(n, m, T, 8)
        kkt = _plan(dims, 4, monkeypatch=monkeypatch)
        for b, name in enumerate(NODE_BLOCKS):
            assert [kkt.model_offset(b, i) for i in range(dims.N)] == dims.node_off[name]
        for b, name in enumerate(EDGE_BLOCKS):
            assert [kkt.model_offset(len(NODE_BLOCKS) + b, e) for e in range(dims.E)] == dims.edge_off[name]
        for b, name in enumerate(THETA_NODE_BLOCKS):
            assert [kkt.theta_offset(b, i) for i in range(dims.N)] == dims.theta_node_off[name]
        for b, name in enumerate(THETA_EDGE_BLOCKS):
            assert [kkt.theta_offset(len(THETA_NODE_BLOCKS) + b, e) for e in range(dims.E)] == \
                dims.theta_edge_off[name]
        assert kkt.theta_len == dims.theta_len
        dims = _dims(n, m, T)
        name = _plan(dims, 4, monkeypatch=monkeypatch).kernel_name
        assert "chain condensation" in name and TAG in name, (n, m, name)
        generic = _plan(dims, 4, {"SIP_KKT_FAMILY": "0"}, monkeypatch).kernel_name
        assert "chain condensation" in generic and TAG not in generic, (n, m, generic)
        assert generic == name.replace(" " + TAG, ""), (name, generic)


NEAR_MISSES = {
    "12_4_edge_c5": (12, 4, dict(edge_c=[5] * T)),
    "8_2_terminal_g3": (8, 2, dict(node_g=[0] * T + [3])),
    "6_3_interior_node_c1": (6, 3, dict(node_c=[1] * T + [3])),   # chain kernels, but cn != 0
    "10_4": (10, 4, {}),
    "12_5": (12, 5, {}),
}


@pytest.mark.parametrize("case", sorted(NEAR_MISSES))
def test_near_miss_plans_run_the_generic_kernels(monkeypatch, case):
    """A plan one dimension away from the family must not run a family instantiation (it would use the hard-wired
    c and g), and must match the oracle."""
    n, m, over = NEAR_MISSES[case]
    dims, batch = _dims(n, m, T, **over), 7
    kkt = _plan(dims, batch, monkeypatch=monkeypatch)
    assert "chain condensation" in kkt.kernel_name and TAG not in kkt.kernel_name, kkt.kernel_name
    arrays = tuple(a.numpy() for a in fb.newton_kkt_batch(dims, batch, seed=_seed(case)))
    ref, ref_st = KKTOracle(dims).batch(*arrays, threads=THREADS)
    assert (ref_st == 0).all()
    d = _dev(*arrays)
    out = _guarded(batch, dims.kkt_dim)
    kkt.factor_solve(*d, sol=out[:batch])
    got = _host(out, batch, "sol")
    assert (_status(kkt, "step") == 0).all()
    print(f"{case}: {kkt.kernel_name}")
    _worst(_rel_rows(got, ref), range(batch), "step", REL)
    rng = np.random.default_rng(_seed(case, "x"))
    x, y0 = rng.standard_normal((2, batch, dims.kkt_dim))
    y = _guarded(batch, dims.kkt_dim, y0)
    kkt.add_Kx_to_y(*d[:5], _dev(x)[0], y=y[:batch])
    got = _host(y, batch, "y")
    o = KKTOracle(dims)
    ref = np.stack([o.add_Kx_to_y(*[a[q] for a in arrays[:5]], x[q], y=y0[q]) for q in range(batch)])
    _worst(_op_rows(got, ref), range(batch), "add_Kx_to_y", REL)


# ---- b. the step, every shape ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SHAPES)
def test_step_every_shape(monkeypatch, n, m):
    """factor_solve and factor + solve, with failures at problems 0, 515 and the last one, against the oracle; the
    one-stage condensation, the copying condensation and the full-square Q | R bitwise equal to the default; the
    generic kernels (SIP_KKT_FAMILY=0) equal to rounding."""
    dims, arrays, expect, ref, _ = _step_problems(n, m, T, BATCH, True)
    ok, bad = np.flatnonzero(expect == 0), np.flatnonzero(expect != 0)
    fb.assert_discriminates(ref, REL, rows=ok, what="step")
    d = _dev(*arrays)

    def run(env, split=False):
        kkt = _plan(dims, BATCH, env, monkeypatch)
        out = _guarded(BATCH, dims.kkt_dim)
        if split:
            kkt.factor(*d[:5])
            np.testing.assert_array_equal(_status(kkt, "factor"), expect)
            kkt.solve(d[0], d[5], sol=out[:BATCH])
        else:
            kkt.factor_solve(*d, sol=out[:BATCH])
        got = _host(out, BATCH, "sol")
        np.testing.assert_array_equal(_status(kkt, "step"), expect)
        assert (got[bad] == F_SENTINEL).all(), "a failed problem's solution was written"
        return got[ok], kkt.kernel_name

    print(f"({n}, {m}) T {T} batch {BATCH}")
    base, name = run({})
    assert TAG in name and "chain condensation" in name, name
    assert ("Q|R packed" in name) == ((n, m) in PACKED), name
    _worst(_rel_rows(base, ref[ok]), ok, f"{name}: factor_solve vs oracle", REL)
    split, _ = run({}, split=True)
    _worst(_rel_rows(split, ref[ok]), ok, "factor + solve vs oracle", REL)
    _worst(_rel_rows(split, base), ok, "factor + solve vs factor_solve", PAIR_TOL)
    switches = [{"SIP_KKT_PIPE": "0"}, {"SIP_KKT_SPLIT": "0"}] + ([{"SIP_KKT_SYM": "0"}] if (n, m) in PACKED else [])
    for env in switches:
        got, other = run(env)
        assert TAG in other, other
        if "SIP_KKT_SPLIT" in env:
            assert "A|B in place" not in other, other
        if "SIP_KKT_SYM" in env:
            assert "Q|R packed" not in other and "A|B in place" in other, other
        mism = np.flatnonzero((got != base).any(axis=1))
        assert mism.size == 0, (env, "not bitwise the default", ok[mism[:5]])
    generic, gname = run({"SIP_KKT_FAMILY": "0"})
    assert TAG not in gname, gname
    _worst(_rel_rows(generic, ref[ok]), ok, "SIP_KKT_FAMILY=0 vs oracle", REL)
    _worst(_rel_rows(base, generic), ok, "family vs SIP_KKT_FAMILY=0", PAIR_TOL)


# ---- c. operators, every shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SHAPES)
def test_operators_every_shape(monkeypatch, n, m):
    """add_Kx_to_y (accumulating onto a nonzero y0) and the five block operators, every problem against the
    oracle's operator, and the family instantiation against the generic kernels."""
    dims, arrays, _, _, _ = _step_problems(n, m, T, BATCH, True)
    model = arrays[0]
    rng = np.random.default_rng(_seed(n, m, "operators"))
    dim = {"x": dims.x_dim, "y": dims.y_dim, "z": dims.z_dim}
    x, y0 = rng.standard_normal((2, BATCH, dims.kkt_dim))
    vx = {s: rng.standard_normal((BATCH, dim[s])) for s in "xyz"}
    vy = {op: rng.standard_normal((BATCH, dim[SPACE[op][1]])) for op in OPS}

    def ref_one(o, q):
        out = [o.add_Kx_to_y(*[a[q] for a in arrays[:5]], x[q], y=y0[q])]
        out += [o.add_block_to_y(op, model[q], vx[SPACE[op][0]][q], y=vy[op][q]) for op in OPS]
        return out

    refs = _pool(dims, ref_one, range(BATCH))
    ref = {"Kx": np.stack([r[0] for r in refs])}
    ref.update({op: np.stack([r[1 + k] for r in refs]) for k, op in enumerate(OPS)})
    for key, r in ref.items():
        fb.assert_discriminates(r, REL, what=key)
    d = _dev(*arrays)
    d_x, d_v = _dev(x)[0], {s: _dev(v)[0] for s, v in vx.items()}
    got = {}
    print(f"({n}, {m}) T {T} batch {BATCH}")
    for env in ({}, {"SIP_KKT_FAMILY": "0"}):
        kkt = _plan(dims, BATCH, env, monkeypatch)
        assert (TAG in kkt.kernel_name) == (not env), kkt.kernel_name
        y = _guarded(BATCH, dims.kkt_dim, y0)
        kkt.add_Kx_to_y(*d[:5], d_x, y=y[:BATCH])
        res = {"Kx": _host(y, BATCH, "add_Kx_to_y")}
        for op in OPS:
            yb = _guarded(BATCH, dim[SPACE[op][1]], vy[op])
            kkt.add_block_to_y(op, d[0], d_v[SPACE[op][0]], y=yb[:BATCH])
            res[op] = _host(yb, BATCH, op)
        tag = "family" if not env else "SIP_KKT_FAMILY=0"
        for key, r in ref.items():
            _worst(_op_rows(res[key], r), range(BATCH), f"{tag} {key} vs oracle", REL)
        got[tag] = res
    for key in ref:
        _worst(_op_rows(got["family"][key], got["SIP_KKT_FAMILY=0"][key]), range(BATCH),
               f"{key} family vs SIP_KKT_FAMILY=0", PAIR_TOL)


# ---- d. theta, every shape ---------------------------------------------------------------------------------------
THETA_CASES = [(n, m, p) for n, m in SHAPES for p in (4, 8)] + [(6, 3, 3), (12, 1, 3)]
THETA_BAD = 515


def _theta_reference(dims, arrays, theta, x, vx):
    """Per problem: (status, solution or None, K x with theta, the five theta block operators) from the oracle."""
    model, w, r1, r2, r3, rhs = arrays

    def one(o, q):
        st = o.factor_theta(model[q], theta[q], w[q], r1[q], r2[q], r3[q])
        sol = o.solve_theta(model[q], theta[q], rhs[q]) if st == 0 else None
        kx = o.add_Kx_to_y_theta(model[q], theta[q], w[q], r1[q], r2[q], r3[q], x[q])
        ops = [o.add_block_to_y(op, model[q], vx[SPACE[op][0]][q], theta_model=theta[q]) for op in OPS]
        return st, sol, kx, ops

    return _pool(dims, one, range(x.shape[0]))


def _theta_check(monkeypatch, dims, batch, arrays, theta, bad, label):
    """factor_theta / solve_theta / add_Kx_to_y_theta / the _theta block operators of the family plan, fused and
    generic theta passes, against the oracle at every problem; fused against generic."""
    model, w, r1, r2, r3, rhs = arrays
    rng = np.random.default_rng(_seed(label, "x"))
    dim = {"x": dims.x_dim + dims.p, "y": dims.y_dim, "z": dims.z_dim}
    x = rng.standard_normal((batch, dims.full_dim))
    vx = {s: rng.standard_normal((batch, dim[s])) for s in "xyz"}
    refs = _theta_reference(dims, arrays, theta, x, vx)
    expect = np.array([r[0] for r in refs], dtype=np.int32)
    want = np.zeros(batch, dtype=np.int32)
    want[bad] = 7
    np.testing.assert_array_equal(expect, want)
    ok = np.flatnonzero(expect == 0)
    ref_sol = np.stack([refs[q][1] for q in ok])
    ref_kx = np.stack([r[2] for r in refs])
    ref_ops = {op: np.stack([r[3][k] for r in refs]) for k, op in enumerate(OPS)}
    fb.assert_discriminates(ref_sol, THETA_TOL, what="theta sol")
    fb.assert_discriminates(ref_kx, REL, what="theta Kx")
    d = _dev(model, theta, w, r1, r2, r3, rhs)
    d_x, d_v = _dev(x)[0], {s: _dev(v)[0] for s, v in vx.items()}
    got = {}
    print(f"{label} batch {batch}")
    for fused in ("1", "0"):
        kkt = _plan(dims, batch, {"SIP_KKT_THETA_FUSED": fused}, monkeypatch)
        assert TAG in kkt.kernel_name and ("fused theta passes" in kkt.kernel_name) == (fused == "1"), \
            kkt.kernel_name
        kkt.factor_theta(*d[:6])
        np.testing.assert_array_equal(_status(kkt, "factor_theta"), expect)
        out = _guarded(batch, dims.full_dim)
        kkt.solve_theta(d[0], d[1], d[6], sol=out[:batch])
        sol = _host(out, batch, "solve_theta")
        assert (sol[bad] == F_SENTINEL).all(), "a failed problem's solution was written"
        y = _guarded(batch, dims.full_dim, np.zeros((batch, dims.full_dim)))
        kkt.add_Kx_to_y_theta(*d[:6], d_x, y=y[:batch])
        res = {"sol": sol[ok], "Kx": _host(y, batch, "add_Kx_to_y_theta")}
        for op in OPS:
            yb = _guarded(batch, dim[SPACE[op][1]], np.zeros((batch, dim[SPACE[op][1]])))
            kkt.add_block_to_y(op, d[0], d_v[SPACE[op][0]], y=yb[:batch], theta_model=d[1])
            res[op] = _host(yb, batch, op + "_theta")
        tag = f"THETA_FUSED={fused}"
        _worst(_rel_rows(res["sol"], ref_sol), ok, f"{tag} solve_theta vs oracle", THETA_TOL)
        _worst(_op_rows(res["Kx"], ref_kx), range(batch), f"{tag} add_Kx_to_y_theta vs oracle", REL)
        for op in OPS:
            _worst(_op_rows(res[op], ref_ops[op]), range(batch), f"{tag} {op}_theta vs oracle", REL)
        got[fused] = res
    _worst(_rel_rows(got["1"]["sol"], got["0"]["sol"]), ok, "solve_theta fused vs generic", THETA_PAIR_TOL)
    for key in ["Kx"] + list(OPS):
        _worst(_op_rows(got["1"][key], got["0"][key]), range(batch), f"{key} fused vs generic", PAIR_TOL)


@pytest.mark.parametrize("n,m,p", THETA_CASES)
def test_theta_every_shape(monkeypatch, n, m, p):
    dims = _dims(n, m, T, p)
    arrays = [a.numpy() for a in fb.newton_kkt_batch(dims, BATCH, seed=_seed(n, m, p, "theta"))]
    theta = arrays.pop()
    theta[THETA_BAD] = rk.initialize_theta_model(dims, -50.0)   # an indefinite Schur complement: status 7
    _theta_check(monkeypatch, dims, BATCH, arrays, theta, [THETA_BAD], f"theta ({n}, {m}) p {p} T {T}")


# ---- e. short horizons -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("horizon,batch", [(1, 3), (2, 3), (1, 1)])
@pytest.mark.parametrize("n,m", SHAPES)
def test_short_horizons(monkeypatch, n, m, horizon, batch):
    """T = 1 (E == 1: the one-interior-node branch of the chain setup) and T = 2: the step and y += K x."""
    dims, arrays, _, ref, _ = _step_problems(n, m, horizon, batch, False)
    kkt = _plan(dims, batch, monkeypatch=monkeypatch)
    assert TAG in kkt.kernel_name, kkt.kernel_name
    d = _dev(*arrays)
    out = _guarded(batch, dims.kkt_dim)
    kkt.factor_solve(*d, sol=out[:batch])
    got = _host(out, batch, "sol")
    assert (_status(kkt, "step") == 0).all()
    print(f"({n}, {m}) T {horizon} batch {batch}")
    _worst(_rel_rows(got, ref), range(batch), "factor_solve vs oracle", REL)
    kkt.factor(*d[:5])
    assert (_status(kkt, "factor") == 0).all()
    out = _guarded(batch, dims.kkt_dim)
    kkt.solve(d[0], d[5], sol=out[:batch])
    _worst(_rel_rows(_host(out, batch, "sol"), ref), range(batch), "factor + solve vs oracle", REL)
    rng = np.random.default_rng(_seed(n, m, horizon, batch, "x"))
    x, y0 = rng.standard_normal((2, batch, dims.kkt_dim))
    y = _guarded(batch, dims.kkt_dim, y0)
    kkt.add_Kx_to_y(*d[:5], _dev(x)[0], y=y[:batch])
    o = KKTOracle(dims)
    ref_y = np.stack([o.add_Kx_to_y(*[a[q] for a in arrays[:5]], x[q], y=y0[q]) for q in range(batch)])
    _worst(_op_rows(_host(y, batch, "y"), ref_y), range(batch), "add_Kx_to_y vs oracle", REL)


# ---- f. the f2 / f4 benchmark configurations at full batch --------------------------------------------------------
F_BATCH, F_BAD = 4096, [3, 2050]


@pytest.fixture(scope="module")
def f_problems():
    """(12, 4, 50), p = 8, batch 4096 (drawn on the GPU), with an indefinite Schur complement at problems 3 and
    2050 (status 7)."""
    dims = _dims(12, 4, 50, 8)
    arrays = [a.cpu().numpy() for a in fb.newton_kkt_batch(dims, F_BATCH, seed=_seed("f2f4"), device="cuda")]
    theta = arrays.pop()
    for q in F_BAD:
        theta[q] = rk.initialize_theta_model(dims, -50.0)
    return dims, arrays, theta


def test_f2_theta_step_full_batch(monkeypatch, f_problems):
    """f2: factor_theta + solve_theta on (12, 4, 50), p = 8, every one of the 4096 problems against the oracle."""
    dims, arrays, theta = f_problems
    model, w, r1, r2, r3, rhs = arrays

    def one(o, q):
        st = o.factor_theta(model[q], theta[q], w[q], r1[q], r2[q], r3[q])
        return st, (o.solve_theta(model[q], theta[q], rhs[q]) if st == 0 else None)

    refs = _pool(dims, one, range(F_BATCH))
    expect = np.array([r[0] for r in refs], dtype=np.int32)
    want = np.zeros(F_BATCH, dtype=np.int32)
    want[F_BAD] = 7
    np.testing.assert_array_equal(expect, want)
    ok = np.flatnonzero(expect == 0)
    ref = np.stack([refs[q][1] for q in ok])
    fb.assert_discriminates(ref, THETA_TOL, what="f2")
    kkt = _plan(dims, F_BATCH, monkeypatch=monkeypatch)
    assert TAG in kkt.kernel_name and "fused theta passes" in kkt.kernel_name, kkt.kernel_name
    d = _dev(model, theta, w, r1, r2, r3, rhs)
    kkt.factor_theta(*d[:6])
    np.testing.assert_array_equal(_status(kkt, "factor_theta"), expect)
    out = _guarded(F_BATCH, dims.full_dim)
    kkt.solve_theta(d[0], d[1], d[6], sol=out[:F_BATCH])
    got = _host(out, F_BATCH, "solve_theta")
    assert (got[F_BAD] == F_SENTINEL).all(), "a failed problem's solution was written"
    print(f"f2 {kkt.kernel_name} batch {F_BATCH}")
    _worst(_rel_rows(got[ok], ref), ok, "solve_theta vs oracle", THETA_TOL)


def test_f4_operator_full_batch(monkeypatch, f_problems):
    """f4: y += K x on (12, 4, 50) at batch 4096, without and with theta (p = 8), every problem against the oracle
    (accumulating onto a nonzero y0)."""
    dims, arrays, theta = f_problems
    model, w, r1, r2, r3, _ = arrays
    plain = _dims(12, 4, 50)
    r1s = np.ascontiguousarray(r1[:, :plain.x_dim])
    rng = np.random.default_rng(_seed("f4"))
    x, y0 = rng.standard_normal((2, F_BATCH, plain.kkt_dim))
    xt = rng.standard_normal((F_BATCH, dims.full_dim))
    refs = _pool(dims, lambda o, q: o.add_Kx_to_y_theta(model[q], theta[q], w[q], r1[q], r2[q], r3[q], xt[q]),
                 range(F_BATCH))
    ref_t = np.stack(refs)
    ref = np.stack(_pool(plain, lambda o, q: o.add_Kx_to_y(model[q], w[q], r1s[q], r2[q], r3[q], x[q], y=y0[q]),
                         range(F_BATCH)))
    fb.assert_discriminates(ref, REL, what="f4")
    fb.assert_discriminates(ref_t, REL, what="f4 theta")
    kkt = _plan(plain, F_BATCH, monkeypatch=monkeypatch)
    assert TAG in kkt.kernel_name, kkt.kernel_name
    d = _dev(model, w, r1s, r2, r3)
    y = _guarded(F_BATCH, plain.kkt_dim, y0)
    kkt.add_Kx_to_y(*d, _dev(x)[0], y=y[:F_BATCH])
    print(f"f4 {kkt.kernel_name} batch {F_BATCH}")
    _worst(_op_rows(_host(y, F_BATCH, "add_Kx_to_y"), ref), range(F_BATCH), "add_Kx_to_y vs oracle", REL)
    del kkt, d, y
    kkt = _plan(dims, F_BATCH, monkeypatch=monkeypatch)
    d = _dev(model, theta, w, r1, r2, r3)
    y = _guarded(F_BATCH, dims.full_dim, np.zeros((F_BATCH, dims.full_dim)))
    kkt.add_Kx_to_y_theta(*d, _dev(xt)[0], y=y[:F_BATCH])
    _worst(_op_rows(_host(y, F_BATCH, "add_Kx_to_y_theta"), ref_t), range(F_BATCH), "add_Kx_to_y_theta vs oracle",
           REL)

"""sip_lqr_tree_residual_multi and sip_lqr_tree_refine_multi on the GPU (BatchedTreeLQR.residual_multi / .refine_multi;
csrc/tree_residual.hpp).

Residual: every column against the formulas in np.longdouble (tree_refine_cases.residual), every entry held to the
derived bound |got - ref| <= k 2^-53 a and every norm to the largest bound of its problem and column, as
tests/test_gpu_tree_refine.py holds the single-column kernel; and every column bit for bit what sip_lqr_tree_residual
computes on it.  The cases are those of that file, built here the same way, and the reference's shallow wide tree (a
root of 63 children).  The outputs live in framed buffers one column longer than the call is told: the frames and the
extra column stay the sentinel, so a masked column of a short group stores nothing.

Refinement: the cells of hard_inputs.TREES x AXES_TREE on the fused size-class kernels and on the general engine, the
cell's hard_inputs.TREE_COLS right-hand-side columns, two rounds from zero; every column held to the project's criterion
e <= 1e-9 + 3 e_ref against its extended-precision solve (form and constants of tests/test_gpu_tree_refine.py; e_ref
the oracle's error on that column).  Where tree_refine_cases.cells_with_a_drop() names the cell, the worst error over
the columns falls 10x from round 1 to round 2.

Every refinement test prints "REFINE_MULTI | family | axis | worst e over columns by round | worst e_ref | worst norms
by round"; DESIGN 7.1 holds the table of one run."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import chain_guards as cg
import extended_reference as xr
import full_batch_problems as fb
import hard_inputs as hi
import tree_refine_cases as tc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

INVALID = -1
COUNTS = (1, 2, 3, 5, 8, 9)          # 9: a group of 8 and a group of 1


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _plan(topo, batch, general=False):
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    with _env(**({"SIP_LQR_TREE": "general"} if general else {})):
        s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    maps = fb.PlanMaps(s, topo)
    # the oracle's sol layout is the plan's output (and right-hand-side) layout
    assert np.array_equal(maps.sol_idx, np.arange(topo.layout.sol_len)) and np.array_equal(maps.rhs_idx, maps.sol_idx)
    assert s.rhs_len == s.out_len == topo.layout.sol_len
    return s, maps


def _load(s, maps, topo, blocks):
    nodes, edges = fb.to_oracle(topo, blocks)
    s.input.copy_(torch.from_numpy(maps.pack_input(s, nodes, edges)))


def _dev(a):
    a = np.asarray(a, dtype=np.float64)
    if a.shape[-1] == 0:                                      # an empty arena is one unused scalar wide
        a = np.zeros(a.shape[:-1] + (1,))
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


# ---- the cases: those of tests/test_gpu_tree_refine.py, built the same way ---------------------------------------------
def _tree(parents, children, sd, cd, seed):
    topo = fb.Topology(parents, children, sd, cd)
    return topo, tc.random_blocks(topo, 3, seed)


def _hard_tree(dims):
    rng = np.random.default_rng(hi._seed("tree", *dims))
    topo = fb.random_topology(rng, hi.TREE_NODES, *dims)
    assert sum(1 for n in topo.sd if n == 0) == 2 and max(np.bincount(topo.parents)) >= 2
    return topo, fb.make_blocks(topo, 3, rng, "random")


def _wide_and_deep():
    rng = np.random.default_rng(25)
    topo = fb.random_topology(rng, 300, 15, 3)
    topo = fb.Topology([0 if e < 160 else p for e, p in enumerate(topo.parents)], topo.children, topo.sd, topo.cd)
    assert (topo.N + topo.E) * max(topo.sd) * 8 > 64 * 1024 and 160 * 4 > topo.N + topo.E
    return topo, fb.make_blocks(topo, 3, rng, "random")


def _shallow_wide():
    """The reference's shallow wide benchmark tree at T = 63: the root's 63 children; max_n = 9."""
    topo = fb.variable_benchmark_topology(1)
    assert max(np.bincount(topo.parents)) == 63 and max(topo.sd) == 9
    return topo, fb.make_blocks(topo, 3, np.random.default_rng(27), "variable_benchmark")


def _name(staged, columns):
    return "tree_residual_cols<%s,%d>/f64" % ("staged" if staged else "direct", columns)


# name -> (builder of (topo, blocks), the multi-column residual kernel of a full group, the solve kernel's name starts
#          with, the column counts)
CASES = {name: (lambda p=prob: tc.batched(p, 3, seed=5), _name(True, 8), "tree_factor_solve_qw16", COUNTS)
         for name, prob in tc.reference_trees().items()}
CASES.update({
    "single_node": (lambda: _tree([], [], [5], [], 21), _name(True, 8), "tree_factor_solve_qw16", COUNTS),
    "random<9,3>": (lambda: _hard_tree((9, 3)), _name(True, 8), "tree_factor_solve_qw16<9,3>", COUNTS),
    "random<15,8>": (lambda: _hard_tree((15, 8)), _name(True, 8), "tree_factor_solve_qw16<15,8>", COUNTS),
    "edge_m0": (lambda: _tree([0, 1, 1], [1, 2, 3], [3, 2, 4, 3], [2, 0, 1], 22), _name(True, 8), "tree_", COUNTS),
    "general<17,9>": (lambda: _tree([0, 0, 1], [1, 2, 3], [5, 17, 3, 4], [9, 2, 3], 23), _name(True, 8), "tree_generic",
                      COUNTS),
    # the 91 x 91 block cannot be staged; its parts (3 items of 2 * 91 NC doubles) and two wavefronts fit at 2 columns
    "beyond_the_staging_budget": (lambda: _tree([0], [1], [91, 2], [1], 24), _name(False, 2), "tree_generic", COUNTS),
    # split over the wavefronts, its parts (25 items) fitting at 8 columns
    "star_of_12": (lambda: _tree([0] * 12, list(range(1, 13)), [6, 3, 4, 5] * 3 + [2], [2, 1, 3] * 4, 26), _name(True, 8),
                   "tree_factor_solve_qw16", COUNTS),
    # never split: the parts exceed LDS at one column.  Three columns keep the host reference short.
    "parts_beyond_lds": (lambda: _wide_and_deep(), _name(True, 8), "tree_factor_solve_qw16<15,", (3,)),
    # split, and its parts (127 items) fit at 2 columns only: four launches carry 8 columns, and 9 end on a launch of
    # one column (csrc/tree_residual_cols_shape.hpp prefers that to nodes in turn at 8 columns: DESIGN 4.10.3)
    "shallow_wide_63": (lambda: _shallow_wide(), _name(True, 2), "tree_factor_solve_qw16", (2, 3, 8, 9)),
})
_DRAWS = {}


class Draw:
    pass


def _draw(name, batch=3):
    """Per case, computed once and left unchanged: topo, blocks, max(counts) columns of right-hand sides and iterates,
    and per column the long-double residual (ref, mag) with q, c, r of the blocks (own) and with the column (rhs)."""
    if name not in _DRAWS:
        builder, _, _, counts = CASES[name] if isinstance(name, str) else (name, None, None, (8,))
        d = Draw()
        d.topo, d.blocks = builder()
        B, C = d.blocks["Q"][0].shape[0], max(counts)
        rng = np.random.default_rng(hi._seed("tree residual multi", name if isinstance(name, str) else "built"))
        d.sol = rng.normal(size=(C, B, d.topo.layout.sol_len))
        d.rhs = [fb.make_rhs(d.topo, B, rng) for _ in range(C)]
        d.own = [tc.residual(d.topo, d.blocks, None, d.sol[c]) for c in range(C)]
        d.other = [tc.residual(d.topo, d.blocks, d.rhs[c], d.sol[c]) for c in range(C)]
        d.sol.setflags(write=False)
        _DRAWS[name] = d
    return _DRAWS[name]


def _setup(name, general=False):
    d = _draw(name)
    B = d.blocks["Q"][0].shape[0]
    s, maps = _plan(d.topo, B, general)
    _load(s, maps, d.topo, d.blocks)
    out_cols = _dev(d.sol)
    rhs_cols = _dev(np.stack([maps.pack_rhs(s, r) for r in d.rhs]))
    return d, s, out_cols, rhs_cols


def _raw_multi(s, out_cols, rhs_cols, want_vector=True):
    """sip_lqr_tree_residual_multi, its outputs in framed buffers that are one column longer than num_rhs: the frames
    and that column must come back as the sentinel, and every other entry written."""
    C, B, L = out_cols.shape[0], s.batch, max(1, s.rhs_len)
    res_full, res = cg.framed((C + 1, B, L), torch.float64, "cuda:0")
    nrm_full, nrm = cg.framed((C + 1, B), torch.float64, "cuda:0")
    code = s._lib.sip_lqr_tree_residual_multi(
        s._plan, ctypes.c_void_p(s.input.data_ptr()), ctypes.c_void_p(rhs_cols.data_ptr() if rhs_cols is not None else None),
        ctypes.c_void_p(out_cols.data_ptr()), C, ctypes.c_void_p(res.data_ptr() if want_vector else None),
        ctypes.c_void_p(nrm.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0, code
    torch.cuda.synchronize()
    assert cg.frame_intact(res_full) and cg.frame_intact(nrm_full)
    res, nrm = res.cpu().numpy(), nrm.cpu().numpy()
    assert (res[C] == cg.F_SENTINEL).all() and (nrm[C] == cg.F_SENTINEL).all()       # nothing past the last column
    assert (nrm[:C] != cg.F_SENTINEL).all()
    written = res[:C, :, :s.rhs_len]
    assert ((written != cg.F_SENTINEL).all() if want_vector else (res == cg.F_SENTINEL).all())
    return written, nrm[:C]


def _check_residual(topo, got, norms, refs, what=""):
    """got [C, B, L], norms [C, B]; refs[c] = (ref, mag)."""
    worst = 0.0
    for c, (ref, mag) in enumerate(refs[:got.shape[0]]):
        bound = tc.bound(topo, mag)
        diff = np.abs(got[c].astype(tc.LD) - ref)
        worst = max(worst, float((diff / np.where(bound > 0, bound, 1)).max(initial=0.0)))
        assert (diff <= bound).all(), (what, c, worst)
        ref_norm = np.abs(ref).max(axis=1, initial=0.0)
        assert (np.abs(norms[c].astype(tc.LD) - ref_norm) <= bound.max(axis=1, initial=0.0)).all(), (what, c, norms[c])
    print(f"RESIDUAL_MULTI | {what} x {got.shape[0]} | worst |got - ref| / (k 2^-53 a) = {worst:.3f}")


def _check_names(s, name):
    _, kernel, solve_kernel, _ = CASES[name]
    got = s.residual_multi_kernel_name
    assert s.kernel_name.startswith(solve_kernel), s.kernel_name
    assert got == _name("staged" in got, s.residual_multi_columns) and 1 <= s.residual_multi_columns <= 8, got
    assert kernel is None or got == kernel, (got, kernel)


@pytest.mark.parametrize("with_rhs", [False, True], ids=["own_qcr", "rhs_columns"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_column_against_long_double(name, with_rhs):
    d, s, out_cols, rhs_cols = _setup(name)
    _check_names(s, name)
    for C in CASES[name][3]:
        cols = rhs_cols[:C] if with_rhs else None
        got, norms = _raw_multi(s, out_cols[:C], cols)
        _check_residual(d.topo, got, norms, d.other if with_rhs else d.own, name)
        _, norms_only = _raw_multi(s, out_cols[:C], cols, want_vector=False)        # d_res_cols = NULL: the same norms
        np.testing.assert_array_equal(norms_only, norms)
    assert not np.array_equal(d.own[0][0], d.other[0][0])      # a column is not the problem's own q, c, r


@pytest.mark.parametrize("with_rhs", [False, True], ids=["own_qcr", "rhs_columns"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_column_is_bit_for_bit_the_single_column_kernel(name, with_rhs):
    d, s, out_cols, rhs_cols = _setup(name)
    L, top = s.rhs_len, max(CASES[name][3])
    single = [s.residual(out_cols[c], rhs=rhs_cols[c] if with_rhs else None) for c in range(top)]
    torch.cuda.synchronize()
    single = [(r.cpu().numpy()[:, :L], n.cpu().numpy()) for r, n in single]
    for C in CASES[name][3]:
        cols = rhs_cols[:C] if with_rhs else None
        got, norms = _raw_multi(s, out_cols[:C], cols)
        for c in range(C):
            np.testing.assert_array_equal(got[c], single[c][0], err_msg=f"{name}: column {c} of {C}")
            np.testing.assert_array_equal(norms[c], single[c][1], err_msg=f"{name}: column {c} of {C}")
        again, norms_again = _raw_multi(s, out_cols[:C], cols)                       # two launches: the same bits
        np.testing.assert_array_equal(again, got)
        np.testing.assert_array_equal(norms_again, norms)
        res, nrm = s.residual_multi(out_cols[:C].contiguous(), None if cols is None else cols.contiguous())
        _, nrm_only = s.residual_multi(out_cols[:C].contiguous(), None if cols is None else cols.contiguous(),
                                       want_vector=False)                            # the same norms
        torch.cuda.synchronize()
        np.testing.assert_array_equal(res.cpu().numpy()[:, :, :L], got)
        np.testing.assert_array_equal(nrm.cpu().numpy(), norms)
        np.testing.assert_array_equal(nrm_only.cpu().numpy(), norms)


@pytest.mark.parametrize("name", ["random<9,3>", "star_of_12", "shallow_wide_63"])
def test_an_input_that_is_not_16_byte_aligned_is_read_in_place(name):
    d, s, out_cols, rhs_cols = _setup(name)
    C = max(CASES[name][3])
    aligned, norms_aligned = _raw_multi(s, out_cols[:C], rhs_cols[:C])
    room = torch.zeros(s.input.numel() + 2, dtype=torch.float64, device="cuda:0")
    assert room.data_ptr() % 16 == 0
    off = room[1:1 + s.input.numel()].view(s.batch, -1)
    off.copy_(s.input)
    assert off.data_ptr() % 16 == 8 and off.is_contiguous()
    s.input = off
    got, norms = _raw_multi(s, out_cols[:C], rhs_cols[:C])
    _check_residual(d.topo, got, norms, d.other, name + " misaligned")
    np.testing.assert_array_equal(got, aligned)
    np.testing.assert_array_equal(norms, norms_aligned)
    for c in (0, C - 1):                                      # and the single-column kernel on the same misaligned input
        one, norm = s.residual(out_cols[c], rhs=rhs_cols[c])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got[c], one.cpu().numpy()[:, :s.rhs_len])
        np.testing.assert_array_equal(norms[c], norm.cpu().numpy())


def test_every_problem_and_column_of_a_batch_beyond_the_cus():
    """300 distinct problems, more workgroups than compute units, 8 columns: every problem's norms and vectors."""
    build = lambda: tc.batched(tc.reference_trees()["five_node"], 300, seed=9)
    d = _draw(build)
    assert np.abs(np.diff(d.own[0][0].astype(np.float64), axis=0)).max(axis=1).min() > 1e-3   # neighbours differ
    s, maps = _plan(d.topo, 300)
    assert s.residual_multi_kernel_name == _name(True, 8)
    _load(s, maps, d.topo, d.blocks)
    got, norms = _raw_multi(s, _dev(d.sol), None)
    _check_residual(d.topo, got, norms, d.own, "five_node x 300")
    got, norms = _raw_multi(s, _dev(d.sol), _dev(np.stack([maps.pack_rhs(s, r) for r in d.rhs])))
    _check_residual(d.topo, got, norms, d.other, "five_node x 300, rhs columns")


def test_the_checks_of_the_python_methods():
    d, s, out_cols, rhs_cols = _setup("random<9,3>")
    ok = out_cols[:2].contiguous()
    for bad in (ok[:, :, :-1], ok[:, :2], ok.float(), ok.cpu(), ok.transpose(0, 1), ok[0]):
        with pytest.raises(ValueError):
            s.residual_multi(bad)
        with pytest.raises(ValueError):
            s.residual_multi(ok, rhs_cols=bad)
        with pytest.raises(ValueError):
            s.refine_multi(bad)
    with pytest.raises(ValueError):
        s.residual_multi(ok, rhs_cols=rhs_cols[:3].contiguous())
    with pytest.raises(ValueError):
        s.refine_multi(rhs_cols[:3].contiguous(), out_cols=ok)


# ---- the scaled form ---------------------------------------------------------------------------------------------------
def _up(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("name", ["random<9,3>", "star_of_12"])
def test_scaled_residual_has_one_power_of_two_per_problem_and_column(name):
    """One round of refine_multi from given iterates leaves rho / s and s in the refine scratch: [rho / s | d | s | the
    solve's scratch], the first two [num_rhs][batch][rhs_len], s [num_rhs][batch], each region a multiple of 256 bytes
    (include/sip_lqr_amd.h).  The columns differ in magnitude by 2^+-20: a scale shared by the columns of a problem
    would put some column's rho / s outside [1, 2)."""
    d, s, out_cols, rhs_cols = _setup(name)
    C, B, L = 9, 3, s.rhs_len
    f = 2.0 ** (20 * (np.arange(C) % 3 - 1))                   # exact: rho and its bound scale with it
    fd = _dev(f)[:, None, None]
    out_cols, rhs_cols = (out_cols[:C] * fd).contiguous(), (rhs_cols[:C] * fd).contiguous()
    s.factor_fused()
    plain, plain_norms = s.residual_multi(out_cols, rhs_cols)
    _, norms = s.refine_multi(rhs_cols, iterations=1, out_cols=out_cols.clone())
    torch.cuda.synchronize()
    region = _up(C * B * L * 8)
    raw = s._refine_multi_scratch.cpu().numpy()
    assert raw.size >= 2 * region + C * B * 8
    scaled = raw[:C * B * L * 8].view(np.float64).reshape(C, B, L)
    scale = raw[2 * region:2 * region + C * B * 8].view(np.float64).reshape(C, B)
    norm = norms[0].cpu().numpy()
    assert norm.shape == (C, B)
    np.testing.assert_array_equal(norm, plain_norms.cpu().numpy())
    np.testing.assert_array_equal(scale, tc.scale_of(norm))           # exactly the power of two below the norm
    assert ((scale <= norm) & (norm < 2 * scale)).all() and (np.log2(scale) % 1 == 0).all()
    assert len({float(v) for v in scale[:, 0]}) >= 3                   # the columns of a problem do not share one
    np.testing.assert_array_equal(scaled * scale[:, :, None], plain.cpu().numpy()[:, :, :L])   # rho / s is exact
    for c in range(C):
        ref, mag = d.other[c]
        fc = tc.LD(f[c])
        assert (np.abs((scaled[c] * scale[c][:, None]).astype(tc.LD) - ref * fc) <= tc.bound(d.topo, mag * fc)).all(), c
    assert np.abs(scaled).max() < 2.0 and (np.abs(scaled).max(axis=2) >= 1.0).all()


# ---- refinement --------------------------------------------------------------------------------------------------------
FAMILIES = {"tree fused size class": (False, "tree_solve_mrhs_qw16"), "tree general engine": (True, "tree_generic")}


def _factor(s, general):
    return s.factor() if general else s.factor_fused()


def _load_cell(cell, general=False, blocks=None):
    s, maps = _plan(cell.topo, hi.BATCH, general)
    if blocks is None:
        s.input.copy_(torch.from_numpy(maps.pack_input(s, cell.nodes, cell.edges)))
    else:
        _load(s, maps, cell.topo, blocks)
    return s, maps


def _columns(s, maps, cell):
    assert cell.ncols == hi.TREE_COLS == len(cell.columns)
    return _dev(np.stack([maps.pack_rhs(s, col) for col in cell.columns]))


def _col_errs(cell, sol_cols):
    return np.array([xr.err(sol_cols[c], cell.col_ext[c]) for c in range(cell.ncols)])


@pytest.mark.parametrize("axis", hi.AXES_TREE)
@pytest.mark.parametrize("dims", hi.TREES, ids=lambda d: "<%d,%d>" % d)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_refine_multi_tree(family, dims, axis):
    general, tag = FAMILIES[family]
    it = tc.ITERATIONS_F64
    assert it == 2
    cell = hi.tree_cell(*dims, axis)
    topo, L = cell.topo, cell.topo.layout.sol_len
    s, maps = _load_cell(cell, general)
    assert s.multi_kernel_name.startswith(tag), s.multi_kernel_name
    status = _factor(s, general)
    rhs_cols = _columns(s, maps, cell)
    sol, norms = s.refine_multi(rhs_cols, iterations=it)
    first, _ = s.refine_multi(rhs_cols, iterations=1)          # round 1 alone, for the errors by round
    plain = s.solve_multi(rhs_cols)
    torch.cuda.synchronize()
    sol, norms, first, plain = (t.cpu().numpy() for t in (sol, norms, first, plain))
    sol, first, plain = sol[:, :, :L], first[:, :, :L], plain[:, :, :L]
    e1, e2 = _col_errs(cell, first), _col_errs(cell, sol)
    e_ref = np.array([xr.err(cell.col_ref[c], cell.col_ext[c]) for c in range(cell.ncols)])
    name = "%s <%d,%d>" % ((family,) + dims)
    print(f"REFINE_MULTI | {name} | {axis} | {e1.max():.1e} {e2.max():.1e} | {e_ref.max():.1e} | " +
          " ".join(f"{v:.1e}" for v in norms.max(axis=(1, 2))))
    np.testing.assert_array_equal(status.cpu().numpy(), cell.ref_status)
    assert (e2 <= tc.CAP + 3 * e_ref).all(), (name, axis, e1, e2, e_ref)
    assert norms.shape == (it + 1, cell.ncols, hi.BATCH), norms.shape
    for c in range(cell.ncols):                                # the last row: the residual of the returned iterate
        ref, mag = tc.residual(topo, cell.blocks, cell.columns[c], sol[c])
        slack = tc.bound(topo, mag).max(axis=1)
        assert (np.abs(norms[-1, c].astype(tc.LD) - np.abs(ref).max(axis=1)) <= slack).all(), (c, norms[-1, c])
    np.testing.assert_array_equal(first, plain)                # round 1 from zero is the plan's solve_multi
    if (dims, axis) in tc.cells_with_a_drop():
        assert e2.max() * 10 <= e1.max(), (name, axis, e1, e2)


def test_rounds_one_by_one_are_the_rounds_of_one_call():
    """from_zero = 0 continues from the iterates it is given: two calls of one round are one call of two."""
    cell = hi.tree_cell(*hi.TREES[0], "cost[1,1e4]")
    s, maps = _load_cell(cell)
    s.factor_fused()
    rhs_cols = _columns(s, maps, cell)
    both, norms = s.refine_multi(rhs_cols, iterations=2)
    one, n1 = s.refine_multi(rhs_cols, iterations=1)
    kept = one.clone()
    two, n2 = s.refine_multi(rhs_cols, iterations=1, out_cols=one)
    torch.cuda.synchronize()
    assert two.data_ptr() == one.data_ptr()                    # refined in place
    np.testing.assert_array_equal(two.cpu().numpy(), both.cpu().numpy())
    np.testing.assert_array_equal(n1.cpu().numpy(), norms.cpu().numpy()[:2])
    np.testing.assert_array_equal(n2.cpu().numpy(), norms.cpu().numpy()[1:])
    assert not np.array_equal(kept.cpu().numpy(), two.cpu().numpy())


def test_a_failed_problem_keeps_its_iterate_in_every_column():
    from sip_optimal_control_amd import FactorStatus
    cell = hi.tree_cell(*hi.TREES[0], hi.BENIGN)
    blocks = {k: [a.copy() for a in v] for k, v in cell.blocks.items()}
    node = next(i for i, n in enumerate(cell.topo.sd) if n >= 3 and i > 0)
    blocks["delta"][node][1, 2] = -1.0
    s, maps = _load_cell(cell, blocks=blocks)
    status = s.factor_fused()
    rhs_cols = _columns(s, maps, cell)
    L = cell.topo.layout.sol_len
    start = np.random.default_rng(5).normal(size=(cell.ncols, hi.BATCH, L))
    sol, norms = s.refine_multi(rhs_cols, iterations=tc.ITERATIONS_F64 + 1, out_cols=_dev(start))
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, int(FactorStatus.INVALID_DELTA), 0]
    sol = sol.cpu().numpy()[:, :, :L]
    np.testing.assert_array_equal(sol[:, 1], start[:, 1])      # exactly what went in, in all columns
    good = [0, 2]
    for c in range(cell.ncols):
        e = xr.err(sol[c][good], cell.col_ext[c][good])
        e_ref = xr.err(cell.col_ref[c][good], cell.col_ext[c][good])
        assert e <= tc.CAP + 3 * e_ref, (c, e, e_ref)
        assert not np.array_equal(sol[c][good], start[c][good])


# ---- the C ABI on valid plans ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,general,batch", [("random<9,3>", False, 3), ("random<9,3>", False, 4096),
                                                ("general<17,9>", False, 5), ("random<15,8>", True, 7),
                                                ("single_node", False, 3)])
def test_refine_multi_workspace_bytes_is_what_the_header_documents(name, general, batch):
    topo = CASES[name][0]()[0]
    s, _ = _plan(topo, batch, general)
    lib = s._lib
    assert s.multi_kernel_name.startswith("tree_generic") == (general or name.startswith("general"))
    for num_rhs in (1, 3, 9):
        multi = int(lib.sip_lqr_tree_solve_multi_scratch_bytes(s._plan, num_rhs))
        want = 2 * _up(num_rhs * batch * s.rhs_len * 8) + _up(num_rhs * batch * 8) + _up(multi)
        assert int(lib.sip_lqr_tree_refine_multi_workspace_bytes(s._plan, num_rhs)) == want, num_rhs
    assert int(lib.sip_lqr_tree_refine_multi_workspace_bytes(s._plan, 0)) == 0
    assert int(lib.sip_lqr_tree_refine_multi_workspace_bytes(s._plan, -1)) == 0
    assert int(lib.sip_lqr_tree_residual_multi_columns(s._plan)) == s.residual_multi_columns >= 1


def test_every_misuse_on_a_valid_plan_is_an_invalid_argument():
    d, s, out_cols, rhs_cols = _setup("random<9,3>")
    s.factor_fused()
    C = 3
    out_cols, rhs_cols = out_cols[:C].contiguous(), rhs_cols[:C].contiguous()
    s.refine_multi(rhs_cols, iterations=1)                                   # sizes the scratch
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    norm = torch.zeros(33 * C * 3, dtype=torch.float64, device="cuda:0")
    res_args = dict(plan=s._plan, input=P(s.input), rhs=None, out=P(out_cols), num_rhs=C, res=None, norms=P(norm),
                    stream=None)
    ref_args = dict(plan=s._plan, input=P(s.input), work=P(s.work), rhs=P(rhs_cols), out=P(out_cols), num_rhs=C,
                    iterations=2, from_zero=0, status=P(s.status), rws=P(s._refine_multi_scratch), norms=P(norm),
                    stream=None)
    res = lambda **kw: s._lib.sip_lqr_tree_residual_multi(*{**res_args, **kw}.values())
    ref = lambda **kw: s._lib.sip_lqr_tree_refine_multi(*{**ref_args, **kw}.values())
    misuse = {"residual plan": res(plan=None), "residual input": res(input=None), "residual out": res(out=None),
              "residual norms": res(norms=None), "residual num_rhs=-1": res(num_rhs=-1),
              "refine plan": ref(plan=None), "refine input": ref(input=None), "refine work": ref(work=None),
              "refine out": ref(out=None), "refine status": ref(status=None), "refine rws": ref(rws=None),
              "refine norms": ref(norms=None), "refine num_rhs=-1": ref(num_rhs=-1), "iterations=0": ref(iterations=0),
              "iterations=33": ref(iterations=33), "iterations=-1": ref(iterations=-1), "from_zero=2": ref(from_zero=2),
              "from_zero=-1": ref(from_zero=-1)}
    for what, rc in misuse.items():
        assert rc == INVALID, (what, rc)
    # the well-formed calls run; no column: nothing is launched, whatever the column pointers are
    assert res() == 0 and ref() == 0 and ref(iterations=32) == 0
    assert res(num_rhs=0, out=None) == 0 and ref(num_rhs=0, out=None, rhs=None) == 0
    torch.cuda.synchronize()

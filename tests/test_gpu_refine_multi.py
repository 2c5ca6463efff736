"""sip_lqr_residual_multi and sip_lqr_refine_multi on the GPU (BatchedChainLQR.residual_multi / .refine_multi;
csrc/chain_residual.hpp).

Residual: every column against the formulas in np.longdouble (refine_cases.residual), every entry held to the derived
bound (2 n + m + 3) 2^-53 a and every norm to the largest of those bounds, as tests/test_gpu_refine.py holds the
single-column kernel; and every column bit for bit what sip_lqr_residual computes on it.  The outputs live in framed
buffers one column longer than the call is told: the frames and the extra column stay the sentinel.

Refinement: the families and axes of tests/test_gpu_refine.py; the columns of a cell are f_c * cell.vecs with
f_c = (-1)^c 2^(e_c), e_c spread over [-20, 20] (a power of two: the extended solution of column c is exactly
f_c * cell.ext), the last ones replaced by the cell's own columns where it has some.  Each column is held to the
project's criterion e <= 1e-9 + 3 e_ref after the number of rounds tests/test_gpu_refine.py uses.

Every refinement test prints "REFINE_MULTI | family | axis | worst e over columns | e_ref | worst norms by round";
DESIGN 7.1 holds the table of one run."""
import ctypes

import numpy as np
import pytest

import chain_guards as cg
import extended_reference as xr
import hard_inputs as hi
import refine_cases as rc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, F64 = "f32", "f64"
TORCH = {F32: torch.float32, F64: torch.float64}
NP = {F32: np.float32, F64: np.float64}


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0", dtype=dtype)      # a copy: the draws are read-only


def _solver(n, m, T, batch, dtype=F64, **kwargs):
    from sip_optimal_control_amd import BatchedChainLQR
    return BatchedChainLQR(n, m, T, batch, dtype=TORCH[dtype], **kwargs)


def _pack(s, mats):
    """FULL-layout device mats -> the plan's layout."""
    if not s.shape.symmetric:
        return mats
    return mats[:, torch.from_numpy(s.shape.pack_index()).to("cuda:0")].contiguous()


def _ids(v):
    return str(v) if not isinstance(v, dict) else "+".join(v) or "plain"


# ---- residual ------------------------------------------------------------------------------------------------------
_DRAWS = {}


def _draw(n, m, T, batch, dtype, wide, num_rhs):
    """Random inputs (float64 numpy, FULL layout) as the plan sees them: mats rounded to the plan's dtype, the columns
    of vecs and sol too unless wide; Q and R exactly symmetric; column c drawn from its own seed.  With the long-double
    residual of every column, computed once per case.  -> mats, vecs [C, B, len], sol, ref, mag."""
    key = (n, m, T, batch, dtype, wide, num_rhs)
    if key not in _DRAWS:
        from sip_optimal_control_amd import ChainShape, synthetic
        mats, vecs0 = synthetic.make_chain_batch(ChainShape(n, m, T), batch, seed=100 + n + 7 * m, cross_term=0.05)
        mats, vecs0 = mats.numpy().copy(), vecs0.numpy().copy()
        views = hi.chain_views(n, m, T, mats)
        for blk in views["Q"] + views["R"]:
            low = np.tril(blk)
            blk[...] = low + np.tril(blk, -1).transpose(0, 2, 1)
        if dtype == F32:
            mats = mats.astype(np.float32).astype(np.float64)
        vecs, sol = [], []
        for c in range(num_rhs):
            rng = np.random.default_rng([n, m, T, c])
            vecs.append(rng.normal(size=vecs0.shape) * np.abs(vecs0).max())
            sol.append(rng.normal(size=vecs0.shape))
        vecs, sol = np.stack(vecs), np.stack(sol)
        if dtype == F32 and not wide:
            vecs, sol = (a.astype(np.float32).astype(np.float64) for a in (vecs, sol))
        both = [rc.residual(n, m, T, mats, vecs[c], sol[c]) for c in range(num_rhs)]
        ref, mag = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
        for a in (mats, vecs, sol, ref, mag):
            a.setflags(write=False)
        _DRAWS[key] = (mats, vecs, sol, ref, mag)
    return _DRAWS[key]


def _check_residual(n, m, got, norms, ref, mag):
    """got, ref, mag [C, B, len]; norms [C, B]."""
    bound = rc.bound_factor(n, m) * mag
    diff = np.abs(got.astype(rc.LD) - ref)
    worst = float((diff / np.where(mag > 0, mag, 1)).max() / 2.0 ** -53)
    print(f"RESIDUAL_MULTI | ({n},{m}) x {got.shape[0]} | worst |got - ref| / (2^-53 a) = {worst:.2f} of {2 * n + m + 3}")
    assert (diff <= bound).all(), worst
    ref_norm = np.abs(ref).max(axis=2)
    assert (np.abs(norms.astype(rc.LD) - ref_norm) <= bound.max(axis=2)).all(), (norms, ref_norm)


def _raw_multi(s, mats, vecs, sol, wide, want_vector=True):
    """sip_lqr_residual_multi with `wide` as given, its outputs in framed buffers that are one column longer than
    num_rhs: the frames and that column must come back as the sentinel, and every other entry written."""
    C, B, L = vecs.shape[0], s.batch, s.shape.vecs_len
    res_full, res = cg.framed((C + 1, B, L), torch.float64, "cuda:0")
    nrm_full, nrm = cg.framed((C + 1, B), torch.float64, "cuda:0")
    code = s._lib.sip_lqr_residual_multi(
        s._plan, ctypes.c_void_p(mats.data_ptr()), ctypes.c_void_p(vecs.data_ptr()), ctypes.c_void_p(sol.data_ptr()),
        C, wide, ctypes.c_void_p(res.data_ptr() if want_vector else None), ctypes.c_void_p(nrm.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0, code
    torch.cuda.synchronize()
    assert cg.frame_intact(res_full) and cg.frame_intact(nrm_full)
    res, nrm = res.cpu().numpy(), nrm.cpu().numpy()
    assert (res[C] == cg.F_SENTINEL).all() and (nrm[C] == cg.F_SENTINEL).all()       # nothing past the last column
    assert (nrm[:C] != cg.F_SENTINEL).all()
    assert ((res[:C] != cg.F_SENTINEL).all() if want_vector else (res == cg.F_SENTINEL).all())
    return res[:C], nrm[:C]


def _raw_single(s, mats, vecs, sol, wide):
    res = torch.full((s.batch, s.shape.vecs_len), float("nan"), dtype=torch.float64, device="cuda:0")
    norm = torch.full((s.batch,), float("nan"), dtype=torch.float64, device="cuda:0")
    code = s._lib.sip_lqr_residual(s._plan, ctypes.c_void_p(mats.data_ptr()), ctypes.c_void_p(vecs.data_ptr()),
                                   ctypes.c_void_p(sol.data_ptr()), wide, ctypes.c_void_p(res.data_ptr()),
                                   ctypes.c_void_p(norm.data_ptr()),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0, code
    torch.cuda.synchronize()
    return res.cpu().numpy(), norm.cpu().numpy()


# (n, m, T or None = horizon(n), batch, dtype, wide, constructor arguments, num_rhs or None = columns of a launch + 1)
RESIDUAL_CASES = [(n, m, None, 3, F64, 0, {}, None) for n, m in ((5, 3), (12, 4), (16, 4), (32, 8), (17, 9), (35, 3))]
RESIDUAL_CASES += [(1, 1, 1, 3, F64, 0, {}, None), (8, 4, None, 3, F64, 0, {"symmetric": True}, None),
                   (12, 4, 2, 5, F64, 0, {}, None), (5, 3, 2, 5, F64, 0, {}, None),
                   (12, 4, None, 3, F64, 0, {}, 1), (12, 4, None, 3, F64, 0, {}, 3)]
RESIDUAL_CASES += [(n, m, None, 3, F32, wide, {}, None) for n, m in ((5, 3), (12, 4), (32, 8)) for wide in (0, 1)]


def _residual_case(n, m, T, batch, dtype, wide, kwargs, num_rhs):
    T = hi.horizon(n) if T is None else T
    s = _solver(n, m, T, batch, dtype, **kwargs)
    assert s.shape.symmetric == bool(kwargs.get("symmetric"))
    columns = s.residual_multi_columns
    assert 1 <= columns <= 8
    num_rhs = columns + 1 if num_rhs is None else num_rhs     # a full group and a tail of one
    draw = _draw(n, m, T, batch, dtype, bool(wide), num_rhs)
    vt = torch.float64 if wide else TORCH[dtype]
    dm, dv, ds = _pack(s, _dev(draw[0], TORCH[dtype])), _dev(draw[1], vt), _dev(draw[2], vt)
    assert np.array_equal(cg.host(dv), draw[1]) and np.array_equal(cg.host(ds), draw[2])   # what the plan sees
    return s, (dm, dv, ds), draw


@pytest.mark.parametrize("n,m,T,batch,dtype,wide,kwargs,num_rhs", RESIDUAL_CASES, ids=_ids)
def test_every_column_against_long_double(n, m, T, batch, dtype, wide, kwargs, num_rhs):
    s, (dm, dv, ds), (_, _, _, ref, mag) = _residual_case(n, m, T, batch, dtype, wide, kwargs, num_rhs)
    got, norms = _raw_multi(s, dm, dv, ds, wide)
    _check_residual(n, m, got, norms, ref, mag)
    _, norms_only = _raw_multi(s, dm, dv, ds, wide, want_vector=False)             # d_res_cols = NULL: the same norms
    np.testing.assert_array_equal(norms_only, norms)
    res2, norms2 = s.residual_multi(dm, dv, ds)                                     # the method infers `wide`
    torch.cuda.synchronize()
    np.testing.assert_array_equal(res2.cpu().numpy(), got)
    np.testing.assert_array_equal(norms2.cpu().numpy(), norms)
    _, norms3 = s.residual_multi(dm, dv, ds, want_vector=False)
    np.testing.assert_array_equal(norms3.cpu().numpy(), norms)


@pytest.mark.parametrize("n,m,T,batch,dtype,wide,kwargs,num_rhs", RESIDUAL_CASES, ids=_ids)
def test_every_column_is_bit_for_bit_the_single_column_kernel(n, m, T, batch, dtype, wide, kwargs, num_rhs):
    s, (dm, dv, ds), _ = _residual_case(n, m, T, batch, dtype, wide, kwargs, num_rhs)
    got, norms = _raw_multi(s, dm, dv, ds, wide)
    for c in range(dv.shape[0]):
        one, norm = _raw_single(s, dm, dv[c], ds[c], wide)
        np.testing.assert_array_equal(got[c], one, err_msg=f"column {c}")
        np.testing.assert_array_equal(norms[c], norm, err_msg=f"column {c}")


def test_mats_that_is_not_16_byte_aligned_is_read_in_place():
    n, m, T, batch = 12, 4, hi.horizon(12), 3
    s, (dm, dv, ds), (_, _, _, ref, mag) = _residual_case(n, m, T, batch, F64, 0, {}, None)
    room = torch.zeros(dm.numel() + 2, dtype=torch.float64, device="cuda:0")
    assert room.data_ptr() % 16 == 0
    off = room[1:1 + dm.numel()].view(batch, -1)
    off.copy_(dm)
    assert off.data_ptr() % 16 == 8 and off.is_contiguous()
    got, norms = _raw_multi(s, off, dv, ds, 0)
    _check_residual(n, m, got, norms, ref, mag)
    aligned, norms_aligned = _raw_multi(s, dm, dv, ds, 0)
    np.testing.assert_array_equal(got, aligned)
    np.testing.assert_array_equal(norms, norms_aligned)
    for c in (0, dv.shape[0] - 1):                       # and the single-column kernel on the same misaligned mats
        one, norm = _raw_single(s, off, dv[c], ds[c], 0)
        np.testing.assert_array_equal(got[c], one)
        np.testing.assert_array_equal(norms[c], norm)


def test_the_checks_of_the_python_methods():
    s = _solver(5, 3, 4, 3, F32)
    L = s.shape.vecs_len
    mats = torch.zeros(3, s.shape.mats_len, dtype=torch.float32, device="cuda:0")
    gains = s.empty_gains()
    ok = torch.zeros(2, 3, L, dtype=torch.float64, device="cuda:0")
    for bad in (ok[:, :, :-1], ok[:, :2], ok.to(torch.float16), ok.cpu(), ok.transpose(0, 1), ok[0]):
        with pytest.raises(ValueError):
            s.residual_multi(mats, bad, ok)
        with pytest.raises(ValueError):
            s.refine_multi(mats, bad, gains)
    with pytest.raises(ValueError):
        s.residual_multi(mats, ok, ok.float())                      # both in the plan's dtype or both float64
    with pytest.raises(ValueError):
        s.residual_multi(mats, ok, ok[:1])
    with pytest.raises(ValueError):
        s.refine_multi(mats, ok.float(), gains)                     # float64 only
    with pytest.raises(ValueError):
        s.refine_multi(mats, ok, gains, sol_cols=ok[:1])


# ---- the scaled form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,dtype,kwargs", [(12, 4, F64, {}), (5, 3, F32, {}), (32, 8, F32, {}),
                                              (8, 4, F64, {"symmetric": True})], ids=_ids)
def test_scaled_residual_has_one_power_of_two_per_problem_and_column(n, m, dtype, kwargs):
    """One round of refine_multi from given iterates leaves rho / s (the plan's dtype) and s in the refine scratch:
    [rho / s | d | s], the first two [num_rhs][batch][vecs_len], s [num_rhs][batch], each region a multiple of 256
    bytes (include/sip_lqr_amd.h).  The columns differ in magnitude by 2^+-20: a scale shared by the columns of a
    problem would put some column's rho / s outside [1, 2)."""
    T, B = hi.horizon(n), 3
    s = _solver(n, m, T, B, dtype, **kwargs)
    C = s.residual_multi_columns + 1
    mats, vecs, sol, ref, mag = _draw(n, m, T, B, dtype, True, C)
    f = (2.0 ** (20 * (np.arange(C) % 3 - 1)))[:, None, None]           # exact: rho and its bound scale with it
    vecs, sol, ref, mag = vecs * f, sol * f, ref * f.astype(rc.LD), mag * f.astype(rc.LD)
    dm = _pack(s, _dev(mats, TORCH[dtype]))
    gains, _ = s.factor(dm)
    _, norms = s.refine_multi(dm, _dev(vecs), gains, iterations=1, sol_cols=_dev(sol))
    torch.cuda.synchronize()
    L, esize = s.shape.vecs_len, 4 if dtype == F32 else 8
    region = (C * B * L * esize + 255) // 256 * 256
    raw = s._refine_multi_ws.cpu().numpy()
    assert raw.size >= 2 * region + C * B * 8
    scaled = raw[:C * B * L * esize].view(NP[dtype]).reshape(C, B, L).astype(np.float64)
    scale = raw[2 * region:2 * region + C * B * 8].view(np.float64).reshape(C, B)
    norm = norms[0].cpu().numpy()
    assert norm.shape == (C, B)
    np.testing.assert_array_equal(scale, rc.scale_of(norm))             # exactly the power of two below the norm
    assert ((scale <= norm) & (norm < 2 * scale)).all() and (np.log2(scale) % 1 == 0).all()
    assert len({float(v) for v in scale[:, 0]}) >= 3                   # the columns of a problem do not share one
    bound = rc.bound_factor(n, m) * mag + (2.0 ** -24 * np.abs(ref) if dtype == F32 else 0)
    assert (np.abs((scaled * scale[:, :, None]).astype(rc.LD) - ref) <= bound).all()
    assert np.abs(scaled).max() < 2.0 and (np.abs(scaled).max(axis=2) >= 1.0 - 2.0 ** -20).all()


# ---- refinement ----------------------------------------------------------------------------------------------------
GENERAL = "tree_generic(chain layout)"
QF32_SEP, MT16_SEP = " + chain_factor_qf32 + chain_solve_qf32", " + chain_factor_mt16 + chain_solve_mt16"
# family -> (n, m, constructor arguments, what the kernel name holds, what it must not hold), as tests/test_gpu_refine.py
REFINE_F32 = {
    "qf32 separate sweeps (12,4)": (12, 4, {"fused_f32": True, "separate_sweeps": True}, ("qf32<12,4,", QF32_SEP), ()),
    "qf32 separate sweeps (5,3)": (5, 3, {"fused_f32": True, "separate_sweeps": True}, ("qf32<5,3,", QF32_SEP), ()),
    "mt16/f32 separate sweeps (32,8)": (32, 8, {"separate_sweeps": True}, ("mt16<32,8,", MT16_SEP), ()),
    "general engine /f32 (12,4)": (12, 4, {}, (GENERAL,), ()),
}
REFINE_F64 = {
    "qw16 staged (12,4)": (12, 4, {}, ("qw16<12,4,staged>",), ()),
    "qw16 symmetric-packed (8,4)": (8, 4, {"symmetric": True}, ("qw16<8,4,staged,sym>",), ()),
    "mt16 (32,8)": (32, 8, {}, ("mt16<32,8,",), ()),
    "general engine (17,9)": (17, 9, {}, (GENERAL,), ()),
}


def _sweep_columns(s):
    """Columns solve_multi carries per sweep on this plan: where its column workspace stops growing; 0: column by
    column."""
    size = [s.solve_multi_workspace_bytes(k) for k in range(1, 34)]
    if size[0] == 0:
        return 0
    return 1 + next(k for k in range(len(size) - 1) if size[k + 1] == size[k])


def _factors(num_rhs):
    """f_c = (-1)^c 2^(e_c), e_c spread over [-20, 20]; f_0 = 1."""
    e = [0] + [int(round(-20 + 40 * (c - 1) / max(1, num_rhs - 2))) for c in range(1, num_rhs)]
    return np.array([(-1.0) ** c * 2.0 ** e[c] for c in range(num_rhs)])


def _refine_multi_cell(family, table, axis, dtype, iterations):
    """Factor and refine the cell's column set from zero.  -> the solver, device (mats, gains, vecs64 columns), the
    cell, the factors f_c (0 for a column of the cell's own), the result, its norms."""
    n, m, kwargs, tags, absent = table[family]
    cell = hi.chain_cell(n, m, axis, dtype)
    T = cell.shape[2]
    s = _solver(n, m, T, hi.BATCH, dtype, **kwargs)
    name = s.kernel_name
    assert all(t in name for t in tags) and not any(t in name for t in absent) and name.count("/" + dtype) == 1, name
    sweep = _sweep_columns(s)
    assert sweep in (0, 8, 16), sweep
    num_rhs = (sweep or 3) + 1
    f = _factors(num_rhs)
    cols = f[:, None, None] * cell.vecs[None]
    own = min(cell.ncols, num_rhs - 1)
    for k in range(own):                                      # the last `own` columns: the cell's own right-hand sides
        cols[num_rhs - own + k] = cell.columns[k]["vecs"]
        f[num_rhs - own + k] = 0.0
    mats = _pack(s, _dev(cell.mats, TORCH[dtype]))
    assert dtype == F64 or np.array_equal(cg.host(_dev(cell.mats, torch.float32)), cell.mats)   # the rounded problem
    vecs64 = _dev(cols)
    gains, status = s.factor(mats)
    sol, norms = s.refine_multi(mats, vecs64, gains, iterations=iterations)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), cell.ref_status)
    return s, (mats, gains, vecs64), cell, f, cols, sol.cpu().numpy(), norms.cpu().numpy()


def _column_errors(cell, f, sol):
    """e of every column against its extended solution, and the e_ref it is held against."""
    own = int((f == 0).sum())
    errs, refs = [], []
    for c in range(len(f)):
        if f[c] != 0:
            errs.append(xr.err(sol[c] / f[c], cell.ext))
            refs.append(cell.e_ref)
        else:
            k = c - (len(f) - own)
            errs.append(xr.err(sol[c][:hi.COL_PROBLEMS], cell.col_ext[k]))
            refs.append(cell.e_ref_cols)
    return np.array(errs), np.array(refs)


def _check_cell(family, axis, cell, f, cols, sol, norms, it):
    errs, refs = _column_errors(cell, f, sol)
    # the norms of column c are |f_c| times those of column 0: shown relative to the column's own right-hand side
    rel = norms / np.abs(cols).max(axis=(1, 2))[None, :, None]
    print(f"REFINE_MULTI | {family} | {axis} | {errs.max():.1e} | {max(refs):.1e} | " +
          " ".join(f"{v:.1e}" for v in rel.max(axis=(1, 2))))
    assert norms.shape == (it + 1, len(f), hi.BATCH), norms.shape
    assert (errs <= rc.CAP + 3 * refs).all(), (family, axis, errs, refs)
    n, m, T = cell.shape
    for c in range(len(f)):                                   # the last row is the residual of the returned iterate
        ref, mag = rc.residual(n, m, T, cell.mats, cols[c], sol[c])
        slack = (rc.bound_factor(n, m) * mag).max(axis=1)
        assert (np.abs(norms[-1, c].astype(rc.LD) - np.abs(ref).max(axis=1)) <= slack).all(), (c, norms[-1, c])


@pytest.mark.parametrize("axis", hi.AXES_F32)
@pytest.mark.parametrize("family", list(REFINE_F32))
def test_refine_multi_f32(family, axis):
    it = rc.ITERATIONS_F32
    s, (mats, gains, vecs64), cell, f, cols, sol, norms = _refine_multi_cell(family, REFINE_F32, axis, F32, it)
    _check_cell(family, axis, cell, f, cols, sol, norms, it)
    # round 1 from zero is the plan's plain solve_multi on the columns rounded to fp32
    first, _ = s.refine_multi(mats, vecs64, gains, iterations=1)
    plain = s.solve_multi(mats, vecs64.float(), gains)
    torch.cuda.synchronize()
    first, plain = first.cpu().numpy(), cg.host(plain)
    gap = np.abs(first - plain).max(axis=2) / np.abs(plain).max(axis=2)
    assert (gap <= 2.0 ** -24).all(), float(gap.max())


@pytest.mark.parametrize("axis", hi.AXES_F64)
@pytest.mark.parametrize("family", list(REFINE_F64))
def test_refine_multi_f64(family, axis):
    it = rc.ITERATIONS_F64
    _, _, cell, f, cols, sol, norms = _refine_multi_cell(family, REFINE_F64, axis, F64, it)
    _check_cell(family, axis, cell, f, cols, sol, norms, it)


def _cols_of(cell, num_rhs):
    return _factors(num_rhs)[:, None, None] * cell.vecs[None]


def test_rounds_one_by_one_are_the_rounds_of_one_call():
    """from_zero = 0 continues from the iterates it is given: two calls of one round are one call of two."""
    cell = hi.chain_cell(12, 4, "cost[1,1e4]")
    n, m, T = cell.shape
    s = _solver(n, m, T, hi.BATCH)
    mats, vecs = _dev(cell.mats), _dev(_cols_of(cell, 9))
    gains, _ = s.factor(mats)
    both, norms = s.refine_multi(mats, vecs, gains, iterations=2)
    one, n1 = s.refine_multi(mats, vecs, gains, iterations=1)
    kept = one.clone()
    two, n2 = s.refine_multi(mats, vecs, gains, iterations=1, sol_cols=one)
    torch.cuda.synchronize()
    assert two.data_ptr() == one.data_ptr()                  # refined in place
    np.testing.assert_array_equal(two.cpu().numpy(), both.cpu().numpy())
    np.testing.assert_array_equal(n1.cpu().numpy(), norms.cpu().numpy()[:2])
    np.testing.assert_array_equal(n2.cpu().numpy(), norms.cpu().numpy()[1:])
    assert not np.array_equal(kept.cpu().numpy(), two.cpu().numpy())


def test_a_failed_problem_keeps_its_iterate_in_every_column():
    cell = hi.chain_cell(12, 4, hi.BENIGN)
    n, m, T = cell.shape
    from sip_optimal_control_amd import ChainShape, FactorStatus
    mats = cell.mats.copy()
    mats[1, ChainShape(n, m, T).mats_off(3)["delta"] + 2] = -1.0
    s = _solver(n, m, T, hi.BATCH)
    f = _factors(9)
    dm, vecs = _dev(mats), _dev(_cols_of(cell, 9))
    gains, status = s.factor(dm)
    start = np.random.default_rng(5).normal(size=(9, hi.BATCH, s.shape.vecs_len))
    sol, norms = s.refine_multi(dm, vecs, gains, iterations=rc.ITERATIONS_F64 + 1, sol_cols=_dev(start))
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, int(FactorStatus.INVALID_DELTA), 0]
    sol = sol.cpu().numpy()
    np.testing.assert_array_equal(sol[:, 1], start[:, 1])               # exactly what went in, in all columns
    good = [0, 2]
    for c in range(9):
        e = xr.err(sol[c][good] / f[c], cell.ext[good])
        assert e <= rc.CAP + 3 * cell.e_ref, (c, e, cell.e_ref)
    # d_status = NULL: nothing is skipped.  Whatever the solve leaves in d for the failed problem is added: d is preset
    # to a value that is not zero.
    s._refine_multi_ws.fill_(0x3f)
    sol2, _ = s.refine_multi(dm, vecs, gains, iterations=rc.ITERATIONS_F64 + 1, sol_cols=_dev(start), use_status=False)
    torch.cuda.synchronize()
    sol2 = sol2.cpu().numpy()
    for c in range(9):
        assert not np.array_equal(sol2[c, 1], start[c, 1]), c
    np.testing.assert_array_equal(sol2[:, good], sol[:, good])

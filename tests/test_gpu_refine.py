"""sip_lqr_residual and sip_lqr_refine on the GPU (BatchedChainLQR.residual / .refine; csrc/chain_residual.hpp).

Residual: against the same formulas in np.longdouble (refine_cases.residual) from the plan's inputs widened to fp64,
every entry held to the derived bound |got - ref| <= (2 n + m + 3) 2^-53 a (refine_cases, module docstring), the norm
to the largest of those bounds; the scaled form (what a refinement round hands the solve: rho / s in the plan's dtype)
to the same bound plus 2^-24 |ref| on fp32 plans, with s exactly the power of two below the norm.

Refinement: batch 3, T = hard_inputs.horizon(n), the cells of refine_cases.CELLS_F32 / CELLS_F64 over every axis; the
result is held to the project's fp64 criterion e <= 1e-9 + 3 e_ref against the extended-precision solve of the
(rounded) problem -- form, 1e-9 and 3 as in tests/test_gpu_hard_inputs.py -- after 4 rounds on fp32 plans and 2 on
fp64 plans.  tests/test_refine_model.py shows without a GPU that a numpy restatement of the scheme meets the same cap
on the same cells in the same number of rounds.

Every refinement test prints "REFINE | family | axis | e by round | e_ref | norms by round (worst problem)"; DESIGN 7.1
holds the table of one run."""
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


# ---- residual against numpy --------------------------------------------------------------------------------------
_DRAWS = {}


def _draw(n, m, T, batch, dtype, wide):
    """Random inputs (float64 numpy, FULL layout) as the plan sees them: mats rounded to the plan's dtype, vecs and sol
    too unless wide; Q and R exactly symmetric.  With the long-double residual, computed once per case."""
    key = (n, m, T, batch, dtype, wide)
    if key not in _DRAWS:
        from sip_optimal_control_amd import ChainShape, synthetic
        mats, vecs = synthetic.make_chain_batch(ChainShape(n, m, T), batch, seed=100 + n + 7 * m, cross_term=0.05)
        mats, vecs = mats.numpy().copy(), vecs.numpy().copy()
        views = hi.chain_views(n, m, T, mats)
        for blk in views["Q"] + views["R"]:
            low = np.tril(blk)
            blk[...] = low + np.tril(blk, -1).transpose(0, 2, 1)
        sol = np.random.default_rng(n * 100 + m).normal(size=vecs.shape)
        if dtype == F32:
            mats = mats.astype(np.float32).astype(np.float64)
            if not wide:
                vecs, sol = (a.astype(np.float32).astype(np.float64) for a in (vecs, sol))
        for a in (mats, vecs, sol):
            a.setflags(write=False)
        ref, mag = rc.residual(n, m, T, mats, vecs, sol)
        _DRAWS[key] = (mats, vecs, sol, ref, mag)
    return _DRAWS[key]


def _check_residual(n, m, got, norm, ref, mag):
    bound = rc.bound_factor(n, m) * mag
    diff = np.abs(got.astype(rc.LD) - ref)
    worst = float((diff / np.where(mag > 0, mag, 1)).max() / 2.0 ** -53)
    print(f"RESIDUAL | ({n},{m}) | worst |got - ref| / (2^-53 a) = {worst:.2f} of {2 * n + m + 3}")
    assert (diff <= bound).all(), worst
    ref_norm = np.abs(ref).max(axis=1)
    assert (np.abs(norm.astype(rc.LD) - ref_norm) <= bound.max(axis=1)).all(), (norm, ref_norm)


def _raw_residual(s, mats, vecs, sol, wide, want_vector=True):
    """sip_lqr_residual with `wide` as given (BatchedChainLQR.residual infers it from the tensors)."""
    res = torch.full((s.batch, s.shape.vecs_len), float("nan"), dtype=torch.float64, device="cuda:0")
    norm = torch.full((s.batch,), float("nan"), dtype=torch.float64, device="cuda:0")
    rc_ = s._lib.sip_lqr_residual(s._plan, ctypes.c_void_p(mats.data_ptr()), ctypes.c_void_p(vecs.data_ptr()),
                                  ctypes.c_void_p(sol.data_ptr()), wide,
                                  ctypes.c_void_p(res.data_ptr() if want_vector else None),
                                  ctypes.c_void_p(norm.data_ptr()),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0, rc_
    torch.cuda.synchronize()
    return res.cpu().numpy(), norm.cpu().numpy()


# (n, m, T or None = horizon(n), batch, dtype, constructor arguments)
RESIDUAL_CASES = [(1, 1, 1, 3, F64, {}), (5, 3, None, 3, F64, {}), (12, 4, None, 3, F64, {}), (16, 4, None, 3, F64, {}),
                  (32, 8, None, 3, F64, {}), (17, 9, None, 3, F64, {}), (35, 3, None, 3, F64, {}),
                  (5, 3, None, 3, F32, {}), (12, 4, None, 3, F32, {}), (32, 8, None, 3, F32, {}),
                  (8, 4, None, 3, F64, {"symmetric": True}), (12, 4, 2, 5, F64, {}), (5, 3, 2, 5, F32, {})]


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("n,m,T,batch,dtype,kwargs", RESIDUAL_CASES,
                         ids=lambda v: str(v) if not isinstance(v, dict) else "+".join(v) or "plain")
def test_residual_against_numpy(n, m, T, batch, dtype, kwargs, wide):
    T = hi.horizon(n) if T is None else T
    s = _solver(n, m, T, batch, dtype, **kwargs)
    assert s.shape.symmetric == bool(kwargs.get("symmetric"))
    mats, vecs, sol, ref, mag = _draw(n, m, T, batch, dtype, bool(wide))
    vt = torch.float64 if wide else TORCH[dtype]
    dm, dv, ds = _pack(s, _dev(mats, TORCH[dtype])), _dev(vecs, vt), _dev(sol, vt)
    assert np.array_equal(cg.host(dv), vecs) and np.array_equal(cg.host(ds), sol)   # the draw is what the plan sees
    got, norm = _raw_residual(s, dm, dv, ds, wide)
    _check_residual(n, m, got, norm, ref, mag)
    _, norm_only = _raw_residual(s, dm, dv, ds, wide, want_vector=False)               # d_res = NULL: the same norms
    np.testing.assert_array_equal(norm_only, norm)
    if dtype == F32 or wide:                                  # the Python method infers `wide` from the tensors
        res2, norm2 = s.residual(dm, dv, ds)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(res2.cpu().numpy(), got)
        np.testing.assert_array_equal(norm2.cpu().numpy(), norm)


@pytest.mark.parametrize("n,m,dtype,kwargs", [(12, 4, F64, {}), (5, 3, F32, {}), (32, 8, F32, {}),
                                              (8, 4, F64, {"symmetric": True})],
                         ids=lambda v: str(v) if not isinstance(v, dict) else "+".join(v) or "plain")
def test_scaled_residual_is_the_residual_over_a_power_of_two(n, m, dtype, kwargs):
    """One refinement round from a given iterate leaves rho / s (the plan's dtype) and s in the refine scratch:
    [rho / s | d | s], each region a multiple of 256 bytes (include/sip_lqr_amd.h)."""
    T = hi.horizon(n)
    s = _solver(n, m, T, 3, dtype, **kwargs)
    mats, vecs, sol, ref, mag = _draw(n, m, T, 3, dtype, True)
    dm = _pack(s, _dev(mats, TORCH[dtype]))
    gains, _ = s.factor(dm)
    _, norms = s.refine(dm, _dev(vecs), gains, iterations=1, sol=_dev(sol))
    torch.cuda.synchronize()
    esize = 4 if dtype == F32 else 8
    region = (3 * s.shape.vecs_len * esize + 255) // 256 * 256
    raw = s._refine_ws.cpu().numpy()
    np_t = np.float32 if dtype == F32 else np.float64
    scaled = raw[:3 * s.shape.vecs_len * esize].view(np_t).reshape(3, -1).astype(np.float64)
    scale = raw[2 * region:2 * region + 24].view(np.float64)
    norm = norms[0].cpu().numpy()
    np.testing.assert_array_equal(scale, rc.scale_of(norm))           # exactly the power of two below the norm
    assert ((scale <= norm) & (norm < 2 * scale)).all() and (np.log2(scale) % 1 == 0).all()
    bound = rc.bound_factor(n, m) * mag + (2.0 ** -24 * np.abs(ref) if dtype == F32 else 0)
    assert (np.abs((scaled * scale[:, None]).astype(rc.LD) - ref) <= bound).all()
    assert np.abs(scaled).max() < 2.0


# ---- the residual of a solved problem ----------------------------------------------------------------------------
def test_residual_of_a_solved_problem():
    cell = hi.chain_cell(12, 4, hi.BENIGN)
    n, m, T = cell.shape
    s = _solver(n, m, T, hi.BATCH)
    mats, vecs = _dev(cell.mats), _dev(cell.vecs)
    sol, _, status = s.factor_solve(mats, vecs)
    res, norm = s.residual(mats, vecs, sol)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    ref, mag = rc.residual(n, m, T, cell.mats, cell.vecs, cg.host(sol))
    _check_residual(n, m, res.cpu().numpy(), norm.cpu().numpy(), ref, mag)
    assert norm.cpu().numpy().max() < 1e-9 * np.abs(cell.vecs).max()   # and it is the residual of a solution


# ---- refinement --------------------------------------------------------------------------------------------------
GENERAL = "tree_generic(chain layout)"
QF32_SEP, MT16_SEP = " + chain_factor_qf32 + chain_solve_qf32", " + chain_factor_mt16 + chain_solve_mt16"
# family -> (n, m, constructor arguments, what the kernel name holds, what it must not hold)
REFINE_F32 = {
    "general engine /f32 (12,4)": (12, 4, {}, (GENERAL,), ()),
    "general engine /f32 (5,3)": (5, 3, {}, (GENERAL,), ()),
    "qf32 (12,4)": (12, 4, {"fused_f32": True}, ("qf32<12,4,",), (QF32_SEP,)),
    "qf32 (5,3)": (5, 3, {"fused_f32": True}, ("qf32<5,3,",), (QF32_SEP,)),
    "qf32 separate sweeps (12,4)": (12, 4, {"fused_f32": True, "separate_sweeps": True}, ("qf32<12,4,", QF32_SEP), ()),
    "qf32 separate sweeps (5,3)": (5, 3, {"fused_f32": True, "separate_sweeps": True}, ("qf32<5,3,", QF32_SEP), ()),
    "mt16/f32 separate sweeps (32,8)": (32, 8, {"separate_sweeps": True}, ("mt16<32,8,", MT16_SEP), ()),
}
REFINE_F64 = {
    "qw16 staged (12,4)": (12, 4, {}, ("qw16<12,4,staged>",), ()),
    "qw16 symmetric-packed (8,4)": (8, 4, {"symmetric": True}, ("qw16<8,4,staged,sym>",), ()),
    "mt16 (32,8)": (32, 8, {}, ("mt16<32,8,",), ()),
    "general engine (17,9)": (17, 9, {}, (GENERAL,), ()),
}


def _refine_cell(family, table, axis, dtype, iterations):
    """Factor, refine from zero in one call, and the same round by round (for the errors by round).  -> the solver,
    device mats and gains, the cell, the result, its norms, the errors by round."""
    n, m, kwargs, tags, absent = table[family]
    cell = hi.chain_cell(n, m, axis, dtype)
    T = cell.shape[2]
    s = _solver(n, m, T, hi.BATCH, dtype, **kwargs)
    name = s.kernel_name
    assert all(t in name for t in tags) and not any(t in name for t in absent) and name.count("/" + dtype) == 1, name
    mats = _pack(s, _dev(cell.mats, TORCH[dtype]))
    assert dtype == F64 or np.array_equal(cg.host(_dev(cell.mats, torch.float32)), cell.mats)   # the rounded problem
    vecs64 = _dev(cell.vecs)
    gains, status = s.factor(mats)
    sol, norms = s.refine(mats, vecs64, gains, iterations=iterations)
    step, errs = None, []
    for _ in range(iterations):
        step, _ = s.refine(mats, vecs64, gains, iterations=1, sol=step)
        errs.append(xr.err(step.cpu().numpy(), cell.ext))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), cell.ref_status)
    sol, norms = sol.cpu().numpy(), norms.cpu().numpy()
    print(f"REFINE | {family} | {axis} | " + " ".join(f"{e:.1e}" for e in errs) + f" | {cell.e_ref:.1e} | " +
          " ".join(f"{v:.1e}" for v in norms.max(axis=1)))
    return s, (mats, gains), cell, sol, norms, errs


def _check_last_norm(cell, sol, norms):
    n, m, T = cell.shape
    ref, mag = rc.residual(n, m, T, cell.mats, cell.vecs, sol)
    slack = (rc.bound_factor(n, m) * mag).max(axis=1)
    assert (np.abs(norms[-1].astype(rc.LD) - np.abs(ref).max(axis=1)) <= slack).all(), (norms[-1], np.abs(ref).max(axis=1))


@pytest.mark.parametrize("axis", hi.AXES_F32)
@pytest.mark.parametrize("family", list(REFINE_F32))
def test_refine_f32(family, axis):
    it = rc.ITERATIONS_F32
    s, (mats, gains), cell, sol, norms, errs = _refine_cell(family, REFINE_F32, axis, F32, it)
    e = xr.err(sol, cell.ext)
    assert e <= rc.CAP + 3 * cell.e_ref, (family, axis, e, errs, cell.e_ref)
    assert norms.shape == (it + 1, hi.BATCH) and (norms[1] <= norms[0]).all(), norms
    _check_last_norm(cell, sol, norms)
    # round 1 from zero is the plan's plain solve
    first, _ = s.refine(mats, _dev(cell.vecs), gains, iterations=1)
    plain = s.solve(mats, _dev(cell.vecs, torch.float32), gains)
    torch.cuda.synchronize()
    first, plain = first.cpu().numpy(), cg.host(plain)
    assert (np.abs(first - plain).max(axis=1) <= 2.0 ** -24 * np.abs(plain).max(axis=1)).all(), \
        float((np.abs(first - plain).max(axis=1) / np.abs(plain).max(axis=1)).max())


@pytest.mark.parametrize("axis", hi.AXES_F64)
@pytest.mark.parametrize("family", list(REFINE_F64))
def test_refine_f64(family, axis):
    it = rc.ITERATIONS_F64
    _, _, cell, sol, norms, errs = _refine_cell(family, REFINE_F64, axis, F64, it)
    e = xr.err(sol, cell.ext)
    assert e <= rc.CAP + 3 * cell.e_ref, (family, axis, e, errs, cell.e_ref)
    assert norms.shape == (it + 1, hi.BATCH) and (norms[2] <= norms[1]).all(), norms
    _check_last_norm(cell, sol, norms)


def test_rounds_one_by_one_are_the_rounds_of_one_call():
    """from_zero = 0 continues from the iterate it is given: two calls of one round are one call of two."""
    cell = hi.chain_cell(12, 4, "cost[1,1e4]")
    n, m, T = cell.shape
    s = _solver(n, m, T, hi.BATCH)
    mats, vecs = _dev(cell.mats), _dev(cell.vecs)
    gains, _ = s.factor(mats)
    both, norms = s.refine(mats, vecs, gains, iterations=2)
    one, n1 = s.refine(mats, vecs, gains, iterations=1)
    kept = one.clone()
    two, n2 = s.refine(mats, vecs, gains, iterations=1, sol=one)
    torch.cuda.synchronize()
    assert two.data_ptr() == one.data_ptr()                  # refined in place
    np.testing.assert_array_equal(two.cpu().numpy(), both.cpu().numpy())
    np.testing.assert_array_equal(n1.cpu().numpy(), norms.cpu().numpy()[:2])
    np.testing.assert_array_equal(n2.cpu().numpy(), norms.cpu().numpy()[1:])
    assert not np.array_equal(kept.cpu().numpy(), two.cpu().numpy())


# ---- the fused mt16/f32 sweep at delta[1e-1,1e2] -------------------------------------------------------------------
OPEN = {"mt16/f32 fused (32,8)": (32, 8, {}, ("mt16<32,8,",), (MT16_SEP,))}


def test_refine_on_the_fused_mt16_f32_sweep_at_large_delta():
    """The cell tests/test_gpu_hard_inputs.py keeps as a strict expected failure (first solve 2.3e-2): whether the
    refinement contracts on that kernel, 8 rounds, figures printed.

    It does not.  One run on an MI355X: e by round 2.3e-02 4.5e-02 1.1e-01 2.8e-01 7.1e-01 1.8e+00 4.5e+00 1.1e+01,
    residual norms 3.8 4.8 12 30 76 1.9e2 4.8e2 1.2e3 3.1e3 (a growth of 2.5 per round).  So the cap is
    not asserted here: the run is a record, held only to finite values and to a last norm that is the residual of
    the returned iterate.  The same plan with separate_sweeps converges (test_refine_f32)."""
    it = rc.ITERATIONS_OPEN
    _, _, cell, sol, norms, errs = _refine_cell("mt16/f32 fused (32,8)", OPEN, "delta[1e-1,1e2]", F32, it)
    assert norms.shape == (it + 1, hi.BATCH) and np.isfinite(norms).all() and np.isfinite(sol).all()
    _check_last_norm(cell, sol, norms)


# ---- failed problems ---------------------------------------------------------------------------------------------
def test_a_failed_problem_keeps_its_iterate():
    cell = hi.chain_cell(12, 4, hi.BENIGN)
    n, m, T = cell.shape
    from sip_optimal_control_amd import ChainShape
    mats = cell.mats.copy()
    mats[1, ChainShape(n, m, T).mats_off(3)["delta"] + 2] = -1.0
    s = _solver(n, m, T, hi.BATCH)
    dm, vecs = _dev(mats), _dev(cell.vecs)
    gains, status = s.factor(dm)
    sol, norms = s.refine(dm, vecs, gains, iterations=rc.ITERATIONS_F64)
    torch.cuda.synchronize()
    from sip_optimal_control_amd import FactorStatus
    assert status.cpu().numpy().tolist() == [0, int(FactorStatus.INVALID_DELTA), 0]
    sol = sol.cpu().numpy()
    assert (sol[1] == 0).all()                                           # exactly what went in: zeros
    good = [0, 2]
    e = xr.err(sol[good], cell.ext[good])
    assert e <= rc.CAP + 3 * cell.e_ref, (e, cell.e_ref)
    # d_status = NULL: nothing is skipped.  Whatever the solve leaves in d for the failed problem (the fused kernels
    # leave it unspecified or untouched) is added: d is preset to a value that is not zero.
    s._refine_ws.fill_(0x3f)
    sol2, _ = s.refine(dm, vecs, gains, iterations=rc.ITERATIONS_F64, use_status=False)
    torch.cuda.synchronize()
    sol2 = sol2.cpu().numpy()
    assert not (sol2[1] == 0).all()
    np.testing.assert_array_equal(sol2[good], sol[good])

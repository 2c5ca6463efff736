"""sip_lqr_vjp_mats on the GPU (csrc/chain_vjp.hpp): the kernel alone against the numpy restatement of its formulas
(tests/vjp_cases.py) on random sol and adj -- no solve involved -- batch 5.

Every entry is held to the derived bound of vjp_cases: |got - ref| <= 3 * 2^-53 * a, a the sum of the absolute values of
the entry's terms (two roundings in fp64: the product and the fused sum; the factor 1/2 is exact), plus 2^-24 |ref| on
the all-float form for the one rounding to float.  Each case prints the worst ratio |got - ref| / (2^-53 a).

The output is pre-filled with NaN and sits between guard words: no NaN survives (every scalar is written) and no guard
changes (nothing else is).  (3, 2, 3) has mats_len = 123, so problems 1 and 3 start off a 16-byte boundary in both
dtypes; one case more starts the whole output one scalar off."""
import ctypes

import numpy as np
import pytest

import chain_guards as cg
import vjp_cases as vc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, F64 = "f32", "f64"
TORCH = {F32: torch.float32, F64: torch.float64}
BATCH = 5

# (n, m, T, symmetric); (33, 17, 2) is a general-engine plan, and at (128, 1, 1) the decoded stage image (33,153 words)
# does not fit the kernel's LDS budget: the form that decodes in place
SHAPES = [(1, 1, 0, False), (1, 1, 1, False), (3, 2, 3, False), (5, 3, 7, False), (12, 4, 5, False), (12, 4, 5, True),
          (16, 8, 3, False), (32, 8, 2, False), (33, 17, 2, False), (128, 1, 1, False)]
# (plan dtype, wide): both dtypes, and the double form on an fp32 plan
FORMS = [(F64, 0), (F32, 0), (F32, 1)]
CASES = [(n, m, T, sym, dtype, wide) for n, m, T, sym in SHAPES for dtype, wide in FORMS if not (sym and dtype == F32)]


def _solver(n, m, T, dtype, symmetric):
    from sip_optimal_control_amd import BatchedChainLQR
    return BatchedChainLQR(n, m, T, BATCH, dtype=TORCH[dtype], symmetric=symmetric)


_DRAWS = {}


def _draw(n, m, T, symmetric, f32_io):
    """sol, adj (float64 numpy, rounded to float where the kernel reads floats) and the long-double reference with its
    magnitudes, computed once per case and read-only."""
    key = (n, m, T, symmetric, f32_io)
    if key not in _DRAWS:
        from sip_optimal_control_amd import ChainShape
        rng = np.random.default_rng(1000 + 37 * n + 5 * m + T)
        shape = ChainShape(n, m, T, symmetric=symmetric)
        sol, adj = rng.normal(size=(BATCH, shape.vecs_len)), rng.normal(size=(BATCH, shape.vecs_len))
        if f32_io:
            sol, adj = (a.astype(np.float32).astype(np.float64) for a in (sol, adj))
        ref, mag = vc.grad_mats(n, m, T, sol, adj, symmetric=symmetric)
        assert ref.shape == (BATCH, shape.mats_len)
        for a in (sol, adj, ref, mag):
            a.setflags(write=False)
        _DRAWS[key] = (sol, adj, ref, mag)
    return _DRAWS[key]


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0", dtype=dtype)


def _launch(s, sol, adj, wide, status, shift=0):
    """sip_lqr_vjp_mats into a NaN-filled output between guards; shift: scalars the output starts off the frame's
    16-byte aligned view.  -> (output [BATCH, mats_len] numpy in its own dtype, guards intact)."""
    io = torch.float64 if wide else s.dtype
    L = s.shape.mats_len
    full, _ = cg.framed((BATCH * L + shift,), io, "cuda:0")
    full[cg.GUARD + shift:cg.GUARD + shift + BATCH * L] = float("nan")
    out = full[cg.GUARD + shift:cg.GUARD + shift + BATCH * L]
    rc_ = s._lib.sip_lqr_vjp_mats(s._plan, ctypes.c_void_p(sol.data_ptr()), ctypes.c_void_p(adj.data_ptr()), wide,
                                  ctypes.c_void_p(status.data_ptr() if status is not None else None),
                                  ctypes.c_void_p(out.data_ptr()),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0, rc_
    torch.cuda.synchronize()
    want = cg._sentinel(io)
    intact = bool((full[:cg.GUARD + shift] == want).all()) and bool((full[cg.GUARD + shift + BATCH * L:] == want).all())
    return out.cpu().numpy().reshape(BATCH, L), intact


def _check(tag, got, ref, mag, f32_out):
    assert not np.isnan(got).any(), (tag, "a scalar of the output was not written", int(np.isnan(got).sum()))
    diff = np.abs(got.astype(vc.LD) - ref)
    bound = vc.kernel_bound(mag, ref, f32_out)
    if f32_out:
        diff_r = np.maximum(diff - 2.0 ** -24 * np.abs(ref), 0)
    else:
        diff_r = diff
    worst = float((diff_r / np.where(mag > 0, mag, 1)).max() / 2.0 ** -53) if ref.size else 0.0
    print(f"VJP | {tag} | worst (|got - ref|{' - 2^-24 |ref|' if f32_out else ''}) / (2^-53 a) = {worst:.2f} "
          f"of {vc.C_ROUNDINGS}")
    assert (diff <= bound).all(), (tag, worst)


@pytest.mark.parametrize("n,m,T,symmetric,dtype,wide", CASES,
                         ids=[f"{n}-{m}-{T}-{'sym' if sym else 'full'}-{d}-wide{w}" for n, m, T, sym, d, w in CASES])
def test_kernel_against_numpy(n, m, T, symmetric, dtype, wide):
    s = _solver(n, m, T, dtype, symmetric)
    assert s.shape.symmetric == symmetric
    f32_io = dtype == F32 and not wide
    sol, adj, ref, mag = _draw(n, m, T, symmetric, f32_io)
    io = torch.float32 if f32_io else torch.float64
    ds, da = _dev(sol, io), _dev(adj, io)
    assert np.array_equal(cg.host(ds), sol) and np.array_equal(cg.host(da), adj)      # the draw is what the kernel reads
    tag = f"({n},{m},{T}){' sym' if symmetric else ''} {dtype} wide={wide}"
    got, intact = _launch(s, ds, da, wide, None)
    assert intact, (tag, "a guard word changed")
    _check(tag, got, ref, mag, f32_io)
    again, _ = _launch(s, ds, da, wide, None)                                          # two launches, the same bits
    assert got.tobytes() == again.tobytes(), tag
    by_method = s.vjp_mats(ds, da, use_status=False)                                   # the Python method infers `wide`
    torch.cuda.synchronize()
    assert by_method.dtype == io and by_method.cpu().numpy().tobytes() == got.tobytes(), tag


@pytest.mark.parametrize("dtype", [F64, F32])
def test_an_output_that_starts_one_scalar_off_alignment(dtype):
    """d_grad_mats need only be aligned to its scalar: every problem of (3, 2, 3) then starts off a 16-byte boundary in
    some way, and the first and the last piece of the whole output are partial."""
    n, m, T = 3, 2, 3
    s = _solver(n, m, T, dtype, False)
    sol, adj, ref, mag = _draw(n, m, T, False, dtype == F32)
    ds, da = _dev(sol, TORCH[dtype]), _dev(adj, TORCH[dtype])
    aligned, _ = _launch(s, ds, da, 0, None)
    for shift in (1, 3) if dtype == F32 else (1,):
        got, intact = _launch(s, ds, da, 0, None, shift=shift)
        assert intact, ("a guard word changed", shift)
        _check(f"(3,2,3) {dtype} output + {shift} scalar", got, ref, mag, dtype == F32)
        assert got.tobytes() == aligned.tobytes(), shift                               # the same values wherever it lies


@pytest.mark.parametrize("n,m,T,symmetric,dtype,wide", [(3, 2, 3, False, F64, 0), (3, 2, 3, False, F32, 0),
                                                        (12, 4, 5, True, F64, 0), (32, 8, 2, False, F32, 1)])
def test_a_failed_problem_gets_zeros_by_a_branch(n, m, T, symmetric, dtype, wide):
    """One problem whose status is not SUCCESS and whose sol and adj are NaN: exact zeros there (a multiplication by
    zero would leave NaN), its neighbours bit for bit what they are without it; d_status = NULL masks nothing."""
    s = _solver(n, m, T, dtype, symmetric)
    f32_io = dtype == F32 and not wide
    sol, adj, ref, mag = _draw(n, m, T, symmetric, f32_io)
    io = torch.float32 if f32_io else torch.float64
    ds, da = _dev(sol, io), _dev(adj, io)
    plain, _ = _launch(s, ds, da, wide, None)
    failed, good = 2, [0, 1, 3, 4]
    ds[failed], da[failed] = float("nan"), float("nan")
    status = torch.zeros(BATCH, dtype=torch.int32, device="cuda:0")
    status[failed] = 3
    got, intact = _launch(s, ds, da, wide, status)
    assert intact
    assert (got[failed] == 0).all() and not np.signbit(got[failed]).any()
    assert got[good].tobytes() == plain[good].tobytes()
    _check("with a failed neighbour", got[good], ref[good], mag[good], f32_io)
    unmasked, intact = _launch(s, ds, da, wide, None)
    assert intact
    assert np.isnan(unmasked[failed]).all()                                            # nothing is masked
    assert unmasked[good].tobytes() == plain[good].tobytes()
    all_ok, _ = _launch(s, ds, da, wide, torch.zeros(BATCH, dtype=torch.int32, device="cuda:0"))
    assert np.isnan(all_ok[failed]).all() and all_ok[good].tobytes() == plain[good].tobytes()

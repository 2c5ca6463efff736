"""sip_lqr_vjp_mats_multi on the GPU (csrc/chain_vjp_cols.hpp): the kernel alone against the numpy restatement of its
formulas (tests/vjp_cases.py) in long double, summed over the columns, on random columns -- no solve involved -- batch 5.

Reference ref = sum_c ref_c and magnitude a = sum_c a_c of vjp_cases.grad_mats.  Bound, derived: an entry of k columns
is a chain of one product and 2 k - 1 fused multiply-adds in fp64, 2 k roundings, each of a partial sum that is at most
a in magnitude (to first order), and s is exact: |got - ref| <= (2 k + 1) 2^-53 a, the + 1 covering the second-order
terms and the 2^-64 of the long-double reference as the 3 of vjp_cases does for k = 1.  Float output rounds the result
once, 2^-24 |ref|, and every group boundary but the last rounds a partial sum (at most a) to float once more:
+ (G - 1) 2^-24 a (1 + 2^-20) for G groups.  Each case prints the worst ratio of the fp64 part to 2^-53 a.

Column counts 1, 3, C, C + 1 and 2 C + 1 with C = vjp_multi_columns: a partial group, a full one, two and three groups.
The output is pre-filled with NaN and sits between guard words: no NaN survives (every scalar is written, and the first
group does not read the output) and no guard changes."""
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
MAX_COLS = 17                                                # 2 C + 1 at C = 8

# (n, m, T, symmetric); (33, 17, 2) is a general-engine plan; at (128, 1, 1) 7 columns fit and the table does not
SHAPES = [(1, 1, 0, False), (3, 2, 3, False), (12, 4, 5, False), (12, 4, 5, True), (32, 8, 2, False),
          (33, 17, 2, False), (128, 1, 1, False)]
FORMS = [(F64, 0), (F32, 0), (F32, 1)]
CASES = [(n, m, T, sym, dtype, wide) for n, m, T, sym in SHAPES for dtype, wide in FORMS if not (sym and dtype == F32)]
IDS = [f"{n}-{m}-{T}-{'sym' if sym else 'full'}-{d}-wide{w}" for n, m, T, sym, d, w in CASES]


def _solver(n, m, T, dtype, symmetric):
    from sip_optimal_control_amd import BatchedChainLQR
    return BatchedChainLQR(n, m, T, BATCH, dtype=TORCH[dtype], symmetric=symmetric)


_DRAWS = {}


def _draw(n, m, T, symmetric, f32_io):
    """sol_cols, adj_cols [MAX_COLS, BATCH, vecs_len] (float64 numpy, rounded to float where the kernel reads floats)
    and the running sums of the long-double reference and its magnitudes: ref[k], mag[k] over the first k columns.
    Computed once per case and read-only."""
    key = (n, m, T, symmetric, f32_io)
    if key not in _DRAWS:
        from sip_optimal_control_amd import ChainShape
        rng = np.random.default_rng(2000 + 37 * n + 5 * m + T)
        shape = ChainShape(n, m, T, symmetric=symmetric)
        sol, adj = (rng.normal(size=(MAX_COLS, BATCH, shape.vecs_len)) for _ in range(2))
        if f32_io:
            sol, adj = (a.astype(np.float32).astype(np.float64) for a in (sol, adj))
        ref = [np.zeros((BATCH, shape.mats_len), dtype=vc.LD)]
        mag = [np.zeros((BATCH, shape.mats_len), dtype=vc.LD)]
        for c in range(MAX_COLS):
            r, a = vc.grad_mats(n, m, T, sol[c], adj[c], symmetric=symmetric)
            ref.append(ref[-1] + r), mag.append(mag[-1] + a)
        for a in [sol, adj] + ref + mag:
            a.setflags(write=False)
        _DRAWS[key] = (sol, adj, ref, mag)
    return _DRAWS[key]


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0", dtype=dtype)


def _launch(s, sol_cols, adj_cols, k, wide, status, shift=0):
    """sip_lqr_vjp_mats_multi on the first k columns into a NaN-filled output between guards; shift: scalars the output
    starts off the frame's 16-byte aligned view.  -> (output [BATCH, mats_len] numpy in its own dtype, guards intact)."""
    io = torch.float64 if wide else s.dtype
    L = s.shape.mats_len
    full, _ = cg.framed((BATCH * L + shift,), io, "cuda:0")
    full[cg.GUARD + shift:cg.GUARD + shift + BATCH * L] = float("nan")
    out = full[cg.GUARD + shift:cg.GUARD + shift + BATCH * L]
    rc_ = s._lib.sip_lqr_vjp_mats_multi(
        s._plan, ctypes.c_void_p(sol_cols.data_ptr()), ctypes.c_void_p(adj_cols.data_ptr()), k, wide,
        ctypes.c_void_p(status.data_ptr() if status is not None else None), ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0, rc_
    torch.cuda.synchronize()
    want = cg._sentinel(io)
    intact = bool((full[:cg.GUARD + shift] == want).all()) and bool((full[cg.GUARD + shift + BATCH * L:] == want).all())
    return out.cpu().numpy().reshape(BATCH, L), intact


def _groups(k, per_launch):
    return max(1, -(-k // per_launch))


def _check(tag, got, ref, mag, k, f32_out, groups):
    """The bound of the module docstring; prints the worst ratio of what is left for the fp64 roundings to 2^-53 a."""
    assert not np.isnan(got).any(), (tag, "a scalar of the output was not written", int(np.isnan(got).sum()))
    diff = np.abs(got.astype(vc.LD) - ref)
    to_float = 2.0 ** -24 * np.abs(ref) + (groups - 1) * 2.0 ** -24 * mag * (1 + 2.0 ** -20) if f32_out else 0
    bound = (2 * k + 1) * 2.0 ** -53 * mag + to_float
    left = np.maximum(diff - to_float, 0)
    worst = float((left / np.where(mag > 0, mag, 1)).max() / 2.0 ** -53) if ref.size else 0.0
    print(f"VJP MULTI | {tag} | {k} columns, {groups} group(s) | worst (|got - ref|"
          f"{' - float roundings' if f32_out else ''}) / (2^-53 a) = {worst:.2f} of {2 * k + 1}")
    assert (diff <= bound).all(), (tag, k, worst)


def _setup(n, m, T, symmetric, dtype, wide):
    s = _solver(n, m, T, dtype, symmetric)
    assert s.shape.symmetric == symmetric
    f32_io = dtype == F32 and not wide
    sol, adj, ref, mag = _draw(n, m, T, symmetric, f32_io)
    io = torch.float32 if f32_io else torch.float64
    ds, da = _dev(sol, io), _dev(adj, io)
    assert np.array_equal(cg.host(ds), sol) and np.array_equal(cg.host(da), adj)      # the draw is what the kernel reads
    return s, f32_io, io, ds, da, ref, mag


@pytest.mark.parametrize("n,m,T,symmetric,dtype,wide", CASES, ids=IDS)
def test_kernel_against_long_double(n, m, T, symmetric, dtype, wide):
    s, f32_io, io, ds, da, ref, mag = _setup(n, m, T, symmetric, dtype, wide)
    C = s.vjp_multi_columns
    assert C == (7 if n == 128 else 8) and 2 * C + 1 <= MAX_COLS
    tag = f"({n},{m},{T}){' sym' if symmetric else ''} {dtype} wide={wide}"
    results = {}
    for k in (1, 3, C, C + 1, 2 * C + 1):
        got, intact = _launch(s, ds, da, k, wide, None)
        assert intact, (tag, k, "a guard word changed")
        _check(tag, got, ref[k], mag[k], k, f32_io, _groups(k, C))
        results[k] = got
    # one column: the bits of the single-column kernel
    single = s.vjp_mats(ds[0], da[0], use_status=False)
    torch.cuda.synchronize()
    assert single.dtype == io and single.cpu().numpy().tobytes() == results[1].tobytes(), tag
    # two calls, the same bits (three groups); the Python method infers `wide` and the column count
    again, _ = _launch(s, ds, da, 2 * C + 1, wide, None)
    assert again.tobytes() == results[2 * C + 1].tobytes(), tag
    by_method = s.vjp_mats_multi(ds[:C + 1], da[:C + 1], use_status=False)
    torch.cuda.synchronize()
    assert by_method.dtype == io and by_method.cpu().numpy().tobytes() == results[C + 1].tobytes(), tag
    # the empty sum: zeros, every scalar written
    empty, intact = _launch(s, ds, da, 0, wide, None)
    assert intact and (empty == 0).all() and not np.signbit(empty).any(), tag
    # columns 1 .. all zero: column 0 alone, numerically (a sum that is zero may differ in sign from a product that
    # is), also where the zero columns make up a later group
    ds[1:], da[1:] = 0, 0
    for k in (3, C + 1, 2 * C + 1):
        got, intact = _launch(s, ds, da, k, wide, None)
        assert intact and not np.isnan(got).any() and (got == results[1]).all(), (tag, k)


@pytest.mark.parametrize("n,m,T,symmetric,dtype,wide",
                         [(3, 2, 3, False, F64, 0), (3, 2, 3, False, F32, 0), (3, 2, 3, False, F32, 1),
                          (12, 4, 5, True, F64, 0), (12, 4, 5, False, F32, 0), (32, 8, 2, False, F64, 0),
                          (128, 1, 1, False, F64, 0), (128, 1, 1, False, F32, 0)])
def test_the_grouping_does_not_change_a_double_result(n, m, T, symmetric, dtype, wide, monkeypatch):
    """9 columns in groups of 3 (SIP_LQR_VJP_MULTI_COLUMNS, read per call) against the default grouping (8 + 1, or
    7 + 2): the same bytes with double output; with float output both are within the bound of their own grouping."""
    s, f32_io, io, ds, da, ref, mag = _setup(n, m, T, symmetric, dtype, wide)
    C = s.vjp_multi_columns
    k = 9
    tag = f"({n},{m},{T}){' sym' if symmetric else ''} {dtype} wide={wide}"
    default, intact = _launch(s, ds, da, k, wide, None)
    assert intact
    _check(tag + " default grouping", default, ref[k], mag[k], k, f32_io, _groups(k, C))
    monkeypatch.setenv("SIP_LQR_VJP_MULTI_COLUMNS", "3")
    by_three, intact = _launch(s, ds, da, k, wide, None)
    assert intact
    _check(tag + " groups of 3", by_three, ref[k], mag[k], k, f32_io, 3)
    assert s.vjp_multi_columns == C                            # the plan's figure, not the cap
    monkeypatch.setenv("SIP_LQR_VJP_MULTI_COLUMNS", "1")
    by_one, intact = _launch(s, ds, da, k, wide, None)
    assert intact
    _check(tag + " groups of 1", by_one, ref[k], mag[k], k, f32_io, k)
    if not f32_io:
        assert by_three.tobytes() == default.tobytes() and by_one.tobytes() == default.tobytes(), tag


@pytest.mark.parametrize("dtype", [F64, F32])
def test_an_output_that_starts_one_scalar_off_alignment(dtype):
    """d_grad_mats need only be aligned to its scalar: every problem of (3, 2, 3) then starts off a 16-byte boundary in
    some way; the accumulating groups read and write the same partial pieces."""
    n, m, T = 3, 2, 3
    s, f32_io, io, ds, da, ref, mag = _setup(n, m, T, False, dtype, 0)
    C = s.vjp_multi_columns
    for k in (3, C + 1, 2 * C + 1):
        aligned, _ = _launch(s, ds, da, k, 0, None)
        for shift in (1, 3) if dtype == F32 else (1,):
            got, intact = _launch(s, ds, da, k, 0, None, shift=shift)
            assert intact, ("a guard word changed", k, shift)
            _check(f"(3,2,3) {dtype} output + {shift} scalar", got, ref[k], mag[k], k, f32_io, _groups(k, C))
            assert got.tobytes() == aligned.tobytes(), (k, shift)                      # the same values wherever it lies


@pytest.mark.parametrize("n,m,T,symmetric,dtype,wide", [(3, 2, 3, False, F64, 0), (3, 2, 3, False, F32, 0),
                                                        (12, 4, 5, True, F64, 0), (32, 8, 2, False, F32, 1),
                                                        (128, 1, 1, False, F64, 0)])
def test_a_failed_problem_gets_zeros_by_a_branch(n, m, T, symmetric, dtype, wide):
    """One problem whose status is not SUCCESS and whose sol and adj are NaN in every column: exact +0 there -- from
    the first group, the later ones leave it alone -- and its neighbours bit for bit what they are without it."""
    s, f32_io, io, ds, da, ref, mag = _setup(n, m, T, symmetric, dtype, wide)
    C = s.vjp_multi_columns
    failed, good = 2, [0, 1, 3, 4]
    plain = {k: _launch(s, ds, da, k, wide, None)[0] for k in (3, C + 1)}
    ds[:, failed], da[:, failed] = float("nan"), float("nan")
    status = torch.zeros(BATCH, dtype=torch.int32, device="cuda:0")
    status[failed] = 3
    for k in (3, C + 1):
        got, intact = _launch(s, ds, da, k, wide, status)
        assert intact
        assert (got[failed] == 0).all() and not np.signbit(got[failed]).any(), k
        assert got[good].tobytes() == plain[k][good].tobytes(), k
        _check("with a failed neighbour", got[good], ref[k][good], mag[k][good], k, f32_io, _groups(k, C))
        unmasked, intact = _launch(s, ds, da, k, wide, None)
        assert intact
        assert np.isnan(unmasked[failed]).all()                                        # nothing is masked
        assert unmasked[good].tobytes() == plain[k][good].tobytes()

"""sip_lqr_vjp_multi on the GPU (BatchedChainLQR.vjp_multi): the backward pass of solve_multi end to end, batch 5, at 3
and 9 columns, on synthetic.make_chain_batch draws, against oracle/dense_kkt.solve.

grad_vecs_cols holds the adjoints lambda_c, K lambda_c + g_c = 0: it has the bytes of solve_multi on the g columns, and
every column is held against the dense solve by the criterion the parity test of the same plan applies to `sol`
(tests/test_gpu_vjp_solve.py: fp64 1e-9, fp32 chain_guards.F32_TOL, per problem max |got - ref| <= TOL max |ref|).  The
forward columns are held to the same.

grad_mats is held against sum_c of the numpy restatement (tests/vjp_cases.py) on the dense z_c and lambda_c, within
sum_c vjp_cases.propagated_bound with the caps e_z = TOL max |z_c| and e_l = TOL max |lambda_c| asserted first: the
derivation of tests/test_gpu_vjp_solve.py, column by column, and a sum of terms moves by at most the sum of what the
terms move.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import chain_guards as cg
import vjp_cases as vc
from oracle import dense_kkt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BATCH = 5
# (n, m, T, torch dtype name, constructor arguments, criterion of the plan's parity test)
PLANS = [(12, 4, 5, "float64", {}, cg.F64_TOL),
         (12, 4, 5, "float32", {"fused_f32": True, "separate_sweeps": True}, cg.F32_TOL),
         (32, 8, 2, "float32", {"separate_sweeps": True}, cg.F32_TOL),
         (33, 17, 2, "float64", {}, cg.F64_TOL)]
CASES = [p + (k,) for p in PLANS for k in (3, 9)]
IDS = [f"{n}-{m}-{T}-{d}-{'+'.join(kw) or 'plain'}-{k}cols" for n, m, T, d, kw, _, k in CASES]


def _pack_sol(n, m, T, x, u, y):
    out = []
    for i in range(T + 1):
        out += [x[i], y[i]] + ([u[i]] if i < T else [])
    return np.concatenate(out)


def _dense(n, m, T, mats, vecs):
    """[B, vecs_len]: dense_kkt.solve of every problem (FULL-layout float64 mats, vecs as the right-hand side)."""
    par, ch = list(range(T)), list(range(1, T + 1))
    out = []
    for b in range(mats.shape[0]):
        blocks = dense_kkt.chain_blocks_from_packed(n, m, T, mats[b], vecs[b])
        out.append(_pack_sol(n, m, T, *dense_kkt.solve(par, ch, [n] * (T + 1), [m] * T, blocks)))
    return np.stack(out)


def _setup(n, m, T, dtype, kwargs, cols):
    from sip_optimal_control_amd import BatchedChainLQR
    dt = getattr(torch, dtype)
    s = BatchedChainLQR(n, m, T, BATCH, dtype=dt, **kwargs)
    for opt in ("fused_f32", "separate_sweeps"):
        assert getattr(s, "has_" + opt) == bool(kwargs.get(opt)), (opt, s.kernel_name)
    mats, _ = cg.make(n, m, T, BATCH, seed=6100 + 13 * n + T, dtype=dt)
    gen = torch.Generator(device="cuda:0").manual_seed(91 + n)
    draw = lambda: torch.randn(cols, BATCH, s.shape.vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(dt)
    return s, mats, draw(), draw()


def _forward_backward(s, mats, vecs_cols, g_cols, **kwargs):
    gains, status = s.factor(mats)
    sol_cols = s.solve_multi(mats, vecs_cols, gains)
    grad_mats, grad_vecs_cols = s.vjp_multi(mats, sol_cols, g_cols, gains, **kwargs)
    torch.cuda.synchronize()
    return sol_cols, gains, status.clone(), grad_mats, grad_vecs_cols


@pytest.mark.parametrize("n,m,T,dtype,kwargs,tol,cols", CASES, ids=IDS)
def test_backward_pass_against_the_dense_solve(n, m, T, dtype, kwargs, tol, cols):
    s, mats, vecs_cols, g_cols = _setup(n, m, T, dtype, kwargs, cols)
    sol_cols, gains, status, grad_mats, lam_cols = _forward_backward(s, mats, vecs_cols, g_cols)
    assert (status.cpu().numpy() == 0).all()
    assert grad_mats.dtype == s.dtype and tuple(grad_mats.shape) == (BATCH, s.shape.mats_len)
    assert lam_cols.dtype == s.dtype and tuple(lam_cols.shape) == (cols, BATCH, s.shape.vecs_len)
    # the adjoints are solve_multi on the g columns, bit for bit
    by_solve = s.solve_multi(mats, g_cols, gains)
    torch.cuda.synchronize()
    assert torch.equal(by_solve, lam_cols)
    hm = cg.host(mats)                                          # the problem the device sees, in float64
    ref = np.zeros((BATCH, s.shape.mats_len), dtype=vc.LD)
    bound = np.zeros_like(ref)
    worst_z = worst_l = 0.0
    for c in range(cols):
        z_ref, l_ref = _dense(n, m, T, hm, cg.host(vecs_cols[c])), _dense(n, m, T, hm, cg.host(g_cols[c]))
        ez, el = cg.rel_err(cg.host(sol_cols[c]), z_ref), cg.rel_err(cg.host(lam_cols[c]), l_ref)
        worst_z, worst_l = max(worst_z, ez.max()), max(worst_l, el.max())
        assert (ez <= tol).all() and (el <= tol).all(), (c, ez, el)
        ref += vc.grad_mats(n, m, T, z_ref, l_ref)[0]
        cap_z, cap_l = tol * np.abs(z_ref).max(axis=1), tol * np.abs(l_ref).max(axis=1)
        bound += vc.propagated_bound(n, m, T, z_ref, l_ref, cap_z, cap_l)
    print(f"VJP MULTI SOLVE | {s.kernel_name} | {cols} columns | rel err sol {worst_z:.2e} lambda {worst_l:.2e} of {tol:.0e}")
    diff = np.abs(cg.host(grad_mats).astype(vc.LD) - ref)
    ratio = float((diff / np.where(bound > 0, bound, 1)).max())
    print(f"VJP MULTI SOLVE | {s.kernel_name} | {cols} columns | worst |grad_mats - ref| / bound = {ratio:.3f}; "
          f"max |diff| {float(diff.max()):.2e}, max |ref| {float(np.abs(ref).max()):.2e}")
    assert (diff <= bound).all(), ratio
    # and it is the kernel on the very columns it was given
    alone = s.vjp_mats_multi(sol_cols, lam_cols)
    torch.cuda.synchronize()
    assert torch.equal(alone, grad_mats)
    # want_mats=False (d_grad_mats = NULL): no gradient, lambda the same bits
    none, again = s.vjp_multi(mats, sol_cols, g_cols, gains, want_mats=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(again, lam_cols)


@pytest.mark.parametrize("n,m,T,dtype,kwargs,tol,cols", CASES, ids=IDS)
def test_a_failed_problem_gets_zero_gradients(n, m, T, dtype, kwargs, tol, cols):
    from sip_optimal_control_amd import ChainShape, FactorStatus
    s, mats, vecs_cols, g_cols = _setup(n, m, T, dtype, kwargs, cols)
    _, _, status0, gm0, gv0 = _forward_backward(s, mats, vecs_cols, g_cols)
    assert (status0.cpu().numpy() == 0).all()
    bad = mats.clone()
    bad[1, ChainShape(n, m, T).mats_off(T // 2)["delta"] + n - 1] = -1.0
    _, _, status, gm, gv = _forward_backward(s, bad, vecs_cols, g_cols)
    assert status.cpu().numpy().tolist() == [0, int(FactorStatus.INVALID_DELTA), 0, 0, 0]
    assert bool((gv[:, 1] == 0).all()) and bool((gm[1] == 0).all())
    good = [0, 2, 3, 4]
    assert torch.equal(gv[:, good], gv0[:, good]) and torch.equal(gm[good], gm0[good])


@pytest.mark.parametrize("cols", [3, 9])
def test_refined_adjoints_on_the_fp32_plan(cols):
    """refine_iterations=3 on the fp32 (12, 4, 5) plan: float64 gradients, and lambda columns whose KKT residual (the
    right-hand side is g_c) is smaller than the unrefined one's on every problem of every column -- the criterion of
    tests/test_gpu_vjp_solve.py for one column."""
    n, m, T, dtype, kwargs, _ = PLANS[1]
    s, mats, vecs_cols, g_cols = _setup(n, m, T, dtype, kwargs, cols)
    sol_cols, gains, status, gm32, lam32 = _forward_backward(s, mats, vecs_cols, g_cols)
    assert (status.cpu().numpy() == 0).all() and gm32.dtype == torch.float32
    gm64, lam64 = s.vjp_multi(mats, sol_cols, g_cols, gains, refine_iterations=3)
    assert gm64.dtype == torch.float64 and lam64.dtype == torch.float64
    assert tuple(gm64.shape) == (BATCH, s.shape.mats_len) and tuple(lam64.shape) == (cols, BATCH, s.shape.vecs_len)
    g64 = g_cols.double()
    _, refined = s.residual_multi(mats, g64, lam64, want_vector=False)
    _, plain = s.residual_multi(mats, g64, lam32.double(), want_vector=False)
    torch.cuda.synchronize()
    refined, plain = refined.cpu().numpy(), plain.cpu().numpy()
    print(f"VJP MULTI REFINE | {s.kernel_name} | {cols} columns | residual norm of lambda: plain max {plain.max():.2e} "
          f"min {plain.min():.2e}, refined max {refined.max():.2e}")
    assert refined.shape == (cols, BATCH) and (refined < plain).all(), (refined, plain)
    # the float64 gradient is the kernel on float64 columns and the refined lambdas
    ref = np.zeros((BATCH, s.shape.mats_len), dtype=vc.LD)
    mag = np.zeros_like(ref)
    for c in range(cols):
        r, a = vc.grad_mats(n, m, T, cg.host(sol_cols[c]), cg.host(lam64[c]))
        ref, mag = ref + r, mag + a
    assert (np.abs(cg.host(gm64).astype(vc.LD) - ref) <= (2 * cols + 1) * 2.0 ** -53 * mag).all()
    none, lam_only = s.vjp_multi(mats, sol_cols, g_cols, gains, want_mats=False, refine_iterations=3)
    torch.cuda.synchronize()
    assert none is None and torch.equal(lam_only, lam64)

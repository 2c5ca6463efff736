"""sip_lqr_vjp on the GPU (BatchedChainLQR.vjp): the backward pass end to end, batch 3, on synthetic.make_chain_batch
draws, against oracle/dense_kkt.solve.

grad_vecs is the adjoint lambda, K lambda + g = 0: the plan's solve kernel on another right-hand side.  It is held
against the dense solve with (q, c, r) <- g by the criterion the parity test of the same plan applies to `sol`
(tests/test_gpu_chain_parity.py, test_gpu_symmetric_layout.py: fp64, 1e-9; tests/test_gpu_qf32_sweeps.py,
test_gpu_mt16_sweeps.py: fp32, chain_guards.F32_TOL = 1e-4): per problem, max |got - ref| <= TOL max |ref|.  The forward
`sol` is held to the same.

grad_mats is held against the numpy restatement (tests/vjp_cases.py) evaluated on the dense z and lambda.  Derivation of
its bound: the kernel sees z' = z + dz and l' = l + dl with |dz| <= e_z = TOL max |z| and |dl| <= e_l = TOL max |l| per
problem (the two caps above, which the test asserts first).  A term l_a z_b of an entry becomes
(l_a + dl_a)(z_b + dz_b) = l_a z_b + dl_a z_b + l_a dz_b + O(e^2), so to first order it moves by at most
e_l |z_b| + |l_a| e_z; summed over the entry's terms with their weights this is vjp_cases.propagated_bound.  On top of
it the kernel's own rounding on the operands it was given: 3 * 2^-53 * a (+ 2^-24 |.| on an fp32 plan), evaluated on
the device's z' and l'.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import chain_guards as cg
import vjp_cases as vc
from oracle import dense_kkt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BATCH = 3
# (n, m, T, torch dtype name, constructor arguments, criterion of the plan's parity test)
PLANS = [(5, 3, 7, "float64", {}, cg.F64_TOL),
         (12, 4, 5, "float64", {}, cg.F64_TOL),
         (12, 4, 5, "float64", {"symmetric": True}, cg.F64_TOL),
         (12, 4, 5, "float32", {"fused_f32": True, "separate_sweeps": True}, cg.F32_TOL),
         (32, 8, 2, "float32", {"separate_sweeps": True}, cg.F32_TOL)]
IDS = [f"{n}-{m}-{T}-{d}-{'+'.join(k) or 'plain'}" for n, m, T, d, k, _ in PLANS]


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


def _setup(n, m, T, dtype, kwargs, seed_shift=0):
    from sip_optimal_control_amd import BatchedChainLQR
    dt = getattr(torch, dtype)
    s = BatchedChainLQR(n, m, T, BATCH, dtype=dt, **kwargs)
    for opt in ("fused_f32", "separate_sweeps"):
        assert getattr(s, "has_" + opt) == bool(kwargs.get(opt)), (opt, s.kernel_name)
    full_mats, vecs = cg.make(n, m, T, BATCH, seed=4100 + 13 * n + T + seed_shift, dtype=dt)
    gen = torch.Generator(device="cuda:0").manual_seed(77 + n)
    g = torch.randn(BATCH, s.shape.vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(dt)
    return s, full_mats, vecs, g


def _plan_mats(s, full_mats):
    if not s.shape.symmetric:
        return full_mats
    return full_mats[:, torch.from_numpy(s.shape.pack_index()).to("cuda:0")].contiguous()


def _forward_backward(s, mats, vecs, g, **kwargs):
    gains, status = s.factor(mats)
    sol = s.solve(mats, vecs, gains)
    grad_mats, grad_vecs = s.vjp(mats, sol, g, gains, **kwargs)
    torch.cuda.synchronize()
    return sol, gains, status.clone(), grad_mats, grad_vecs


@pytest.mark.parametrize("n,m,T,dtype,kwargs,tol", PLANS, ids=IDS)
def test_backward_pass_against_the_dense_solve(n, m, T, dtype, kwargs, tol):
    s, full_mats, vecs, g = _setup(n, m, T, dtype, kwargs)
    mats = _plan_mats(s, full_mats)
    sol, gains, status, grad_mats, grad_vecs = _forward_backward(s, mats, vecs, g)
    assert (status.cpu().numpy() == 0).all()
    assert grad_mats.dtype == s.dtype and tuple(grad_mats.shape) == (BATCH, s.shape.mats_len)
    symmetric = bool(kwargs.get("symmetric"))
    f32 = dtype == "float32"
    hm = cg.host(full_mats)                                     # the problem the device sees, in float64
    z_ref, l_ref = _dense(n, m, T, hm, cg.host(vecs)), _dense(n, m, T, hm, cg.host(g))
    z, lam = cg.host(sol), cg.host(grad_vecs)
    ez, el = cg.rel_err(z, z_ref), cg.rel_err(lam, l_ref)
    print(f"VJP SOLVE | {s.kernel_name} | rel err sol {ez.max():.2e} lambda {el.max():.2e} of {tol:.0e}")
    assert (ez <= tol).all() and (el <= tol).all(), (ez, el)
    ref, _ = vc.grad_mats(n, m, T, z_ref, l_ref, symmetric=symmetric)
    cap_z, cap_l = tol * np.abs(z_ref).max(axis=1), tol * np.abs(l_ref).max(axis=1)
    on_device, mag = vc.grad_mats(n, m, T, z, lam, symmetric=symmetric)
    bound = vc.propagated_bound(n, m, T, z_ref, l_ref, cap_z, cap_l, symmetric) + vc.kernel_bound(mag, on_device, f32)
    diff = np.abs(cg.host(grad_mats).astype(vc.LD) - ref)
    ratio = float((diff / np.where(bound > 0, bound, 1)).max())
    print(f"VJP SOLVE | {s.kernel_name} | worst |grad_mats - ref| / bound = {ratio:.3f}; "
          f"max |diff| {float(diff.max()):.2e}, max |ref| {float(np.abs(ref).max()):.2e}")
    assert (diff <= bound).all(), ratio
    # and the kernel alone on the very operands it was given: its own bound, nothing propagated
    own = np.abs(cg.host(grad_mats).astype(vc.LD) - on_device)
    assert (own <= vc.kernel_bound(mag, on_device, f32)).all()
    # want_mats=False: lambda alone, the same bits
    none, again = s.vjp(mats, sol, g, gains, want_mats=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(again, grad_vecs)


@pytest.mark.parametrize("n,m,T,dtype,kwargs,tol", PLANS, ids=IDS)
def test_a_failed_problem_gets_zero_gradients(n, m, T, dtype, kwargs, tol):
    from sip_optimal_control_amd import ChainShape, FactorStatus
    s, full_mats, vecs, g = _setup(n, m, T, dtype, kwargs)
    _, _, status0, gm0, gv0 = _forward_backward(s, _plan_mats(s, full_mats), vecs, g)
    assert (status0.cpu().numpy() == 0).all()
    bad = full_mats.clone()
    bad[1, ChainShape(n, m, T).mats_off(T // 2)["delta"] + n - 1] = -1.0
    _, _, status, gm, gv = _forward_backward(s, _plan_mats(s, bad), vecs, g)
    assert status.cpu().numpy().tolist() == [0, int(FactorStatus.INVALID_DELTA), 0]
    assert bool((gv[1] == 0).all()) and bool((gm[1] == 0).all())
    good = [0, 2]
    assert torch.equal(gv[good], gv0[good]) and torch.equal(gm[good], gm0[good])


def test_refined_adjoint_on_the_fp32_plan():
    """refine_iterations=3 on the fp32 (12, 4, 5) plan: float64 gradients, and a lambda whose KKT residual (the
    right-hand side is g) is smaller than the unrefined one's on every problem."""
    n, m, T, dtype, kwargs, _ = PLANS[3]
    s, mats, vecs, g = _setup(n, m, T, dtype, kwargs)
    sol, gains, status, gm32, lam32 = _forward_backward(s, mats, vecs, g)
    assert (status.cpu().numpy() == 0).all() and gm32.dtype == torch.float32
    gm64, lam64 = s.vjp(mats, sol, g, gains, refine_iterations=3)
    assert gm64.dtype == torch.float64 and lam64.dtype == torch.float64
    assert tuple(gm64.shape) == (BATCH, s.shape.mats_len) and tuple(lam64.shape) == (BATCH, s.shape.vecs_len)
    g64 = g.double()
    _, refined = s.residual(mats, g64, lam64, want_vector=False)
    _, plain = s.residual(mats, g64, lam32.double(), want_vector=False)
    torch.cuda.synchronize()
    refined, plain = refined.cpu().numpy(), plain.cpu().numpy()
    print(f"VJP REFINE | {s.kernel_name} | residual norm of lambda: plain {plain} refined {refined}")
    assert (refined < plain).all(), (refined, plain)
    # the float64 gradient is the kernel on float64 sol and the refined lambda
    ref, mag = vc.grad_mats(n, m, T, cg.host(sol), cg.host(lam64))
    assert (np.abs(cg.host(gm64).astype(vc.LD) - ref) <= vc.kernel_bound(mag, ref, False)).all()
    none, lam_only = s.vjp(mats, sol, g, gains, want_mats=False, refine_iterations=3)
    torch.cuda.synchronize()
    assert none is None and torch.equal(lam_only, lam64)

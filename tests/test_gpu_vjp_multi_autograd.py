"""autograd.chain_lqr_solve_multi on the GPU: torch.autograd through solve_multi is BatchedChainLQR.vjp_multi, bit for
bit; it agrees with the sum of chain_lqr_solve gradients over the single columns within the propagated bound;
gradients are produced only for the inputs that ask for them; a factor call between forward and backward is noticed and
the saved problem factored again; the status is not differentiable and there is no second derivative."""
import numpy as np
import pytest

import chain_guards as cg
import vjp_cases as vc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, M, T, BATCH, COLS = 5, 3, 7, 5, 9


def _setup(dtype=torch.float64, seed=0):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(N, M, T, BATCH, dtype=dtype)
    mats, _ = cg.make(N, M, T, BATCH, seed=7200 + seed, dtype=dtype)
    gen = torch.Generator(device="cuda:0").manual_seed(19)
    draw = lambda: torch.randn(COLS, BATCH, s.shape.vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(dtype)
    return s, mats, draw(), draw()


def _by_hand(s, mats, vecs_cols, w, **kwargs):
    gains, _ = s.factor(mats)
    sol_cols = s.solve_multi(mats, vecs_cols, gains)
    grad_mats, grad_vecs_cols = s.vjp_multi(mats, sol_cols, w, gains, **kwargs)
    torch.cuda.synchronize()
    return sol_cols, grad_mats, grad_vecs_cols


def test_autograd_is_the_vjp_multi_bit_for_bit():
    from sip_optimal_control_amd import chain_lqr_solve_multi
    s, mats, vecs_cols, w = _setup()
    sol0, gm0, gv0 = _by_hand(s, mats, vecs_cols, w)
    mats_r, vecs_r = mats.clone().requires_grad_(True), vecs_cols.clone().requires_grad_(True)
    sol, status = chain_lqr_solve_multi(s, mats_r, vecs_r, return_status=True)
    assert torch.equal(sol.detach(), sol0) and sol.requires_grad
    assert status.dtype == torch.int32 and not status.requires_grad and bool((status == 0).all())
    assert status.grad_fn is None                               # non-differentiable: nothing flows back through it
    only_sol = chain_lqr_solve_multi(s, mats_r, vecs_r)
    assert torch.is_tensor(only_sol) and torch.equal(only_sol.detach(), sol0)
    gm, gv = torch.autograd.grad((w * sol).sum(), (mats_r, vecs_r))
    torch.cuda.synchronize()
    assert torch.equal(gm, gm0) and torch.equal(gv, gv0)
    assert tuple(gm.shape) == tuple(mats.shape) and tuple(gv.shape) == tuple(vecs_cols.shape)


def test_the_sum_of_single_column_gradients_agrees():
    """sum_c of chain_lqr_solve gradients on the single columns.  Both routes evaluate the same formulas on device
    solutions and adjoints that are each within F64_TOL of the exact ones (tests/test_gpu_chain_parity.py's criterion),
    so each is within sum_c propagated_bound of the exact gradient; the two are held to ONE such bound of each other,
    half of what that argument allows."""
    from sip_optimal_control_amd import chain_lqr_solve, chain_lqr_solve_multi
    s, mats, vecs_cols, w = _setup()
    mats_r = mats.clone().requires_grad_(True)
    sol = chain_lqr_solve_multi(s, mats_r, vecs_cols)
    (gm,) = torch.autograd.grad((w * sol).sum(), (mats_r,))
    total = torch.zeros_like(gm)
    bound = np.zeros(tuple(gm.shape), dtype=vc.LD)
    for c in range(COLS):
        mats_c, vecs_c = mats.clone().requires_grad_(True), vecs_cols[c].clone().requires_grad_(True)
        sol_c = chain_lqr_solve(s, mats_c, vecs_c)
        g_c, lam_c = torch.autograd.grad((w[c] * sol_c).sum(), (mats_c, vecs_c))
        total += g_c
        z, lam = cg.host(sol_c), cg.host(lam_c)
        bound += vc.propagated_bound(N, M, T, z, lam, cg.F64_TOL * np.abs(z).max(axis=1),
                                     cg.F64_TOL * np.abs(lam).max(axis=1))
    torch.cuda.synchronize()
    diff = np.abs(cg.host(gm).astype(vc.LD) - cg.host(total))
    ratio = float((diff / np.where(bound > 0, bound, 1)).max())
    print(f"VJP MULTI AUTOGRAD | worst |multi - sum of singles| / propagated bound = {ratio:.2e}")
    assert (diff <= bound).all(), ratio


def test_only_the_gradients_that_are_asked_for(monkeypatch):
    from sip_optimal_control_amd import chain_lqr_solve_multi
    s, mats, vecs_cols, w = _setup()
    _, _, gv0 = _by_hand(s, mats, vecs_cols, w)
    calls, returned = [], []
    real = s.vjp_multi

    def spy(*a, **k):
        calls.append(k)
        returned.append(real(*a, **k))
        return returned[-1]

    monkeypatch.setattr(s, "vjp_multi", spy)
    vecs_r = vecs_cols.clone().requires_grad_(True)
    sol = chain_lqr_solve_multi(s, mats, vecs_r)
    (gv,) = torch.autograd.grad((w * sol).sum(), (vecs_r,))
    torch.cuda.synchronize()
    assert calls == [{"want_mats": False}] and returned[0][0] is None     # the kernel was not launched, nothing allocated
    assert torch.equal(gv, gv0)
    # and with only mats asking, vecs_cols gets none
    mats_r = mats.clone().requires_grad_(True)
    sol = chain_lqr_solve_multi(s, mats_r, vecs_cols)
    assert not vecs_cols.requires_grad
    (gm,) = torch.autograd.grad((w * sol).sum(), (mats_r,))
    torch.cuda.synchronize()
    assert calls[-1] == {"want_mats": True} and tuple(gm.shape) == tuple(mats.shape)
    # neither asks: no graph at all
    assert not chain_lqr_solve_multi(s, mats, vecs_cols).requires_grad


def test_a_factor_call_in_between_is_noticed():
    from sip_optimal_control_amd import chain_lqr_solve_multi
    s, mats, vecs_cols, w = _setup()
    other, _ = cg.make(N, M, T, BATCH, seed=7300, dtype=torch.float64)
    grads = []
    for intrude in (False, True):
        mats_r, vecs_r = mats.clone().requires_grad_(True), vecs_cols.clone().requires_grad_(True)
        sol = chain_lqr_solve_multi(s, mats_r, vecs_r)
        generation = s.factor_generation
        if intrude:
            s.factor(other)                                   # overwrites the factor state in the workspace
            assert s.factor_generation == generation + 1
        grads.append(torch.autograd.grad((w * sol).sum(), (mats_r, vecs_r)))
        torch.cuda.synchronize()
        assert s.factor_generation == generation + (2 if intrude else 0)     # factored again, or not at all
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # the stale state would have given something else: the intrusion is not a no-op
    gains, _ = s.factor(mats)
    sol_cols = s.solve_multi(mats, vecs_cols, gains)
    s.factor(other, gains.clone())
    _, stale = s.vjp_multi(mats, sol_cols, w, gains, want_mats=False)
    torch.cuda.synchronize()
    assert not torch.equal(stale, grads[0][1])


def test_double_backward_raises():
    from sip_optimal_control_amd import chain_lqr_solve_multi
    s, mats, vecs_cols, w = _setup()
    mats_r = mats.clone().requires_grad_(True)
    sol = chain_lqr_solve_multi(s, mats_r, vecs_cols)
    (gm,) = torch.autograd.grad((w * sol).sum(), (mats_r,), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gm.sum(), (mats_r,))

"""autograd.chain_lqr_solve on the GPU: torch.autograd through the chain solve is BatchedChainLQR.vjp, bit for bit;
gradients are produced only for the inputs that ask for them; a factor call between forward and backward is noticed and
the saved problem factored again; there is no second derivative."""
import pytest

import chain_guards as cg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, M, T, BATCH = 5, 3, 7, 3


def _setup(dtype=torch.float64, seed=0):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(N, M, T, BATCH, dtype=dtype)
    mats, vecs = cg.make(N, M, T, BATCH, seed=5200 + seed, dtype=dtype)
    gen = torch.Generator(device="cuda:0").manual_seed(9)
    w = torch.randn(BATCH, s.shape.vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(dtype)
    return s, mats, vecs, w


def _by_hand(s, mats, vecs, w, **kwargs):
    gains, _ = s.factor(mats)
    sol = s.solve(mats, vecs, gains)
    grad_mats, grad_vecs = s.vjp(mats, sol, w, gains, **kwargs)
    torch.cuda.synchronize()
    return sol, grad_mats, grad_vecs


def test_autograd_is_the_vjp_bit_for_bit():
    from sip_optimal_control_amd import chain_lqr_solve
    s, mats, vecs, w = _setup()
    sol0, gm0, gv0 = _by_hand(s, mats, vecs, w)
    mats_r, vecs_r = mats.clone().requires_grad_(True), vecs.clone().requires_grad_(True)
    sol, status = chain_lqr_solve(s, mats_r, vecs_r, return_status=True)
    assert torch.equal(sol.detach(), sol0) and sol.requires_grad
    assert status.dtype == torch.int32 and not status.requires_grad and bool((status == 0).all())
    gm, gv = torch.autograd.grad((w * sol).sum(), (mats_r, vecs_r))
    torch.cuda.synchronize()
    assert torch.equal(gm, gm0) and torch.equal(gv, gv0)


def test_only_the_gradients_that_are_asked_for(monkeypatch):
    from sip_optimal_control_amd import chain_lqr_solve
    s, mats, vecs, w = _setup()
    _, _, gv0 = _by_hand(s, mats, vecs, w)
    calls, returned = [], []
    real = s.vjp

    def spy(*a, **k):
        calls.append(k)
        returned.append(real(*a, **k))
        return returned[-1]

    monkeypatch.setattr(s, "vjp", spy)
    vecs_r = vecs.clone().requires_grad_(True)
    sol = chain_lqr_solve(s, mats, vecs_r)
    (gv,) = torch.autograd.grad((w * sol).sum(), (vecs_r,))
    torch.cuda.synchronize()
    assert calls == [{"want_mats": False}] and returned[0][0] is None     # the kernel was not launched, nothing allocated
    assert torch.equal(gv, gv0)
    # and with only mats asking, vecs gets none
    mats_r = mats.clone().requires_grad_(True)
    sol = chain_lqr_solve(s, mats_r, vecs)
    assert not vecs.requires_grad
    (gm,) = torch.autograd.grad((w * sol).sum(), (mats_r,))
    torch.cuda.synchronize()
    assert calls[-1] == {"want_mats": True} and tuple(gm.shape) == tuple(mats.shape)


def test_a_factor_call_in_between_is_noticed():
    from sip_optimal_control_amd import chain_lqr_solve
    s, mats, vecs, w = _setup()
    other, _ = cg.make(N, M, T, BATCH, seed=5300, dtype=torch.float64)
    grads = []
    for intrude in (False, True):
        mats_r, vecs_r = mats.clone().requires_grad_(True), vecs.clone().requires_grad_(True)
        sol = chain_lqr_solve(s, mats_r, vecs_r)
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
    sol = s.solve(mats, vecs, gains)
    s.factor(other, gains.clone())
    _, stale = s.vjp(mats, sol, w, gains, want_mats=False)
    torch.cuda.synchronize()
    assert not torch.equal(stale, grads[0][1])


def test_every_factor_call_bumps_the_generation():
    s, mats, vecs, _ = _setup()
    g0 = s.factor_generation
    s.factor_solve(mats, vecs)
    assert s.factor_generation == g0 + 1
    s.factor(mats)
    assert s.factor_generation == g0 + 2
    if s.has_split:
        qmr, ab = s.split_inputs(mats)
        s.factor_solve_split(qmr, ab, vecs)
        assert s.factor_generation == g0 + 3
    torch.cuda.synchronize()


def test_double_backward_raises():
    from sip_optimal_control_amd import chain_lqr_solve
    s, mats, vecs, w = _setup()
    mats_r = mats.clone().requires_grad_(True)
    sol = chain_lqr_solve(s, mats_r, vecs)
    (gm,) = torch.autograd.grad((w * sol).sum(), (mats_r,), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gm.sum(), (mats_r,))

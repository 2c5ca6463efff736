"""autograd.tree_lqr_solve on the GPU: torch.autograd through the tree solve is BatchedTreeLQR.vjp, bit for bit; a
gradient is produced only where the input asks for one; a pack() or a factor*() between forward and backward is noticed
and the saved input factored again; the status is not differentiable; a failed problem gets zero gradient rows; there is
no second derivative."""
import numpy as np
import pytest

import full_batch_problems as fb
import hard_inputs as hi
import tree_vjp_cases as tv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BATCH = 3


def _setup(seed=0):
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    topo = tv.topologies()["random<9,3>"][0]
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=BATCH)
    maps = fb.PlanMaps(s, topo)
    rng = np.random.default_rng(hi._seed("tree vjp autograd", seed))
    blocks = fb.make_blocks(topo, BATCH, rng, "random")
    nodes, edges = fb.to_oracle(topo, blocks)
    arena = torch.from_numpy(maps.pack_input(s, nodes, edges)).to("cuda:0")
    w = torch.from_numpy(rng.normal(size=(BATCH, s.out_len))).to("cuda:0")
    return s, topo, blocks, arena, w


def _by_hand(s, arena, w, **kwargs):
    s.input.copy_(arena)
    status = s.factor_fused().clone()
    out = s.solve_fused().clone()
    grad_input, adj = s.vjp(w, output=out, **kwargs)
    torch.cuda.synchronize()
    return out, status, grad_input, adj


def test_autograd_is_the_vjp_bit_for_bit():
    from sip_optimal_control_amd import tree_lqr_solve
    s, _, _, arena, w = _setup()
    out0, status0, gi0, adj0 = _by_hand(s, arena, w)
    assert bool((status0 == 0).all())
    x = arena.clone().requires_grad_(True)
    out, status = tree_lqr_solve(s, x, return_status=True)
    assert torch.equal(out.detach(), out0) and out.requires_grad
    assert status.dtype == torch.int32 and not status.requires_grad and torch.equal(status, status0)
    assert out.data_ptr() != s.output.data_ptr() and status.data_ptr() != s.status.data_ptr()      # clones
    (gi,) = torch.autograd.grad((w * out).sum(), (x,))
    torch.cuda.synchronize()
    assert tuple(gi.shape) == tuple(x.shape) and torch.equal(gi, gi0)
    # the q, c, r slots of the gradient are lambda itself
    copy = torch.from_numpy(tv.grad_input(tv.topologies()["random<9,3>"][0], np.zeros((1, s.out_len)),
                                          np.arange(1.0, s.out_len + 1)[None], dt=np.float64)[0][0]).to("cuda:0")
    slots = copy != 0                                         # where the gradient of a probe lambda = 1, 2, ... is a copy
    assert torch.equal(gi[:, slots], adj0[:, (copy[slots] - 1).long()])
    assert tree_lqr_solve(s, arena).requires_grad is False                                         # return_status=False


def test_only_the_gradient_that_is_asked_for(monkeypatch):
    from sip_optimal_control_amd import tree_lqr_solve
    s, _, _, arena, w = _setup()
    calls = []
    real = s.vjp

    def spy(*a, **k):
        calls.append(k)
        return real(*a, **k)

    monkeypatch.setattr(s, "vjp", spy)
    out = tree_lqr_solve(s, arena)                            # the input asks for nothing: no graph, no backward pass
    assert not out.requires_grad and out.grad_fn is None
    x = arena.clone().requires_grad_(True)
    out = tree_lqr_solve(s, x)
    other = torch.ones(1, dtype=torch.float64, device="cuda:0", requires_grad=True)
    (g_other,) = torch.autograd.grad((other * out.detach()).sum(), (other,))                       # not through the solve
    assert calls == []
    (gi,) = torch.autograd.grad((w * out).sum(), (x,))
    torch.cuda.synchronize()
    assert len(calls) == 1 and calls[0].get("want_input") is True and tuple(gi.shape) == tuple(x.shape)


def test_a_pack_or_a_factor_call_in_between_is_noticed():
    from sip_optimal_control_amd import tree_lqr_solve
    s, topo, blocks, arena, w = _setup()
    _, _, other_blocks, other, _ = _setup(seed=1)
    intrusions = {
        "none": lambda: None,
        "pack": lambda: s.pack([fb.problem(other_blocks, b) for b in range(BATCH)]),
        "factor": lambda: (s.input.copy_(other), s.factor()),
        "factor_fused": lambda: (s.input.copy_(other), s.factor_fused()),
        "factor_solve": lambda: (s.input.copy_(other), s.factor_solve(workspace=True)),
    }
    grads = {}
    for name, intrude in intrusions.items():
        x = arena.clone().requires_grad_(True)
        out = tree_lqr_solve(s, x)
        generation = s.factor_generation
        intrude()
        assert s.factor_generation == generation + (0 if name == "none" else 1), name
        (grads[name],) = torch.autograd.grad((w * out).sum(), (x,))
        torch.cuda.synchronize()
        # factored again (one more bump), or not at all
        assert s.factor_generation == generation + (0 if name == "none" else 2), name
        assert torch.equal(s.input, arena), name
    for name in intrusions:
        assert torch.equal(grads[name], grads["none"]), name
    # the foreign state would have given something else: the intrusion is not a no-op
    out0, _, _, adj0 = _by_hand(s, arena, w)
    s.input.copy_(other)
    s.factor_fused()
    _, stale = s.vjp(w, output=out0, want_input=False)
    torch.cuda.synchronize()
    assert not torch.equal(stale, adj0)


def test_every_factor_call_and_pack_bump_the_generation():
    s, _, blocks, arena, _ = _setup()
    g0 = s.factor_generation
    s.pack([fb.problem(blocks, b) for b in range(BATCH)])
    assert s.factor_generation == g0 + 1
    s.factor()
    assert s.factor_generation == g0 + 2
    s.factor_fused()
    assert s.factor_generation == g0 + 3
    s.factor_solve()
    assert s.factor_generation == g0 + 4
    s.factor_solve(workspace=True)
    assert s.factor_generation == g0 + 5
    s.solve(), s.solve_fused()
    assert s.factor_generation == g0 + 5                      # a solve is not a factor call
    torch.cuda.synchronize()


def test_a_failed_problem_gets_zero_gradient_rows():
    from sip_optimal_control_amd import FactorStatus, tree_lqr_solve
    s, topo, _, arena, w = _setup()
    x = arena.clone().requires_grad_(True)
    out = tree_lqr_solve(s, x)
    (good,) = torch.autograd.grad((w * out).sum(), (x,))
    node = next(i for i, n in enumerate(topo.sd) if n >= 3 and i > 0)
    bad = arena.clone()
    bad[1, s.offset(0, 0, node) + topo.sd[node] ** 2 + 2 * topo.sd[node] + 2] = -1.0              # delta[node][2]
    x = bad.clone().requires_grad_(True)
    out, status = tree_lqr_solve(s, x, return_status=True)
    (gi,) = torch.autograd.grad((w * out).sum(), (x,))
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, int(FactorStatus.INVALID_DELTA), 0]
    assert bool((gi[1] == 0).all()) and torch.equal(gi[[0, 2]], good[[0, 2]]) and bool((good[1] != 0).any())


def test_double_backward_raises():
    from sip_optimal_control_amd import tree_lqr_solve
    s, _, _, arena, w = _setup()
    x = arena.clone().requires_grad_(True)
    out = tree_lqr_solve(s, x)
    (gi,) = torch.autograd.grad((w * out).sum(), (x,), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gi.sum(), (x,))

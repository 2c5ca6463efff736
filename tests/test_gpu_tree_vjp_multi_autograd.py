"""autograd.tree_lqr_solve_multi on the GPU: torch.autograd through the tree's solve_multi is BatchedTreeLQR.vjp_multi,
bit for bit; the gradient of rhs_cols is adj_cols and the q, c, r slots of the input's gradient are zero; a gradient is
produced only where an input asks for one; a pack() or a factor*() between forward and backward is noticed and the saved
input factored again; the status is not differentiable; and a 2-column call whose second column copies the first, with
the loss on the first only, agrees with tree_lqr_solve off the q, c, r slots."""
import numpy as np
import pytest

import full_batch_problems as fb
import hard_inputs as hi
import tree_vjp_cases as tv
import tree_vjp_multi_cases as tm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BATCH = 3
COLS = 3


def _setup(seed=0):
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    topo = tv.topologies()["random<9,3>"][0]
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=BATCH)
    maps = fb.PlanMaps(s, topo)
    rng = np.random.default_rng(hi._seed("tree vjp multi autograd", seed))
    blocks = fb.make_blocks(topo, BATCH, rng, "random")
    nodes, edges = fb.to_oracle(topo, blocks)
    arena = torch.from_numpy(maps.pack_input(s, nodes, edges)).to("cuda:0")
    rhs = torch.from_numpy(rng.normal(size=(COLS, BATCH, s.out_len))).to("cuda:0")
    w = torch.from_numpy(rng.normal(size=(COLS, BATCH, s.out_len))).to("cuda:0")
    return s, topo, blocks, arena, rhs, w


def _by_hand(s, arena, rhs, w, **kwargs):
    s.input.copy_(arena)
    status = s.factor_fused().clone()
    out = s.solve_multi(rhs)
    grad_input, adj = s.vjp_multi(w, out, **kwargs)
    torch.cuda.synchronize()
    return out, status, grad_input, adj


def _copy_slots(topo):
    return torch.from_numpy(tm.grad_input_multi(topo, np.zeros((0, 1, topo.layout.sol_len)),
                                                np.zeros((0, 1, topo.layout.sol_len)))[2]).to("cuda:0")


def test_autograd_is_the_vjp_multi_bit_for_bit():
    from sip_optimal_control_amd import tree_lqr_solve_multi
    s, topo, _, arena, rhs, w = _setup()
    out0, status0, gi0, adj0 = _by_hand(s, arena, rhs, w)
    assert bool((status0 == 0).all())
    x, r = arena.clone().requires_grad_(True), rhs.clone().requires_grad_(True)
    out, status = tree_lqr_solve_multi(s, x, r, return_status=True)
    assert torch.equal(out.detach(), out0) and out.requires_grad and tuple(out.shape) == (COLS, BATCH, s.out_len)
    assert status.dtype == torch.int32 and not status.requires_grad and torch.equal(status, status0)
    assert status.data_ptr() != s.status.data_ptr()                                                # a clone
    gi, gr = torch.autograd.grad((w * out).sum(), (x, r))
    torch.cuda.synchronize()
    assert tuple(gi.shape) == tuple(x.shape) and torch.equal(gi, gi0)
    assert tuple(gr.shape) == tuple(r.shape) and torch.equal(gr, adj0)                             # dL/d(rhs_cols) = adj_cols
    slots = _copy_slots(topo)
    assert int(slots.sum()) == 2 * sum(topo.sd) + sum(topo.cd)
    assert bool((gi[:, slots] == 0).all()) and bool((gi[:, ~slots] != 0).any())                    # q, c, r are not read
    assert tree_lqr_solve_multi(s, arena, rhs).requires_grad is False                              # return_status=False


def test_only_the_gradients_that_are_asked_for(monkeypatch):
    from sip_optimal_control_amd import tree_lqr_solve_multi
    s, _, _, arena, rhs, w = _setup()
    _, _, gi0, adj0 = _by_hand(s, arena, rhs, w)
    calls = []
    real = s.vjp_multi

    def spy(*a, **k):
        calls.append(k)
        return real(*a, **k)

    monkeypatch.setattr(s, "vjp_multi", spy)
    out = tree_lqr_solve_multi(s, arena, rhs)                 # nothing asks for a gradient: no graph, no backward pass
    assert not out.requires_grad and out.grad_fn is None
    x, r = arena.clone().requires_grad_(True), rhs.clone().requires_grad_(True)
    out = tree_lqr_solve_multi(s, x, rhs)                     # the input alone
    (gi,) = torch.autograd.grad((w * out).sum(), (x,))
    assert len(calls) == 1 and calls[0].get("want_input") is True and torch.equal(gi, gi0)
    out = tree_lqr_solve_multi(s, arena, r)                   # the right-hand sides alone: the kernel is not launched
    (gr,) = torch.autograd.grad((w * out).sum(), (r,))
    torch.cuda.synchronize()
    assert len(calls) == 2 and calls[1].get("want_input") is False and torch.equal(gr, adj0)
    out = tree_lqr_solve_multi(s, x, r)
    other = torch.ones(1, dtype=torch.float64, device="cuda:0", requires_grad=True)
    (g_other,) = torch.autograd.grad((other * out.detach()).sum(), (other,))                       # not through the solve
    assert len(calls) == 2


def test_a_pack_or_a_factor_call_in_between_is_noticed():
    from sip_optimal_control_amd import tree_lqr_solve_multi
    s, topo, blocks, arena, rhs, w = _setup()
    _, _, other_blocks, other, _, _ = _setup(seed=1)
    intrusions = {
        "none": lambda: None,
        "pack": lambda: s.pack([fb.problem(other_blocks, b) for b in range(BATCH)]),
        "factor": lambda: (s.input.copy_(other), s.factor()),
        "factor_fused": lambda: (s.input.copy_(other), s.factor_fused()),
        "factor_solve": lambda: (s.input.copy_(other), s.factor_solve(workspace=True)),
    }
    grads = {}
    for name, intrude in intrusions.items():
        x, r = arena.clone().requires_grad_(True), rhs.clone().requires_grad_(True)
        out = tree_lqr_solve_multi(s, x, r)
        generation = s.factor_generation
        intrude()
        assert s.factor_generation == generation + (0 if name == "none" else 1), name
        grads[name] = torch.autograd.grad((w * out).sum(), (x, r))
        torch.cuda.synchronize()
        # factored again (one more bump), or not at all
        assert s.factor_generation == generation + (0 if name == "none" else 2), name
        assert torch.equal(s.input, arena), name
    for name in intrusions:
        assert torch.equal(grads[name][0], grads["none"][0]) and torch.equal(grads[name][1], grads["none"][1]), name
    # the foreign state would have given something else: the intrusion is not a no-op
    out0, _, _, adj0 = _by_hand(s, arena, rhs, w)
    s.input.copy_(other)
    s.factor_fused()
    _, stale = s.vjp_multi(w, out0, want_input=False)
    torch.cuda.synchronize()
    assert not torch.equal(stale, adj0)


def test_a_copied_column_without_loss_against_the_single_solve():
    """Two columns, the second a copy of the first, the loss on the first only: the adjoint of the second column is
    exactly zero, so its terms add +-0 and the gradient is the one-column gradient of tree_lqr_solve with the arena's
    q, c, r set to that column -- off the q, c, r slots.  Bound: the kernel's for two columns, (2 * 2 + 1) 2^-53 a, plus
    what the operands of the two routes may differ by -- z comes from solve_multi here and from solve_fused there, each
    within 1e-10 max(1, max |z|) of the other (the criterion of the solve tests, asserted first; likewise lambda) --
    propagated to first order by tree_vjp_cases.propagated_bound.  Both gradients are held to that bound around the
    formula, so to twice it around each other; the figures and whether the bits agree are printed."""
    from sip_optimal_control_amd import tree_lqr_solve, tree_lqr_solve_multi
    s, topo, _, arena, rhs, w = _setup()
    L = s.out_len
    two = torch.stack([rhs[0], rhs[0]]).contiguous().requires_grad_(True)
    x = arena.clone().requires_grad_(True)
    out, status = tree_lqr_solve_multi(s, x, two, return_status=True)
    assert torch.equal(out[0], out[1]) and bool((status == 0).all())
    gi, adj_m = torch.autograd.grad((w[0] * out[0]).sum(), (x, two))
    torch.cuda.synchronize()
    assert bool((adj_m[1] == 0).all()) and bool((adj_m[0] != 0).any())
    # the same problem through the one-column solve: the column as q | c | r of the arena
    single = arena.clone()
    probe = tv.grad_input(topo, np.zeros((1, L)), np.arange(1.0, L + 1)[None], dt=np.float64)[0][0]
    slots = torch.from_numpy(probe != 0).to("cuda:0")                                    # the q, c, r slots ...
    place = torch.from_numpy(probe[probe != 0] - 1).long().to("cuda:0")                  # ... and where in z each sits
    single[:, slots] = rhs[0][:, place]
    y = single.clone().requires_grad_(True)
    out1 = tree_lqr_solve(s, y)
    (g1,) = torch.autograd.grad((w[0] * out1).sum(), (y,))
    _, adj1 = s.vjp(w[0].contiguous(), output=out1.detach(), want_input=False)
    torch.cuda.synchronize()
    z, lam = out1.detach().cpu().numpy(), adj1.cpu().numpy()
    zm, lm = out[0].detach().cpu().numpy(), adj_m[0].cpu().numpy()
    cap_z = 1e-10 * np.maximum(1.0, np.abs(z).max(axis=1))                               # the criterion of the solve tests
    cap_l = 1e-10 * np.maximum(1.0, np.abs(lam).max(axis=1))
    assert (np.abs(zm - z).max(axis=1) <= cap_z).all() and (np.abs(lm - lam).max(axis=1) <= cap_l).all()
    ref, mag, copy = tm.grad_input_multi(topo, np.stack([z, z]), np.stack([lam, np.zeros_like(lam)]))
    bound = tm.kernel_bound(mag, 2) * (1 + 1e-9) + tv.propagated_bound(topo, z, lam, cap_z, cap_l)
    keep = ~copy
    got, want = gi.cpu().numpy(), g1.cpu().numpy()
    d_ref, d_single = np.abs(got.astype(tv.LD) - ref), np.abs(got.astype(tv.LD) - want)
    print(f"TREE VJP MULTI AUTOGRAD | copied column | worst |multi - formula| / bound "
          f"{float((d_ref / np.where(bound > 0, bound, 1))[:, keep].max()):.2e}, |multi - single| / bound "
          f"{float((d_single / np.where(bound > 0, bound, 1))[:, keep].max()):.2e}; bits agree: "
          f"{got[:, keep].tobytes() == want[:, keep].tobytes()}")
    assert (d_ref[:, keep] <= bound[:, keep]).all()
    assert (d_single[:, keep] <= 2 * bound[:, keep]).all()                               # each within `bound` of the formula
    assert (got[:, copy] == 0).all() and (want[:, copy] != 0).any()                      # there the single one holds lambda

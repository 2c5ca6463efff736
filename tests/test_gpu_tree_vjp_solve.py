"""sip_lqr_tree_vjp on the GPU (BatchedTreeLQR.vjp): the backward pass end to end, batch 3, on
full_batch_problems.make_blocks draws, against oracle/dense_kkt.solve -- on the fused size-class kernels and on the
general engine (SIP_LQR_TREE=general), after each of factor(), factor_fused() and factor_solve(workspace=True).

adj is the adjoint lambda, K lambda + g = 0: the plan's one-column solve on another right-hand side.  It and the forward
output are held against the dense solve (with (q, c, r) <- g for lambda) by the criterion of tests/test_gpu_tree_multi.py:
|got - ref| <= 1e-10 max(1, max |ref|), block by block (x_i, y_i, u_e), which is no wider than the same with the
problem's largest block.

grad_input is held against the numpy restatement (tests/tree_vjp_cases.py) evaluated on the dense z and lambda.
Derivation of its bound: the kernel sees z' = z + dz and l' = l + dl with |dz| <= e_z = 1e-10 max(1, max |z|) and
|dl| <= e_l = 1e-10 max(1, max |l|) per problem (the caps above, which the test asserts first).  A term l_a z_b of an
entry becomes l_a z_b + dl_a z_b + l_a dz_b + O(e^2), so to first order it moves by at most e_l |z_b| + |l_a| e_z; summed
over the entry's terms with their weights this is tree_vjp_cases.propagated_bound (a copy moves by e_l).  On top of it
the kernel's own rounding on the operands it was given: 3 * 2^-53 * a, evaluated on the device's z' and l'.  Every
figure is printed before it is asserted."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import full_batch_problems as fb
import hard_inputs as hi
import tree_vjp_cases as tv
from oracle import dense_kkt, oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BATCH = 3
TOL = 1e-10
INVALID = -1
TOPOLOGIES = tv.topologies()
NAMES = ["five_node", "single_node", "edge_m0", "node_n0", "random<9,3>", "random<15,8>", "general<17,9>"]
FACTORS = ["factor", "factor_fused", "factor_solve_workspace"]


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _plan(topo, general=False, batch=BATCH):
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    with _env(**({"SIP_LQR_TREE": "general"} if general else {})):
        s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    maps = fb.PlanMaps(s, topo)
    assert np.array_equal(maps.sol_idx, np.arange(topo.layout.sol_len))
    assert np.array_equal(maps.input_idx, np.arange(tv.input_len(topo)))
    return s, maps


def _row(topo, x, u, y):
    out = np.zeros(topo.layout.sol_len)
    vx, vy, vu = tv.views(topo, out[None])
    for dst, src in zip(vx + vy + vu, list(x) + list(y) + list(u)):
        dst[0, :] = src
    return out


def _dense(topo, blocks, rhs=None):
    """[B, sol_len]: dense_kkt.solve of every problem; rhs [B, sol_len]: in place of q, c, r."""
    B = blocks["Q"][0].shape[0]
    out = []
    for b in range(B):
        prob = fb.problem(blocks, b)
        if rhs is not None:
            gx, gy, gu = tv.views(topo, rhs[b:b + 1])
            prob = dict(prob, q=[v[0] for v in gx], c=[v[0] for v in gy], r=[v[0] for v in gu])
        out.append(_row(topo, *dense_kkt.solve(topo.parents, topo.children, topo.sd, topo.cd, prob)))
    return np.stack(out)


_DRAWS = {}


def _draw(name):
    """(topo, blocks, g, z_ref, l_ref), computed once and read-only."""
    if name not in _DRAWS:
        topo = TOPOLOGIES[name][0]
        rng = np.random.default_rng(hi._seed("tree vjp solve", name))
        blocks = fb.make_blocks(topo, BATCH, rng, "random")
        g = rng.normal(size=(BATCH, topo.layout.sol_len))
        z_ref, l_ref = _dense(topo, blocks), _dense(topo, blocks, g)
        for a in (g, z_ref, l_ref):
            a.setflags(write=False)
        _DRAWS[name] = (topo, blocks, g, z_ref, l_ref)
    return _DRAWS[name]


def _load(s, maps, topo, blocks):
    nodes, edges = fb.to_oracle(topo, blocks)
    s.input.copy_(torch.from_numpy(maps.pack_input(s, nodes, edges)))


def _dev(a):
    a = np.asarray(a, dtype=np.float64)
    if a.shape[-1] == 0:                                      # an empty arena is one unused scalar wide
        a = np.zeros(a.shape[:-1] + (1,))
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _forward(s, how):
    """Factor state in `work` and the solution in `output`, by one of the three factor entry points."""
    if how == "factor":
        status = s.factor()
        s.solve()
    elif how == "factor_fused":
        status = s.factor_fused()
        s.solve_fused()
    else:
        _, status = s.factor_solve(workspace=True)
    return status


@pytest.mark.parametrize("general", [False, True], ids=["size_class", "general_engine"])
@pytest.mark.parametrize("name", NAMES)
def test_backward_pass_against_the_dense_solve(name, general):
    topo, blocks, g, z_ref, l_ref = _draw(name)
    L, Lin = topo.layout.sol_len, tv.input_len(topo)
    s, maps = _plan(topo, general)
    if general or TOPOLOGIES[name][2] == "tree_generic":
        assert s.multi_kernel_name.startswith("tree_generic"), s.multi_kernel_name
    elif TOPOLOGIES[name][2].startswith("tree_factor_solve_qw16"):
        assert s.multi_kernel_name.startswith("tree_solve_mrhs_qw16"), s.multi_kernel_name
    assert s.vjp_kernel_name == tv.STAGED
    ref, _, _ = tv.grad_input(topo, z_ref, l_ref)
    cap_z = TOL * np.maximum(1.0, np.abs(z_ref).max(axis=1, initial=0.0))
    cap_l = TOL * np.maximum(1.0, np.abs(l_ref).max(axis=1, initial=0.0))
    dg = _dev(g)
    for how in FACTORS:
        s.work.zero_(), s.output.zero_()
        _load(s, maps, topo, blocks)
        status = _forward(s, how)
        work_before = s.work.clone()
        grad_input, adj = s.vjp(dg)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all(), (how, status)
        assert torch.equal(s.work, work_before), (how, "d_work was written")
        assert tuple(grad_input.shape) == (BATCH, max(1, Lin)) and tuple(adj.shape) == (BATCH, max(1, L))
        z, lam = s.output.cpu().numpy()[:, :L], adj.cpu().numpy()[:, :L]
        ez, el = fb.block_rel_err(z, z_ref, maps.sol_blocks), fb.block_rel_err(lam, l_ref, maps.sol_blocks)
        print(f"TREE VJP SOLVE | {name} {s.multi_kernel_name} after {how} | block rel err output {ez.max():.2e} "
              f"lambda {el.max():.2e} of {TOL:.0e}")
        assert (ez <= TOL).all() and (el <= TOL).all(), (how, ez, el)
        assert (np.abs(z - z_ref).max(axis=1, initial=0.0) <= cap_z).all()
        assert (np.abs(lam - l_ref).max(axis=1, initial=0.0) <= cap_l).all()
        on_device, mag, copy = tv.grad_input(topo, z, lam)
        bound = tv.propagated_bound(topo, z_ref, l_ref, cap_z, cap_l) + tv.kernel_bound(mag)
        got = grad_input.cpu().numpy()[:, :Lin]
        diff = np.abs(got.astype(tv.LD) - ref)
        share = float((diff / np.where(bound > 0, bound, 1)).max(initial=0.0))
        print(f"TREE VJP SOLVE | {name} after {how} | worst |grad_input - ref| / bound = {share:.2e}; max |diff| "
              f"{float(diff.max(initial=0.0)):.2e}, max |ref| {float(np.abs(ref).max(initial=0.0)):.2e}")
        assert (diff <= bound).all(), (how, share)
        # and the kernel alone on the very operands it was given: its own bound, nothing propagated
        own = np.abs(got.astype(tv.LD) - on_device)
        assert (own <= tv.kernel_bound(mag)).all() and (own[:, copy] == 0).all()
        # want_input=False: lambda alone, the same bits
        none, again = s.vjp(dg, want_input=False)
        torch.cuda.synchronize()
        assert none is None and torch.equal(again, adj)


@pytest.mark.parametrize("general", [False, True], ids=["size_class", "general_engine"])
def test_a_failed_problem_gets_zero_gradients(general):
    from sip_optimal_control_amd import FactorStatus
    topo, blocks, g, _, _ = _draw("random<9,3>")
    bad = {k: [a.copy() for a in v] for k, v in blocks.items()}
    node = next(i for i, n in enumerate(topo.sd) if n >= 3 and i > 0)
    bad["delta"][node][1, 2] = -1.0
    nodes, edges = fb.to_oracle(topo, bad)
    _, _, cpu_status = oracle.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, nodes, edges)
    want = [0, int(FactorStatus.INVALID_DELTA), 0]
    assert cpu_status.tolist() == want                        # on the CPU oracle only that problem fails
    s, maps = _plan(topo, general)
    dg = _dev(g)
    _load(s, maps, topo, blocks)
    _forward(s, "factor_fused")
    gi0, adj0 = s.vjp(dg)
    gi0, adj0 = gi0.clone(), adj0.clone()
    _load(s, maps, topo, bad)
    status = _forward(s, "factor_fused")
    gi, adj = s.vjp(dg)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == want
    assert bool((adj[1] == 0).all()) and bool((gi[1] == 0).all())
    good = [0, 2]
    assert torch.equal(adj[good], adj0[good]) and torch.equal(gi[good], gi0[good])
    assert bool((adj0[1] != 0).any()) and bool((gi0[1] != 0).any())


@pytest.mark.parametrize("dims", hi.TREES, ids=lambda d: "<%d,%d>" % d)
def test_refined_adjoint_on_the_smallest_deltas(dims):
    """refine_iterations=2 on the delta[1e-9,1e-7] cell: lambda is what refine() gives on g from a zero iterate, its
    residual norms by round do not increase, and the result's is below the unrefined lambda's on every problem."""
    cell = hi.tree_cell(*dims, "delta[1e-9,1e-7]")
    topo, L = cell.topo, cell.topo.layout.sol_len
    s, maps = _plan(topo, batch=hi.BATCH)
    s.input.copy_(torch.from_numpy(maps.pack_input(s, cell.nodes, cell.edges)))
    status = s.factor_fused()
    s.solve_fused()
    g = _dev(np.random.default_rng(hi._seed("tree vjp refine", dims)).normal(size=(hi.BATCH, L)))
    gi0, lam0 = s.vjp(g)
    gi2, lam2 = s.vjp(g, refine_iterations=2)
    by_hand, norms = s.refine(iterations=2, rhs=g, output=torch.zeros_like(lam2))
    _, plain = s.residual(lam0, rhs=g, want_vector=False)
    _, refined = s.residual(lam2, rhs=g, want_vector=False)
    none, lam_only = s.vjp(g, want_input=False, refine_iterations=2)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    norms, plain, refined = norms.cpu().numpy(), plain.cpu().numpy(), refined.cpu().numpy()
    print(f"TREE VJP REFINE | <{dims[0]},{dims[1]}> | residual norm of lambda by round {norms.max(axis=1)} | plain "
          f"{plain} refined {refined}")
    assert torch.equal(by_hand, lam2) and none is None and torch.equal(lam_only, lam2)
    assert (norms[1:] <= norms[:-1]).all(), norms
    np.testing.assert_array_equal(norms[-1], refined)
    assert (refined < plain).all(), (refined, plain)
    # the gradient is the kernel on the output and the refined lambda
    z = s.output.cpu().numpy()[:, :L]
    ref, mag, copy = tv.grad_input(topo, z, lam2.cpu().numpy()[:, :L])
    assert (np.abs(gi2.cpu().numpy().astype(tv.LD) - ref) <= tv.kernel_bound(mag)).all()


@pytest.mark.parametrize("name,general,batch", [("random<9,3>", False, 3), ("random<9,3>", False, 4096),
                                                ("general<17,9>", False, 5), ("random<15,8>", True, 7),
                                                ("single_node", False, 3)])
def test_scratch_bytes_is_what_the_header_documents(name, general, batch):
    s, _ = _plan(TOPOLOGIES[name][0], general, batch)
    lib = s._lib
    want = int(lib.sip_lqr_tree_solve_multi_scratch_bytes(s._plan, 1))
    assert int(lib.sip_lqr_tree_vjp_scratch_bytes(s._plan)) == want and want > 0
    assert int(lib.sip_lqr_tree_vjp_scratch_bytes(None)) == 0


def test_every_misuse_on_a_valid_plan_is_an_invalid_argument():
    topo, blocks, g, _, _ = _draw("random<9,3>")
    s, maps = _plan(topo)
    _load(s, maps, topo, blocks)
    _forward(s, "factor_fused")
    dg = _dev(g)
    grad, adj = s.vjp(dg)                                                    # sizes the scratch
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ker_args = dict(plan=s._plan, output=P(s.output), adj=P(adj), status=P(s.status), grad=P(grad), stream=None)
    vjp_args = dict(plan=s._plan, input=P(s.input), work=P(s.work), output=P(s.output), gout=P(dg), status=P(s.status),
                    adj=P(adj), grad=P(grad), scratch=P(s._multi_scratch), stream=None)
    ker = lambda **kw: s._lib.sip_lqr_tree_vjp_input(*{**ker_args, **kw}.values())
    vjp = lambda **kw: s._lib.sip_lqr_tree_vjp(*{**vjp_args, **kw}.values())
    misuse = {"kernel plan": ker(plan=None), "kernel output": ker(output=None), "kernel adj": ker(adj=None),
              "kernel grad": ker(grad=None), "vjp plan": vjp(plan=None), "vjp input": vjp(input=None),
              "vjp work": vjp(work=None), "vjp output with grad_input": vjp(output=None), "vjp gout": vjp(gout=None),
              "vjp status": vjp(status=None), "vjp adj": vjp(adj=None), "vjp scratch": vjp(scratch=None)}
    for what, rc in misuse.items():
        assert rc == INVALID, (what, rc)
    # and the well-formed calls run: the optional pointers left out too
    assert ker() == 0 and ker(status=None) == 0 and vjp() == 0 and vjp(grad=None) == 0
    assert vjp(grad=None, output=None) == 0
    torch.cuda.synchronize()

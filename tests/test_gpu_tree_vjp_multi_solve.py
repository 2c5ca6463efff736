"""sip_lqr_tree_vjp_multi on the GPU (BatchedTreeLQR.vjp_multi): the backward pass of solve_multi end to end, batch 3,
3 columns with independent right-hand sides and loss gradients, on full_batch_problems.make_blocks draws, against
oracle/dense_kkt.solve -- on the fused size-class kernels and on the general engine (SIP_LQR_TREE=general), after each
of factor(), factor_fused() and factor_solve(workspace=True).

adj_cols are the adjoints lambda_c, K lambda_c + g_c = 0: they must have the bytes of solve_multi on the g_c, and they
and the forward columns are held against the dense solve by the criterion of tests/test_gpu_tree_vjp_solve.py:
|got - ref| <= 1e-10 max(1, max |ref|), block by block.

grad_input is held against the numpy restatement (tests/tree_vjp_multi_cases.py) evaluated on the dense z_c and
lambda_c.  Its bound is the sum over the columns of tree_vjp_cases.propagated_bound with that column's caps
e_z = 1e-10 max(1, max |z_c|), e_l = 1e-10 max(1, max |l_c|) (asserted first; the copies' share e_l is left out: those
slots are exactly 0 here) -- first-order propagation, as derived there, is linear in the columns -- plus the kernel's
own rounding (2 k + 1) 2^-53 a on the device's operands.  Every figure is printed before it is asserted."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import full_batch_problems as fb
import hard_inputs as hi
import tree_vjp_cases as tv
import tree_vjp_multi_cases as tm
from oracle import dense_kkt, oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BATCH = 3
COLS = 3
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


def _dense(topo, blocks, rhs):
    """[B, sol_len]: dense_kkt.solve of every problem with rhs [B, sol_len] in place of q, c, r."""
    out = []
    for b in range(rhs.shape[0]):
        gx, gy, gu = tv.views(topo, rhs[b:b + 1])
        prob = dict(fb.problem(blocks, b), q=[v[0] for v in gx], c=[v[0] for v in gy], r=[v[0] for v in gu])
        out.append(_row(topo, *dense_kkt.solve(topo.parents, topo.children, topo.sd, topo.cd, prob)))
    return np.stack(out)


_DRAWS = {}


def _draw(name):
    """(topo, blocks, rhs_cols, g_cols, z_ref, l_ref), the last four [COLS, B, sol_len]: computed once and read-only."""
    if name not in _DRAWS:
        topo = TOPOLOGIES[name][0]
        rng = np.random.default_rng(hi._seed("tree vjp multi solve", name))
        blocks = fb.make_blocks(topo, BATCH, rng, "random")
        L = topo.layout.sol_len
        rhs, g = rng.normal(size=(COLS, BATCH, L)), rng.normal(size=(COLS, BATCH, L))
        z_ref = np.stack([_dense(topo, blocks, rhs[c]) for c in range(COLS)])
        l_ref = np.stack([_dense(topo, blocks, g[c]) for c in range(COLS)])
        for a in (rhs, g, z_ref, l_ref):
            a.setflags(write=False)
        _DRAWS[name] = (topo, blocks, rhs, g, z_ref, l_ref)
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
    """Factor state in `work`, by one of the three factor entry points."""
    if how == "factor":
        return s.factor()
    if how == "factor_fused":
        return s.factor_fused()
    return s.factor_solve(workspace=True)[1]


@pytest.mark.parametrize("general", [False, True], ids=["size_class", "general_engine"])
@pytest.mark.parametrize("name", NAMES)
def test_backward_pass_against_the_dense_solve(name, general):
    topo, blocks, rhs, g, z_ref, l_ref = _draw(name)
    L, Lin = topo.layout.sol_len, tv.input_len(topo)
    s, maps = _plan(topo, general)
    if general or TOPOLOGIES[name][2] == "tree_generic":
        assert s.multi_kernel_name.startswith("tree_generic"), s.multi_kernel_name
    elif TOPOLOGIES[name][2].startswith("tree_factor_solve_qw16"):
        assert s.multi_kernel_name.startswith("tree_solve_mrhs_qw16"), s.multi_kernel_name
    assert s.vjp_multi_kernel_name == "tree_vjp_cols<staged,8>/f64" and s.vjp_multi_columns == 8
    ref, _, copy = tm.grad_input_multi(topo, z_ref, l_ref)
    cap_z = TOL * np.maximum(1.0, np.abs(z_ref).max(axis=2, initial=0.0))                # [COLS, B]
    cap_l = TOL * np.maximum(1.0, np.abs(l_ref).max(axis=2, initial=0.0))
    propagated = sum(tv.propagated_bound(topo, z_ref[c], l_ref[c], cap_z[c], cap_l[c]) for c in range(COLS))
    propagated = np.where(copy[None, :], 0, propagated)
    drhs, dg = _dev(rhs), _dev(g)
    for how in FACTORS:
        s.work.zero_(), s.output.zero_()
        _load(s, maps, topo, blocks)
        status = _forward(s, how)
        out_cols = s.solve_multi(drhs)
        work_before = s.work.clone()
        grad_input, adj = s.vjp_multi(dg, out_cols)
        by_solve = s.solve_multi(dg)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all(), (how, status)
        assert torch.equal(s.work, work_before), (how, "d_work was written")
        assert tuple(grad_input.shape) == (BATCH, max(1, Lin)) and tuple(adj.shape) == (COLS, BATCH, max(1, L))
        assert torch.equal(adj, by_solve), (how, "adj_cols are not the bytes of solve_multi on the g_c")
        z, lam = out_cols.cpu().numpy()[:, :, :L], adj.cpu().numpy()[:, :, :L]
        for c in range(COLS):
            ez = fb.block_rel_err(z[c], z_ref[c], maps.sol_blocks)
            el = fb.block_rel_err(lam[c], l_ref[c], maps.sol_blocks)
            print(f"TREE VJP MULTI SOLVE | {name} {s.multi_kernel_name} after {how} | column {c} block rel err output "
                  f"{ez.max():.2e} lambda {el.max():.2e} of {TOL:.0e}")
            assert (ez <= TOL).all() and (el <= TOL).all(), (how, c, ez, el)
            assert (np.abs(z[c] - z_ref[c]).max(axis=1, initial=0.0) <= cap_z[c]).all()
            assert (np.abs(lam[c] - l_ref[c]).max(axis=1, initial=0.0) <= cap_l[c]).all()
        on_device, mag, _ = tm.grad_input_multi(topo, z, lam)
        bound = propagated + tm.kernel_bound(mag, COLS)
        got = grad_input.cpu().numpy()[:, :Lin]
        diff = np.abs(got.astype(tv.LD) - ref)
        share = float((diff / np.where(bound > 0, bound, 1)).max(initial=0.0))
        print(f"TREE VJP MULTI SOLVE | {name} after {how} | worst |grad_input - ref| / bound = {share:.2e}; max |diff| "
              f"{float(diff.max(initial=0.0)):.2e}, max |ref| {float(np.abs(ref).max(initial=0.0)):.2e}")
        assert (diff <= bound).all(), (how, share)
        # and the kernel alone on the very operands it was given: its own bound, nothing propagated; the copies +0.0
        own = np.abs(got.astype(tv.LD) - on_device)
        assert (own <= tm.kernel_bound(mag, COLS)).all()
        assert (got[:, copy] == 0).all() and not np.signbit(got[:, copy]).any()
        # want_input=False: the lambda_c alone, the same bits, and out_cols is not needed
        none, again = s.vjp_multi(dg, None, want_input=False)
        torch.cuda.synchronize()
        assert none is None and torch.equal(again, adj)


@pytest.mark.parametrize("general", [False, True], ids=["size_class", "general_engine"])
def test_a_failed_problem_gets_zero_gradients_in_every_column(general):
    from sip_optimal_control_amd import FactorStatus
    topo, blocks, rhs, g, _, _ = _draw("random<9,3>")
    bad = {k: [a.copy() for a in v] for k, v in blocks.items()}
    node = next(i for i, n in enumerate(topo.sd) if n >= 3 and i > 0)
    bad["delta"][node][1, 2] = -1.0
    nodes, edges = fb.to_oracle(topo, bad)
    _, _, cpu_status = oracle.tree_batch(topo.parents, topo.children, topo.sd, topo.cd, nodes, edges)
    want = [0, int(FactorStatus.INVALID_DELTA), 0]
    assert cpu_status.tolist() == want                        # on the CPU oracle only that problem fails
    s, maps = _plan(topo, general)
    drhs, dg = _dev(rhs), _dev(g)
    _load(s, maps, topo, blocks)
    _forward(s, "factor_fused")
    out0 = s.solve_multi(drhs)
    gi0, adj0 = s.vjp_multi(dg, out0)
    gi0, adj0 = gi0.clone(), adj0.clone()
    _load(s, maps, topo, bad)
    status = _forward(s, "factor_fused")
    out = s.solve_multi(drhs)
    out[:, 1] = float("nan")                                  # whatever the failed problem's columns hold is not read
    gi, adj = s.vjp_multi(dg, out)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == want
    assert bool((adj[:, 1] == 0).all()) and bool((gi[1] == 0).all())
    good = [0, 2]
    assert torch.equal(adj[:, good], adj0[:, good]) and torch.equal(gi[good], gi0[good])
    assert bool((adj0[:, 1] != 0).any()) and bool((gi0[1] != 0).any())


@pytest.mark.parametrize("dims", hi.TREES, ids=lambda d: "<%d,%d>" % d)
def test_refined_adjoints_on_the_smallest_deltas(dims):
    """refine_iterations=2 on the delta[1e-9,1e-7] cell: the lambda_c are what refine_multi() gives on the g_c from a
    zero iterate, masked by status; the residual norms by round are recorded, and the result's is below the unrefined
    lambda's -- the criterion of the one-column test -- in every column on every problem."""
    cell = hi.tree_cell(*dims, "delta[1e-9,1e-7]")
    topo, L = cell.topo, cell.topo.layout.sol_len
    s, maps = _plan(topo, batch=hi.BATCH)
    s.input.copy_(torch.from_numpy(maps.pack_input(s, cell.nodes, cell.edges)))
    status = s.factor_fused()
    rng = np.random.default_rng(hi._seed("tree vjp multi refine", dims))
    rhs, g = _dev(rng.normal(size=(COLS, hi.BATCH, L))), _dev(rng.normal(size=(COLS, hi.BATCH, L)))
    out = s.solve_multi(rhs)
    gi0, lam0 = s.vjp_multi(g, out)
    gi2, lam2 = s.vjp_multi(g, out, refine_iterations=2)
    by_hand, norms = s.refine_multi(g, iterations=2, out_cols=torch.zeros_like(lam2))
    _, plain = s.residual_multi(lam0, rhs_cols=g, want_vector=False)
    _, refined = s.residual_multi(lam2, rhs_cols=g, want_vector=False)
    none, lam_only = s.vjp_multi(g, None, want_input=False, refine_iterations=2)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    norms, plain, refined = norms.cpu().numpy(), plain.cpu().numpy(), refined.cpu().numpy()
    for c in range(COLS):
        print(f"TREE VJP MULTI REFINE | <{dims[0]},{dims[1]}> column {c} | residual norm of lambda by round "
              f"{norms[:, c].max(axis=1)} | before (plain) {plain[c].max():.2e} after (refined) {refined[c].max():.2e}")
    assert torch.equal(by_hand, lam2) and none is None and torch.equal(lam_only, lam2)
    np.testing.assert_array_equal(norms[-1], refined)
    assert (refined < plain).all(), (refined, plain)
    # the gradient is the kernel on the columns and the refined lambdas
    z, lam = out.cpu().numpy()[:, :, :L], lam2.cpu().numpy()[:, :, :L]
    ref, mag, copy = tm.grad_input_multi(topo, z, lam)
    assert (np.abs(gi2.cpu().numpy().astype(tv.LD) - ref) <= tm.kernel_bound(mag, COLS)).all()


@pytest.mark.parametrize("name,general,batch", [("random<9,3>", False, 3), ("random<9,3>", False, 4096),
                                                ("general<17,9>", False, 5), ("random<15,8>", True, 7),
                                                ("single_node", False, 3)])
def test_scratch_bytes_is_what_the_header_documents(name, general, batch):
    s, _ = _plan(TOPOLOGIES[name][0], general, batch)
    lib = s._lib
    for num_rhs in (1, 3, 8, 17):
        want = int(lib.sip_lqr_tree_solve_multi_scratch_bytes(s._plan, num_rhs))
        assert int(lib.sip_lqr_tree_vjp_multi_scratch_bytes(s._plan, num_rhs)) == want and want > 0
    assert int(lib.sip_lqr_tree_vjp_multi_scratch_bytes(s._plan, 0)) == 0
    assert int(lib.sip_lqr_tree_vjp_multi_scratch_bytes(None, 3)) == 0


def test_every_misuse_on_a_valid_plan_is_an_invalid_argument():
    topo, blocks, rhs, g, _, _ = _draw("random<9,3>")
    s, maps = _plan(topo)
    _load(s, maps, topo, blocks)
    _forward(s, "factor_fused")
    drhs, dg = _dev(rhs), _dev(g)
    out = s.solve_multi(drhs)
    grad, adj = s.vjp_multi(dg, out)                                         # sizes the scratch
    want_grad, want_adj = grad.clone(), adj.clone()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ker_args = dict(plan=s._plan, out=P(out), adj=P(adj), num_rhs=COLS, status=P(s.status), grad=P(grad), stream=None)
    vjp_args = dict(plan=s._plan, input=P(s.input), work=P(s.work), out=P(out), gout=P(dg), num_rhs=COLS,
                    status=P(s.status), adj=P(adj), grad=P(grad), scratch=P(s._multi_scratch), stream=None)
    ker = lambda **kw: s._lib.sip_lqr_tree_vjp_input_multi(*{**ker_args, **kw}.values())
    vjp = lambda **kw: s._lib.sip_lqr_tree_vjp_multi(*{**vjp_args, **kw}.values())
    misuse = {"kernel plan": ker(plan=None), "kernel num_rhs": ker(num_rhs=-1), "kernel out": ker(out=None),
              "kernel adj": ker(adj=None), "kernel grad": ker(grad=None), "kernel grad, no columns": ker(grad=None, num_rhs=0),
              "vjp plan": vjp(plan=None), "vjp num_rhs": vjp(num_rhs=-1), "vjp input": vjp(input=None),
              "vjp work": vjp(work=None), "vjp out with grad_input": vjp(out=None), "vjp gout": vjp(gout=None),
              "vjp status": vjp(status=None), "vjp adj": vjp(adj=None), "vjp scratch": vjp(scratch=None)}
    for what, rc in misuse.items():
        assert rc == INVALID, (what, rc)
    torch.cuda.synchronize()
    assert torch.equal(grad, want_grad) and torch.equal(adj, want_adj)       # a refused call wrote nothing
    # and the well-formed calls run: the optional pointers left out too
    assert ker() == 0 and ker(status=None) == 0 and vjp() == 0 and vjp(grad=None) == 0
    assert vjp(grad=None, out=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad, want_grad) and torch.equal(adj, want_adj)
    # no column: nothing is solved, the gradient is zeros, and the column arrays may be NULL
    assert ker(num_rhs=0, out=None, adj=None) == 0 and vjp(num_rhs=0, out=None, gout=None, adj=None) == 0
    torch.cuda.synchronize()
    assert bool((grad == 0).all()) and torch.equal(adj, want_adj)

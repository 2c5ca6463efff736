"""sip_lqr_tree_vjp_input on the GPU (csrc/tree_vjp.hpp): the kernel alone against the numpy restatement of its formulas
(tests/tree_vjp_cases.py, long double) on random z and lambda -- no solve involved -- batch 3.

Every entry is held to |got - ref| <= 3 * 2^-53 * a, a = |s| (|l[ia] z[ib]| + |z[ia] l[ib]|), and the copies (q, c, r)
are exact.  Derivation of the 3: the kernel computes t2 = fl(z[ia] l[ib]), then fl(l[ia] z[ib] + t2) in one fused
operation: the first rounding errs by at most u |t2|, the second by at most u |t1 + t2| (1 + u), together at most
(2 u + u^2) (|t1| + |t2|) with u = 2^-53; the factor s is a power of two and exact.  The third u covers u^2 and the 2^-64
of the long-double reference.  Each case prints the worst ratio |got - ref| / (2^-53 a); DESIGN 4.11.1 records one run.

The output is pre-filled with NaN and sits between guard words: no NaN survives (every scalar is written) and no guard
changes (nothing else is).  variable_branch has input_len = 59, so problems 1 and 2 of the batch, laid out back to back,
start off a 16-byte boundary; one case more starts the whole output one scalar off."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import chain_guards as cg
import full_batch_problems as fb
import tree_vjp_cases as tv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BATCH = 3
CASES = tv.topologies()


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


def _plan(topo, batch=BATCH):
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    maps = fb.PlanMaps(s, topo)
    # the oracle's sol layout is the plan's output layout, and [nodes | edges] the plan's input arena
    assert np.array_equal(maps.sol_idx, np.arange(topo.layout.sol_len))
    assert np.array_equal(maps.input_idx, np.arange(tv.input_len(topo))) and s.in_len == tv.input_len(topo)
    return s


_DRAWS = {}


def _draw(name, batch=BATCH):
    """z, lambda (float64 numpy) and the long-double reference with its magnitudes, computed once and read-only."""
    key = (name, batch)
    if key not in _DRAWS:
        topo = CASES[name][0]
        rng = np.random.default_rng(2000 + 7 * len(name) + topo.layout.sol_len + batch)
        sol, adj = rng.normal(size=(batch, topo.layout.sol_len)), rng.normal(size=(batch, topo.layout.sol_len))
        ref, mag, copy = tv.grad_input(topo, sol, adj)
        for a in (sol, adj, ref, mag, copy):
            a.setflags(write=False)
        _DRAWS[key] = (sol, adj, ref, mag, copy)
    return _DRAWS[key]


def _dev(a):
    a = np.asarray(a, dtype=np.float64)
    if a.shape[-1] == 0:                                      # an empty arena is one unused scalar wide
        a = np.zeros(a.shape[:-1] + (1,))
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _launch(s, sol, adj, status, shift=0):
    """sip_lqr_tree_vjp_input into a NaN-filled output between guards; shift: scalars the output starts off the frame's
    16-byte aligned view.  -> (output [batch, in_len] numpy, guards intact)."""
    B, L = s.batch, s.in_len
    full, _ = cg.framed((B * L + shift,), torch.float64, "cuda:0")
    assert full.data_ptr() % 16 == 0 and cg.GUARD % 2 == 0
    full[cg.GUARD + shift:cg.GUARD + shift + B * L] = float("nan")
    out = full[cg.GUARD + shift:cg.GUARD + shift + B * L]
    assert (out.data_ptr() % 16 == 0) == (shift % 2 == 0)
    rc_ = s._lib.sip_lqr_tree_vjp_input(s._plan, ctypes.c_void_p(sol.data_ptr()), ctypes.c_void_p(adj.data_ptr()),
                                        ctypes.c_void_p(status.data_ptr() if status is not None else None),
                                        ctypes.c_void_p(out.data_ptr()),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0, rc_
    torch.cuda.synchronize()
    want = cg._sentinel(torch.float64)
    intact = bool((full[:cg.GUARD + shift] == want).all()) and bool((full[cg.GUARD + shift + B * L:] == want).all())
    return out.cpu().numpy().reshape(B, L), intact


def _check(tag, got, ref, mag, copy):
    assert not np.isnan(got).any(), (tag, "a scalar of the output was not written", int(np.isnan(got).sum()))
    diff = np.abs(got.astype(tv.LD) - ref)
    worst = float((diff / np.where(mag > 0, mag, 1)).max(initial=0.0) / tv.U)
    print(f"TREE VJP | {tag} | worst |got - ref| / (2^-53 a) = {worst:.2f} of {tv.C_ROUNDINGS}")
    assert (diff <= tv.kernel_bound(mag)).all(), (tag, worst)
    assert (diff[:, copy] == 0).all(), (tag, "a copy is not exact")


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_numpy(name):
    topo, kernel, solve_kernel = CASES[name]
    s = _plan(topo)
    assert s.vjp_kernel_name == kernel and s.kernel_name.startswith(solve_kernel), (s.vjp_kernel_name, s.kernel_name)
    sol, adj, ref, mag, copy = _draw(name)
    ds, da = _dev(sol), _dev(adj)
    got, intact = _launch(s, ds, da, None)
    assert intact, (name, "a guard word changed")
    _check(name, got, ref, mag, copy)
    again, _ = _launch(s, ds, da, None)                                                # two launches, the same bits
    assert got.tobytes() == again.tobytes(), name
    by_method = s.vjp_input(ds, da, use_status=False)
    torch.cuda.synchronize()
    assert by_method.cpu().numpy()[:, :s.in_len].tobytes() == got.tobytes(), name


def test_an_odd_input_len_and_an_output_one_scalar_off_alignment():
    """input_len = 59: problems 1 and 2 start off a 16-byte boundary and begin and end with partial pieces; with the
    output one scalar off, problem 0 does too.  The same values wherever the output lies."""
    name = "variable_branch"
    s = _plan(CASES[name][0])
    assert s.in_len == 59
    sol, adj, ref, mag, copy = _draw(name)
    ds, da = _dev(sol), _dev(adj)
    aligned, intact = _launch(s, ds, da, None)
    assert intact
    got, intact = _launch(s, ds, da, None, shift=1)
    assert intact, "a guard word changed"
    _check(f"{name} output + 1 scalar", got, ref, mag, copy)
    assert got.tobytes() == aligned.tobytes()


@pytest.mark.parametrize("name", ["five_node", "random<15,8>", "chain_30x70"])
def test_a_failed_problem_gets_zeros_by_a_branch(name):
    """One problem whose status is not SUCCESS and whose z and lambda are NaN: exact zeros there (a multiplication by
    zero would leave NaN), its neighbours bit for bit what they are without it; d_status = NULL masks nothing."""
    s = _plan(CASES[name][0])
    sol, adj, ref, mag, copy = _draw(name)
    ds, da = _dev(sol), _dev(adj)
    plain, _ = _launch(s, ds, da, None)
    failed, good = 1, [0, 2]
    ds[failed], da[failed] = float("nan"), float("nan")
    status = torch.zeros(BATCH, dtype=torch.int32, device="cuda:0")
    status[failed] = 3
    got, intact = _launch(s, ds, da, status, shift=1)
    assert intact
    assert (got[failed] == 0).all() and not np.signbit(got[failed]).any()
    assert got[good].tobytes() == plain[good].tobytes()
    _check(f"{name} with a failed neighbour", got[good], ref[good], mag[good], copy)
    unmasked, intact = _launch(s, ds, da, None)
    assert intact
    assert np.isnan(unmasked[failed]).all()                                            # nothing is masked
    assert unmasked[good].tobytes() == plain[good].tobytes()


def test_every_problem_of_a_batch_beyond_the_cus():
    """300 distinct problems of the five-node tree, more workgroups than compute units: problem by problem."""
    name, batch = "five_node", 300
    s = _plan(CASES[name][0], batch)
    sol, adj, ref, mag, copy = _draw(name, batch)
    assert np.abs(np.diff(ref.astype(np.float64), axis=0)).max(axis=1).min() > 1e-3    # neighbours differ
    got, intact = _launch(s, _dev(sol), _dev(adj), None)
    assert intact
    _check(f"{name} x {batch}", got, ref, mag, copy)


@pytest.mark.parametrize("name", ["random<15,8>", "variable_branch", "chain_30x70"])
def test_several_runs_per_problem_give_the_bits_of_one(name):
    """SIP_LQR_TREE_VJP_SHAPE=<wavefronts>,<entries per run> splits a problem over several workgroups: the same bits,
    guards intact, on the aligned and on the shifted output."""
    s = _plan(CASES[name][0])
    sol, adj, ref, mag, copy = _draw(name)
    ds, da = _dev(sol), _dev(adj)
    with _env(SIP_LQR_TREE_VJP_SHAPE="8,%d" % (2 * s.in_len)):
        one, intact = _launch(s, ds, da, None)
    assert intact
    _check(f"{name} one run", one, ref, mag, copy)
    for shape in ("2,10", "3,7", "8,128", "1,%d" % max(2, s.in_len // 2)):
        for shift in (0, 1):
            with _env(SIP_LQR_TREE_VJP_SHAPE=shape):
                got, intact = _launch(s, ds, da, None, shift=shift)
            assert intact, (shape, shift)
            assert got.tobytes() == one.tobytes(), (shape, shift)


def test_a_chain_written_as_a_tree_against_the_chain_kernel():
    """The uniform chain (5, 3, T = 7) as a tree plan and as a chain plan, the same z and lambda through the offset maps
    of the two layouts: the matrix blocks of the tree's gradient against sip_lqr_vjp_mats.  Both are held to the bound
    above; beyond that the two kernels compute fma(l[ia], z[ib], z[ia] * l[ib]) times s with the same ia, ib, and the
    test asserts that THE BITS AGREE."""
    from sip_optimal_control_amd import BatchedChainLQR, ChainShape
    n, m, T = 5, 3, 7
    topo = fb.Topology(list(range(T)), list(range(1, T + 1)), [n] * (T + 1), [m] * T, "chain(5,3,7)")
    s = _plan(topo)
    assert s.vjp_kernel_name == tv.STAGED
    chain = BatchedChainLQR(n, m, T, BATCH)
    shape = ChainShape(n, m, T)
    lay = topo.layout
    rng = np.random.default_rng(99)
    sol, adj = rng.normal(size=(BATCH, lay.sol_len)), rng.normal(size=(BATCH, lay.sol_len))
    # tree sol -> chain sol (x_i | y_i | u_i per stage), and chain mats index -> tree input index
    to_chain = []
    for i in range(T + 1):
        to_chain += list(range(lay.x_off[i], lay.x_off[i] + 2 * n))
        if i < T:
            to_chain += list(range(lay.u_off[i], lay.u_off[i] + m))
    to_chain = np.array(to_chain)
    assert to_chain.size == shape.vecs_len == lay.sol_len
    tree_of = np.full(shape.mats_len, -1, dtype=np.int64)
    for i in range(T + 1):
        off = shape.mats_off(i)
        node = lay.node_off[i]
        tree_of[off["Q"]:off["Q"] + n * n] = node + np.arange(n * n)
        tree_of[off["delta"]:off["delta"] + n] = node + n * n + 2 * n + np.arange(n)
        if i < T:
            edge, at = lay.nodes_len + lay.edge_off[i], 0
            for key, size in (("A", n * n), ("B", n * m), ("M", n * m), ("R", m * m)):
                tree_of[off[key]:off[key] + size] = edge + at + np.arange(size)
                at += size
    assert (tree_of >= 0).all() and np.unique(tree_of).size == tree_of.size
    got_tree, intact = _launch(s, _dev(sol), _dev(adj), None)
    assert intact
    got_chain = chain.vjp_mats(_dev(sol[:, to_chain]), _dev(adj[:, to_chain]), use_status=False)
    torch.cuda.synchronize()
    got_chain = got_chain.cpu().numpy()
    ref, mag, copy = tv.grad_input(topo, sol, adj)
    _check("chain(5,3,7) as a tree", got_tree, ref, mag, copy)
    diff = np.abs(got_chain.astype(tv.LD) - ref[:, tree_of])
    assert (diff <= tv.kernel_bound(mag[:, tree_of])).all()
    same = got_tree[:, tree_of].tobytes() == got_chain.tobytes()
    print(f"TREE VJP | chain(5,3,7) as a tree against chain_vjp_kernel | bits agree: {same}")
    assert same

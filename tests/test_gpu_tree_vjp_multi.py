"""sip_lqr_tree_vjp_input_multi on the GPU (csrc/tree_vjp_cols.hpp): the kernel alone against the numpy restatement of
its formulas (tests/tree_vjp_multi_cases.py, long double) on random z_c and lambda_c -- no solve involved -- batch 3.

Every entry is held to |got - ref| <= (2 k + 1) * 2^-53 * a for k columns, a = sum_c |s| (|l_c[ia] z_c[ib]| +
|z_c[ia] l_c[ib]|) (derived in tests/tree_vjp_multi_cases.py: two roundings per column, chained; s and its undoing
between two launches are exact), and the q, c, r slots are exactly +0.0.  Each case prints the worst ratio
|got - ref| / (2^-53 a).

Trees: all twelve of tree_vjp_cases.topologies() (chain_30x70 is the direct form) and one staged tree whose 8 columns do
not fit 64 KiB: the chain [14] * 20 with m = 4, out_len 636 -- 6 columns under 64 KiB, 8 where the kernel's limit of
dynamic LDS is raised; the test takes either, whichever csrc/tree_vjp_cols_shape.hpp keeps.  Columns: 1, 3, C, C + 1,
2 C + 1 with C the plan's vjp_multi_columns: a short group, a full one, a full one and one column, two full ones and
one.  chain_30x30 (out_len 1916) has a natural group below 8 under either candidate.

The output is pre-filled with NaN and sits between guard words: no NaN survives (every scalar is written, and the first
group never reads the output) and no guard changes (nothing else is written)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import chain_guards as cg
import full_batch_problems as fb
import tree_vjp_cases as tv
import tree_vjp_multi_cases as tm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BATCH = 3
CASES = dict(tv.topologies())
CASES["chain_14x20"] = (fb.Topology(list(range(19)), list(range(1, 20)), [14] * 20, [4] * 19, "chain_14x20"), tv.STAGED,
                        "tree_")
# and one whose natural group is below 8 whichever candidate is kept: out_len 1916, 2 columns in 64 KiB, 5 in 160 KiB
CASES["chain_30x30"] = (fb.Topology(list(range(29)), list(range(1, 30)), [30] * 30, [4] * 29, "chain_30x30"), tv.STAGED,
                        "tree_")
BUDGET, MOST = 64 * 1024, 160 * 1024


def _columns(topo):
    """The candidates of csrc/tree_vjp_cols_shape.hpp, restated: the direct form with 8 where not one column fits 64 KiB,
    else what 64 KiB hold or what the 160 KiB of a workgroup hold, 8 at the most -> the set of admissible answers."""
    L = topo.layout.sol_len
    if L == 0 or 16 * L > BUDGET:
        return {8}
    return {min(8, BUDGET // (16 * L)), min(8, MOST // (16 * L))}


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


def _draw(name, cols, batch=BATCH):
    """z_c, lambda_c [cols, batch, sol_len] (float64 numpy) and, for every k <= cols, the long-double reference of the
    first k columns with its magnitudes: computed once, cumulatively in ascending order, and read-only."""
    key = (name, batch)
    if key not in _DRAWS or _DRAWS[key][0].shape[0] < cols:
        topo = CASES[name][0]
        rng = np.random.default_rng(3000 + 7 * len(name) + topo.layout.sol_len + batch)
        sol = rng.normal(size=(cols, batch, topo.layout.sol_len))
        adj = rng.normal(size=(cols, batch, topo.layout.sol_len))
        refs, mags = [], []
        ref, mag, copy = tm.grad_input_multi(topo, sol[:0], adj[:0])
        for c in range(cols):
            g, a, _ = tv.grad_input(topo, sol[c], adj[c])
            ref, mag = ref + np.where(copy[None, :], 0, g), mag + a
            refs.append(ref), mags.append(mag)
        for a in [sol, adj, copy] + refs + mags:
            a.setflags(write=False)
        _DRAWS[key] = (sol, adj, refs, mags, copy)
    sol, adj, refs, mags, copy = _DRAWS[key]
    return sol[:cols], adj[:cols], refs[cols - 1], mags[cols - 1], copy


def _dev(a):
    a = np.asarray(a, dtype=np.float64)
    if a.shape[-1] == 0:                                      # an empty arena is one unused scalar wide
        a = np.zeros(a.shape[:-1] + (1,))
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _launch(s, sol, adj, status, shift=0, num_rhs=None):
    """sip_lqr_tree_vjp_input_multi into a NaN-filled output between guards; shift: scalars the output starts off the
    frame's 16-byte aligned view.  -> (output [batch, in_len] numpy, guards intact)."""
    B, L = s.batch, s.in_len
    num_rhs = sol.shape[0] if num_rhs is None else num_rhs
    full, _ = cg.framed((B * L + shift,), torch.float64, "cuda:0")
    assert full.data_ptr() % 16 == 0 and cg.GUARD % 2 == 0
    full[cg.GUARD + shift:cg.GUARD + shift + B * L] = float("nan")
    out = full[cg.GUARD + shift:cg.GUARD + shift + B * L]
    assert (out.data_ptr() % 16 == 0) == (shift % 2 == 0)
    rc_ = s._lib.sip_lqr_tree_vjp_input_multi(
        s._plan, ctypes.c_void_p(sol.data_ptr() if num_rhs else None),
        ctypes.c_void_p(adj.data_ptr() if num_rhs else None), num_rhs,
        ctypes.c_void_p(status.data_ptr() if status is not None else None), ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0, rc_
    torch.cuda.synchronize()
    want = cg._sentinel(torch.float64)
    intact = bool((full[:cg.GUARD + shift] == want).all()) and bool((full[cg.GUARD + shift + B * L:] == want).all())
    return out.cpu().numpy().reshape(B, L), intact


def _check(tag, got, ref, mag, copy, cols):
    assert not np.isnan(got).any(), (tag, "a scalar of the output was not written", int(np.isnan(got).sum()))
    diff = np.abs(got.astype(tv.LD) - ref)
    worst = float((diff / np.where(mag > 0, mag, 1)).max(initial=0.0) / tv.U)
    print(f"TREE VJP MULTI | {tag} | {cols} columns | worst |got - ref| / (2^-53 a) = {worst:.2f} of {tm.roundings(cols)}")
    assert (diff <= tm.kernel_bound(mag, cols)).all(), (tag, cols, worst)
    assert (got[:, copy] == 0).all() and not np.signbit(got[:, copy]).any(), (tag, "a q, c or r slot is not +0.0")


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_numpy(name):
    topo, single, _ = CASES[name]
    s = _plan(topo)
    C = s.vjp_multi_columns
    assert C in _columns(topo), (C, _columns(topo))
    form = "direct" if single == tv.DIRECT else "staged"
    assert s.vjp_multi_kernel_name == f"tree_vjp_cols<{form},{C}>/f64", s.vjp_multi_kernel_name
    if name == "chain_14x20":
        assert s.out_len == 636 and C in (6, 8) and 8 * 16 * s.out_len > BUDGET
    if name == "chain_30x30":
        assert s.out_len == 1916 and C in (2, 5)
    if name == "chain_30x70":
        assert 16 * s.out_len > BUDGET and C == 8
    _draw(name, 2 * C + 1)                                    # one draw: the shorter calls are its first columns
    for cols in (1, 3, C, C + 1, 2 * C + 1):
        sol, adj, ref, mag, copy = _draw(name, cols)
        ds, da = _dev(sol), _dev(adj)
        got, intact = _launch(s, ds, da, None)
        assert intact, (name, cols, "a guard word changed")
        _check(name, got, ref, mag, copy, cols)
        if cols == 1:                                         # bit for bit the one-column kernel off the copy slots
            one = s.vjp_input(ds[0], da[0], use_status=False)
            torch.cuda.synchronize()
            one = one.cpu().numpy()[:, :s.in_len]
            assert got[:, ~copy].tobytes() == one[:, ~copy].tobytes(), name
            if copy.any():
                assert one[:, copy].tobytes() != got[:, copy].tobytes()                # there it holds lambda
        if cols == 2 * C + 1:
            again, _ = _launch(s, ds, da, None)                                        # two launches, the same bits
            assert got.tobytes() == again.tobytes(), name
            by_method = s.vjp_input_multi(ds, da, use_status=False)
            torch.cuda.synchronize()
            assert by_method.cpu().numpy()[:, :s.in_len].tobytes() == got.tobytes(), name


@pytest.mark.parametrize("name", ["five_node", "chain_14x20", "chain_30x30", "chain_30x70"])
def test_the_grouping_does_not_change_a_bit(name):
    """7 columns in groups of 8 (or the plan's own), 3 and 1: identical bytes -- the later groups undo s exactly and chain
    onto the scalar the earlier ones left."""
    s = _plan(CASES[name][0])
    sol, adj, ref, mag, copy = _draw(name, 7)
    ds, da = _dev(sol), _dev(adj)
    got = {}
    for cap in ("8", "3", "1"):
        with _env(SIP_LQR_TREE_VJP_MULTI_COLUMNS=cap):
            got[cap], intact = _launch(s, ds, da, None, shift=1)
        assert intact, (name, cap)
        _check(f"{name} groups of {cap}", got[cap], ref, mag, copy, 7)
    assert got["8"].tobytes() == got["3"].tobytes() == got["1"].tobytes(), name
    plain, _ = _launch(s, ds, da, None)
    assert plain.tobytes() == got["8"].tobytes()


@pytest.mark.parametrize("name", ["variable_branch", "chain_30x70", "single_node"])
def test_no_column_gives_zeros(name):
    s = _plan(CASES[name][0])
    sol, adj, _, _, _ = _draw(name, 1)
    got, intact = _launch(s, _dev(sol), _dev(adj), None, shift=1, num_rhs=0)
    assert intact
    assert (got == 0).all() and not np.signbit(got).any()
    empty = torch.empty(0, BATCH, max(1, s.out_len), dtype=torch.float64, device="cuda:0")
    by_method = s.vjp_input_multi(empty, empty)
    torch.cuda.synchronize()
    assert bool((by_method == 0).all())


def test_an_odd_input_len_and_an_output_one_scalar_off_alignment():
    """input_len = 59: problems 1 and 2 start off a 16-byte boundary and begin and end with partial pieces; with the
    output one scalar off, problem 0 does too.  The same values wherever the output lies, with one group and with an
    accumulating second one (which reads and writes the same pieces)."""
    name = "variable_branch"
    s = _plan(CASES[name][0])
    assert s.in_len == 59
    for cols in (3, 9):
        sol, adj, ref, mag, copy = _draw(name, cols)
        ds, da = _dev(sol), _dev(adj)
        aligned, intact = _launch(s, ds, da, None)
        assert intact
        got, intact = _launch(s, ds, da, None, shift=1)
        assert intact, "a guard word changed"
        _check(f"{name} output + 1 scalar", got, ref, mag, copy, cols)
        assert got.tobytes() == aligned.tobytes()


@pytest.mark.parametrize("name", ["five_node", "chain_14x20", "chain_30x70"])
def test_a_failed_problem_gets_zeros_by_a_branch(name):
    """One problem whose status is not SUCCESS and whose columns are NaN: exact zeros there (a multiplication by zero
    would leave NaN) after the first group and after the accumulating ones, its neighbours bit for bit what they are
    without it; d_status = NULL masks nothing."""
    s = _plan(CASES[name][0])
    cols = s.vjp_multi_columns + 2
    sol, adj, ref, mag, copy = _draw(name, cols)
    ds, da = _dev(sol), _dev(adj)
    plain, _ = _launch(s, ds, da, None)
    failed, good = 1, [0, 2]
    ds[:, failed], da[:, failed] = float("nan"), float("nan")
    status = torch.zeros(BATCH, dtype=torch.int32, device="cuda:0")
    status[failed] = 3
    got, intact = _launch(s, ds, da, status, shift=1)
    assert intact
    assert (got[failed] == 0).all() and not np.signbit(got[failed]).any()
    assert got[good].tobytes() == plain[good].tobytes()
    _check(f"{name} with a failed neighbour", got[good], ref[good], mag[good], copy, cols)
    unmasked, intact = _launch(s, ds, da, None)
    assert intact
    assert np.isnan(unmasked[failed][~copy]).all() and (unmasked[failed][copy] == 0).all()   # nothing is masked
    assert unmasked[good].tobytes() == plain[good].tobytes()


def test_every_problem_of_a_batch_beyond_the_cus():
    """300 distinct problems of the five-node tree, more workgroups than compute units: problem by problem."""
    name, batch, cols = "five_node", 300, 3
    s = _plan(CASES[name][0], batch)
    sol, adj, ref, mag, copy = _draw(name, cols, batch)
    assert np.abs(np.diff(ref.astype(np.float64), axis=0)).max(axis=1).min() > 1e-3    # neighbours differ
    got, intact = _launch(s, _dev(sol), _dev(adj), None)
    assert intact
    _check(f"{name} x {batch}", got, ref, mag, copy, cols)


@pytest.mark.parametrize("name", ["random<15,8>", "variable_branch", "chain_30x70"])
def test_several_runs_per_problem_give_the_bits_of_one(name):
    """SIP_LQR_TREE_VJP_COLS_SHAPE=<wavefronts>,<entries per run> splits a problem over several workgroups: the same
    bits, guards intact, on the aligned and on the shifted output, with an accumulating group among them."""
    s = _plan(CASES[name][0])
    cols = s.vjp_multi_columns + 1
    sol, adj, ref, mag, copy = _draw(name, cols)
    ds, da = _dev(sol), _dev(adj)
    with _env(SIP_LQR_TREE_VJP_COLS_SHAPE="8,%d" % (2 * s.in_len)):
        one, intact = _launch(s, ds, da, None)
    assert intact
    _check(f"{name} one run", one, ref, mag, copy, cols)
    for shape in ("2,10", "3,7", "8,128", "1,%d" % max(2, s.in_len // 2)):
        for shift in (0, 1):
            with _env(SIP_LQR_TREE_VJP_COLS_SHAPE=shape):
                got, intact = _launch(s, ds, da, None, shift=shift)
            assert intact, (shape, shift)
            assert got.tobytes() == one.tobytes(), (shape, shift)


def test_a_chain_written_as_a_tree_against_the_chain_kernel():
    """The uniform chain (5, 3, T = 7) as a tree plan and as a chain plan, 3 columns of the same z_c and lambda_c through
    the offset maps of the two layouts: the matrix blocks of the tree's gradient against sip_lqr_vjp_mats_multi.  The two
    kernels chain the same fma expressions over the columns in the same order with the same ia, ib, and the test
    asserts that THE BITS AGREE on the shared blocks."""
    from sip_optimal_control_amd import BatchedChainLQR, ChainShape
    n, m, T, cols = 5, 3, 7, 3
    topo = fb.Topology(list(range(T)), list(range(1, T + 1)), [n] * (T + 1), [m] * T, "chain(5,3,7)")
    s = _plan(topo)
    assert s.vjp_multi_kernel_name == "tree_vjp_cols<staged,8>/f64"
    chain = BatchedChainLQR(n, m, T, BATCH)
    shape = ChainShape(n, m, T)
    lay = topo.layout
    rng = np.random.default_rng(199)
    sol, adj = rng.normal(size=(cols, BATCH, lay.sol_len)), rng.normal(size=(cols, BATCH, lay.sol_len))
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
    got_chain = chain.vjp_mats_multi(_dev(sol[:, :, to_chain]), _dev(adj[:, :, to_chain]), use_status=False)
    torch.cuda.synchronize()
    got_chain = got_chain.cpu().numpy()
    ref, mag, copy = tm.grad_input_multi(topo, sol, adj)
    _check("chain(5,3,7) as a tree", got_tree, ref, mag, copy, cols)
    assert not copy[tree_of].any()
    same = got_tree[:, tree_of].tobytes() == got_chain.tobytes()
    print(f"TREE VJP MULTI | chain(5,3,7) as a tree against chain_vjp_cols_kernel | bits agree: {same}")
    assert same

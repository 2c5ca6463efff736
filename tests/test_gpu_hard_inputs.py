"""Every kernel family over the regularization and scaling range: tests/hard_inputs.py's axes (delta from 1e-9 to 1e6,
mixed inside a node; a condensed-problem cost with the diagonal of F around 1e3; both; expanding dynamics) against an
extended-precision solve of the dense KKT system (tests/extended_reference.py).  Batch 3, every problem checked;
T = 12 for n <= 16, T = 6 above, trees of 10 nodes.  Every test asserts the kernel it expects to run on.

Notation: e(v) = max over the problems of max |v - ext| / max |ext| over x, u, y.

fp64: statuses are the oracle's (all 0); e_gpu <= 1e-9 + 3 e_ref, e_ref = e(CPU oracle), the reference algorithm in
fp64 (1e-9: the project's fp64 tolerance; 3: the margin test_accuracy_tracks_the_reference_algorithm_over_delta gives
a kernel over the oracle for another summation order).  Gains: u = K x + k at the kernel's own x to 1e-9 of max |u|;
and K, k against the oracle's to the same form of cap, 1e-9 + 3 e_ref_gains, where e_ref_gains = e(the oracle's K, k
against extended_reference.riccati_gains, the recursion in long double) is the reference algorithm's own error on the
gains -- at delta ~ 1e-9 its W = D^-1/2 (I - F^-1) D^-1/2 cancels and two correct fp64 evaluations of K differ by up to
5e-8 on the trees, which the error of x, u, y (e_ref) does not measure; K, k against the extended gains themselves are
held to the same cap.  tests/test_hard_inputs_reference.py asserts without a GPU that every cell used here has e_ref
and e_ref_gains <= 1e-7, a dense reference whose last refinement step moved it by <= 1e-12, and the two extended
references tied by u = K x + k to 1e-12.

fp32: the CPU oracle is fp64, so the yardstick is the general fp32 engine (tree_generic(chain layout)/f32) on the same
fp32-rounded inputs, `ext` being the solution of the rounded problem: e_gpu <= F32_TOL + 3 e_general, and
e_general <= 1e-2 keeps the cell meaningful.

Two cases differ from a plain reading of the list of families: the large-delta axis of the trees is [1, 30] (the
random family is not convex: hard_inputs.AXES_TREE), and an fp64 chain at (17, 4) is embedded in mt16<32,4>, so the
general engine is met at (17, 4) under SIP_LQR_PAD=0 and, with nothing set, at (17, 9).

Every test prints its figures ("HARD | family | axis | e_gpu | yardstick | gains against the oracle's | gains against
the extended ones | e_ref_gains | u = K x + k"); DESIGN 7.1 holds the table of one run.

Expected to fail (strict): the fused fp32 mt16 kernel at delta in [1e-1, 1e2] measures 2.3e-2 against 2.4e-6 of the
general engine -- it sweeps F = I + D^1/2 V D^1/2 as it stands, which the fp64 instantiation no longer does."""
import contextlib
import os

import numpy as np
import pytest

import chain_guards as cg
import extended_reference as xr
import full_batch_problems as fb
import hard_inputs as hi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CAP = 1e-9
SEP = " + chain_factor_mt16 + chain_solve_mt16"
GENERAL = "tree_generic(chain layout)"


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype=dtype or torch.float64)


NAN = float("nan")


def _report(family, axis, e_gpu, yardstick, e_gains=NAN, e_gains_ext=NAN, e_ref_gains=NAN, e_u=NAN):
    print(f"HARD | {family} | {axis} | {e_gpu:.1e} | {yardstick:.1e} | {e_gains:.1e} | {e_gains_ext:.1e} | "
          f"{e_ref_gains:.1e} | {e_u:.1e}")


def _u_from_gains_chain(n, m, T, sol, gains):
    """max |u - (K x + k)| / max |u| per problem, x and u the kernel's own (lqr.cpp:856-857)."""
    B, vs = sol.shape[0], 2 * n + m
    body = sol[:, :T * vs].reshape(B, T, vs)
    x, u = body[:, :, :n], body[:, :, 2 * n:]
    g = gains.reshape(B, T, m * n + m)
    K, k = g[:, :, :m * n].reshape(B, T, n, m), g[:, :, m * n:]      # K column-major m x n: (j, c) at c * m + j
    return float((np.abs(u - (np.einsum("btcj,btc->btj", K, x) + k)).max(axis=(1, 2)) / np.abs(u).max(axis=(1, 2))).max())


def _judge_f64(family, cell, sol, status, gains, u_err):
    np.testing.assert_array_equal(status, cell.ref_status)
    e_gpu, e_gains, e_gains_ext = xr.err(sol, cell.ext), xr.err(gains, cell.ref_gains), xr.err(gains, cell.ext_gains)
    _report(family, cell.axis, e_gpu, cell.e_ref, e_gains, e_gains_ext, cell.e_ref_gains, u_err)
    assert e_gpu <= CAP + 3 * cell.e_ref, (family, cell.axis, e_gpu, cell.e_ref)
    assert u_err <= CAP, (family, cell.axis, "u = K x + k", u_err)
    assert e_gains <= CAP + 3 * cell.e_ref_gains, (family, cell.axis, "gains against the oracle's", e_gains, cell.e_ref_gains)
    assert e_gains_ext <= CAP + 3 * cell.e_ref_gains, (family, cell.axis, "gains", e_gains_ext, cell.e_ref_gains)


def _judge_columns(family, cell, sol_cols, rows):
    e_gpu = max(xr.err(sol_cols[c][:rows], cell.col_ext[c]) for c in range(cell.ncols))
    _report(family, cell.axis, e_gpu, cell.e_ref_cols)
    assert e_gpu <= CAP + 3 * cell.e_ref_cols, (family, cell.axis, e_gpu, cell.e_ref_cols)


# ---- chains, fp64 ------------------------------------------------------------------------------------------------
# family -> (n, m, environment of the plan's creation, constructor arguments, what the kernel name holds, entry points)
CHAINS = {
    "qw16 staged (12,4)": (12, 4, {}, {}, ("qw16<12,4,staged>",), "fused"),
    "qw16 staged odd (5,3)": (5, 3, {}, {}, ("qw16<5,3,staged>",), "fused"),
    "qw16 staged largest (15,8)": (15, 8, {}, {}, ("qw16<15,8,staged>",), "fused"),
    "qw16 direct (16,4)": (16, 4, {}, {}, ("qw16<16,4,direct>",), "fused"),
    "qw16 symmetric-packed (8,4)": (8, 4, {}, {"symmetric": True}, ("qw16<8,4,staged,sym>",), "fused"),
    "qw16 split form (12,4)": (12, 4, {}, {}, ("qw16<12,4,staged>",), "split"),
    "qw16 embedding (10,3) in <12,3>": (10, 3, {"SIP_LQR_EXTRA": "0"}, {}, ("qw16<12,3,staged>", "embedding (10,3)"), "fused"),
    "qw16 factor + solve_multi(8) (12,4)": (12, 4, {}, {}, ("qw16<12,4,staged>",), "multi"),
    "qw16 factor + solve_multi(8) (16,8)": (16, 8, {}, {}, ("qw16<16,8,direct>",), "multi"),
    "mt16 fused (32,8)": (32, 8, {}, {}, ("mt16<32,8,",), "fused"),
    "mt16 factor + solve (32,8)": (32, 8, {}, {}, ("mt16<32,8,",), "factor_solve"),
    "mt16 separate sweeps, factor + solve (32,8)": (32, 8, {}, {"separate_sweeps": True}, ("mt16<32,8,", SEP), "factor_solve"),
    "mt16 separate sweeps, solve_multi(9) (32,8)": (32, 8, {}, {"separate_sweeps": True}, ("mt16<32,8,", SEP), "multi"),
    "mt16 embedding (20,3)": (20, 3, {}, {}, ("mt16<32,4,", "embedding (20,3)"), "fused"),
    "mt16 embedding (17,4)": (17, 4, {}, {}, ("mt16<32,4,", "embedding (17,4)"), "fused"),
    "general engine forced (12,4)": (12, 4, {"SIP_LQR_VARIANT": "general"}, {}, (GENERAL,), "fused"),
    "general engine, no embedding (17,4)": (17, 4, {"SIP_LQR_PAD": "0"}, {}, (GENERAL,), "fused"),
    "general engine natural (17,9)": (17, 9, {}, {}, (GENERAL,), "fused"),
}
NO_SEP = ("mt16 fused (32,8)", "mt16 factor + solve (32,8)", "mt16 embedding (20,3)", "mt16 embedding (17,4)")


@pytest.mark.parametrize("axis", hi.AXES_F64)
@pytest.mark.parametrize("family", list(CHAINS))
def test_hard_chain_f64(family, axis):
    from sip_optimal_control_amd import BatchedChainLQR
    n, m, env, kwargs, tags, entry = CHAINS[family]
    cell = hi.chain_cell(n, m, axis)
    T = cell.shape[2]
    with _env(**env):
        s = BatchedChainLQR(n, m, T, hi.BATCH, **kwargs)
    assert all(t in s.kernel_name for t in tags) and s.kernel_name.count("/f64") == 1, (s.kernel_name, tags)
    assert family not in NO_SEP or SEP not in s.kernel_name
    mats, vecs = _dev(cell.mats), _dev(cell.vecs)
    if kwargs.get("symmetric"):
        mats = mats[:, torch.from_numpy(s.shape.pack_index()).to("cuda:0")].contiguous()
    if entry == "multi":
        cols = hi.CHAINS_F64[(n, m)]
        assert cell.ncols == cols and (s.solve_multi_workspace_bytes(cols) > 0), "no multi-rhs sweep on this plan"
        gains, status = s.factor(mats)
        sol_cols = s.solve_multi(mats, _dev(np.stack([c["vecs"] for c in cell.columns])), gains)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(status.cpu().numpy(), cell.ref_status)
        _judge_columns(family, cell, cg.host(sol_cols), hi.COL_PROBLEMS)
        return
    if entry == "fused":
        sol, gains, status = s.factor_solve(mats, vecs)
    elif entry == "split":
        assert s.has_split
        qmr, ab = s.split_inputs(mats)
        sol, gains, status = s.factor_solve_split(qmr, ab, vecs)
    else:
        gains, status = s.factor(mats)
        sol = s.solve(mats, vecs, gains)
    torch.cuda.synchronize()
    sol, gains = cg.host(sol), cg.host(gains)
    _judge_f64(family, cell, sol, status.cpu().numpy(), gains, _u_from_gains_chain(n, m, T, sol, gains))


# ---- trees, fp64 -------------------------------------------------------------------------------------------------
def _u_from_gains_tree(topo, sol, gains):
    lay, worst = topo.layout, 0.0
    for b in range(sol.shape[0]):
        err = scale = 0.0
        for e in range(topo.E):
            np_, _, m = topo.edge_dims(e)
            o = lay.gains_off[e]
            K, k = gains[b, o:o + m * np_].reshape((m, np_), order="F"), gains[b, o + m * np_:o + m * np_ + m]
            x = sol[b, lay.x_off[topo.parents[e]]:lay.x_off[topo.parents[e]] + np_]
            u = sol[b, lay.u_off[e]:lay.u_off[e] + m]
            err, scale = max(err, np.abs(u - (K @ x + k)).max()), max(scale, np.abs(u).max())
        worst = max(worst, err / scale)
    return worst


TREE_FAMILIES = ["tree fused factor_solve", "tree factor_fused + solve_fused", "tree solve_multi(3)", "tree general engine"]


@pytest.mark.parametrize("axis", hi.AXES_TREE)
@pytest.mark.parametrize("dims", hi.TREES, ids=lambda d: "<%d,%d>" % d)
@pytest.mark.parametrize("family", TREE_FAMILIES)
def test_hard_tree_f64(family, dims, axis):
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    cell = hi.tree_cell(*dims, axis)
    topo, cls = cell.topo, "<%d,%d>" % dims
    assert sum(1 for n in topo.sd if n == 0) == 2 and max(topo.sd) == dims[0] and max(topo.cd) == dims[1]
    with _env(**({"SIP_LQR_TREE": "general"} if family == "tree general engine" else {})):
        s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=hi.BATCH)
    maps = fb.PlanMaps(s, topo)
    s.input.copy_(torch.from_numpy(maps.pack_input(s, cell.nodes, cell.edges)))
    name = family + " " + cls
    if family == "tree solve_multi(3)":
        assert s.multi_kernel_name == "tree_solve_mrhs_qw16" + cls + "/f64", s.multi_kernel_name
        status = s.factor()
        out = s.solve_multi(_dev(np.stack([maps.pack_rhs(s, c) for c in cell.columns])))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(status.cpu().numpy(), cell.ref_status)
        _judge_columns(name, cell, out.cpu().numpy()[:, :, maps.sol_idx], hi.BATCH)
        return
    if family == "tree fused factor_solve":
        assert s.kernel_name == "tree_factor_solve_qw16" + cls + "/f64", s.kernel_name
        s.factor_solve()
    elif family == "tree factor_fused + solve_fused":
        assert s.split_kernel_name == "tree_factor_qw16{0}/f64 + tree_solve_qw16{0}/f64".format(cls), s.split_kernel_name
        s.factor_fused()
        s.solve_fused()
    else:
        assert s.kernel_name == "tree_generic/f64" and s.split_kernel_name == "tree_generic/f64", s.kernel_name
        s.factor()
        s.solve()
    torch.cuda.synchronize()
    sol, gains = s.output.cpu().numpy()[:, maps.sol_idx], s.work.cpu().numpy()[:, maps.gains_idx]
    _judge_f64(name, cell, sol, s.status.cpu().numpy(), gains, _u_from_gains_tree(topo, sol, gains))


# ---- chains, fp32 ------------------------------------------------------------------------------------------------
CHAINS_F32 = {
    "mt16/f32 fused (32,8)": (32, 8, {}, {}, ("mt16<32,8,",), "fused"),
    "mt16/f32 separate sweeps (32,8)": (32, 8, {}, {"separate_sweeps": True}, ("mt16<32,8,", SEP), "factor_solve"),
    "mf32 (32,8)": (32, 8, {"SIP_LQR_VARIANT": "mf32"}, {}, ("chain_factor_solve_mf32<32,8,",), "fused"),
    "qf32 (12,4)": (12, 4, {}, {"fused_f32": True}, ("qf32<12,4,",), "fused"),
    "qf32 odd (5,3)": (5, 3, {}, {"fused_f32": True}, ("qf32<5,3,",), "fused"),
}
E_GENERAL_CAP = 1e-2


def _run_f32(cell, env, kwargs, entry):
    from sip_optimal_control_amd import BatchedChainLQR
    n, m, T = cell.shape
    with _env(**env):
        s = BatchedChainLQR(n, m, T, hi.BATCH, dtype=torch.float32, **kwargs)
    mats, vecs = _dev(cell.mats, torch.float32), _dev(cell.vecs, torch.float32)
    assert np.array_equal(cg.host(mats), cell.mats)          # the cell is the rounded problem
    if entry == "fused":
        sol, _, status = s.factor_solve(mats, vecs)
    else:
        gains, status = s.factor(mats)
        sol = s.solve(mats, vecs, gains)
    torch.cuda.synchronize()
    return s.kernel_name, cg.host(sol), status.cpu().numpy()


def _e_general(cell):
    """e of the general fp32 engine on the cell, once per cell."""
    if not hasattr(cell, "e_general"):
        name, sol, status = _run_f32(cell, {"SIP_LQR_VARIANT": "general"}, {}, "fused")
        assert name == GENERAL + "/f32", name
        np.testing.assert_array_equal(status, cell.ref_status)
        cell.e_general = xr.err(sol, cell.ext)
    return cell.e_general


XFAIL_F32 = {("mt16/f32 fused (32,8)", "delta[1e-1,1e2]"): "e_gpu 2.3e-2 against e_general 2.4e-6: the fused fp32 sweep of F "
                                                           "is not scaled to a unit diagonal (DESIGN 7)"}


@pytest.mark.parametrize("family,axis", [
    pytest.param(f, a, marks=[pytest.mark.xfail(strict=True, reason=XFAIL_F32[(f, a)])] if (f, a) in XFAIL_F32 else [])
    for f in CHAINS_F32 for a in hi.AXES_F32])
def test_hard_chain_f32(family, axis):
    n, m, env, kwargs, tags, entry = CHAINS_F32[family]
    cell = hi.chain_cell(n, m, axis, "f32")
    e_general = _e_general(cell)
    name, sol, status = _run_f32(cell, env, kwargs, entry)
    assert all(t in name for t in tags) and name.count("/f32") == 1, (name, tags)
    np.testing.assert_array_equal(status, cell.ref_status)
    e_gpu = xr.err(sol, cell.ext)
    _report(family, axis, e_gpu, e_general)
    assert e_general <= E_GENERAL_CAP, (axis, e_general)
    assert e_gpu <= cg.F32_TOL + 3 * e_general, (family, axis, e_gpu, e_general)

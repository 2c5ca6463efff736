"""The n = 32 matrix-core kernels for 12 and 16 controls (wide_controls=True) over the regularization and scaling range
of tests/hard_inputs.py, against an extended-precision solve of the dense KKT system (tests/extended_reference.py);
notation and rules as in tests/test_gpu_hard_inputs.py.

fp64: the cell hard_inputs.chain_cell(17, 9, axis) of every axis of AXES_F64 -- the shape that test meets on the general
engine -- now embedded in mt16<32,12>, through the fused sweep and through the separate sweeps:
e_gpu <= 1e-9 + 3 e_ref, u = K x + k to 1e-9, the gains to 1e-9 + 3 e_ref_gains.

fp32: a cell of this test's own at (32, 16), T = 6, 3 problems, built as chain_cell builds its cells (the benign draw,
the axis applied through chain_views, rounded to fp32 before anything is solved), over AXES_F32, fused and separate
sweeps: e_gpu <= F32_TOL + 3 e_general with e_general <= 1e-2, e_general the general fp32 engine on the same inputs.
delta[1e-1,1e2] is the axis the fused fp32 (32, 8) kernel fails (it sweeps F as it stands); the wide rows scale F to a
unit diagonal in both precisions and are held to the rule there as everywhere.  The conditions that keep the fp32 cell
meaningful are checked without a GPU: the dense reference's last refinement step moved it by <= 1e-12 and every status
of the CPU oracle is 0."""
import contextlib
import os

import numpy as np
import pytest

import chain_guards as cg
import extended_reference as xr
import hard_inputs as hi

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

CAP = 1e-9
E_GENERAL_CAP = 1e-2
CORRECTION_CAP = 1e-12
SEP = " + chain_factor_mt16 + chain_solve_mt16"
GENERAL = "tree_generic(chain layout)"
N32, M32, T32 = 32, 16, 6


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


def _report(family, axis, e_gpu, yardstick, *more):
    print(f"HARD | {family} | {axis} | {e_gpu:.1e} | {yardstick:.1e}" + "".join(f" | {v:.1e}" for v in more))


def _u_from_gains(n, m, T, sol, gains):
    """max |u - (K x + k)| / max |u| per problem, x and u the kernel's own (lqr.cpp:856-857)."""
    B, vs = sol.shape[0], 2 * n + m
    body = sol[:, :T * vs].reshape(B, T, vs)
    x, u = body[:, :, :n], body[:, :, 2 * n:]
    g = gains.reshape(B, T, m * n + m)
    K, k = g[:, :, :m * n].reshape(B, T, n, m), g[:, :, m * n:]      # K column-major m x n: (j, c) at c * m + j
    return float((np.abs(u - (np.einsum("btcj,btc->btj", K, x) + k)).max(axis=(1, 2)) / np.abs(u).max(axis=(1, 2))).max())


# ---- fp64: (17, 9) embedded in mt16<32,12> -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("axis", hi.AXES_F64)
@pytest.mark.parametrize("entry", ["fused", "separate sweeps"])
def test_hard_chain_f64(entry, axis):
    from sip_optimal_control_amd import BatchedChainLQR
    n, m = 17, 9
    cell = hi.chain_cell(n, m, axis)
    T = cell.shape[2]
    s = BatchedChainLQR(n, m, T, hi.BATCH, wide_controls=True, separate_sweeps=entry != "fused")
    want = "chain_factor_solve_mt16<32,12,mfma16x16x4>/f64 embedding (17,9)" + ("" if entry == "fused" else SEP)
    assert s.kernel_name == want, s.kernel_name
    mats, vecs = _dev(cell.mats), _dev(cell.vecs)
    if entry == "fused":
        sol, gains, status = s.factor_solve(mats, vecs)
    else:
        gains, status = s.factor(mats)
        sol = s.solve(mats, vecs, gains)
    torch.cuda.synchronize()
    sol, gains = cg.host(sol), cg.host(gains)
    np.testing.assert_array_equal(status.cpu().numpy(), cell.ref_status)
    family = f"mt16 wide {entry} (17,9)"
    e_gpu, e_gains, e_gains_ext = xr.err(sol, cell.ext), xr.err(gains, cell.ref_gains), xr.err(gains, cell.ext_gains)
    u_err = _u_from_gains(n, m, T, sol, gains)
    _report(family, axis, e_gpu, cell.e_ref, e_gains, e_gains_ext, cell.e_ref_gains, u_err)
    assert e_gpu <= CAP + 3 * cell.e_ref, (family, axis, e_gpu, cell.e_ref)
    assert u_err <= CAP, (family, axis, "u = K x + k", u_err)
    assert e_gains <= CAP + 3 * cell.e_ref_gains, (family, axis, "gains against the oracle's", e_gains, cell.e_ref_gains)
    assert e_gains_ext <= CAP + 3 * cell.e_ref_gains, (family, axis, "gains", e_gains_ext, cell.e_ref_gains)


# ---- fp32: a cell at (32, 16) ---------------------------------------------------------------------------------------
class Cell32:
    pass


def cell_f32(axis):
    """The fp32 cell (32, 16, T = 6) of `axis`, 3 problems: mats, vecs (rounded to fp32, stored as float64), the
    extended-precision solution of the rounded problem, the oracle's statuses and the size of the dense reference's
    last refinement step.  Cached: the fused and the separate case and the CPU check share one reference."""
    n, m, T = N32, M32, T32
    key = ("wide chain", n, m, T, axis, "f32")

    def make():
        from oracle import dense_kkt, oracle
        from sip_optimal_control_amd import ChainShape, synthetic
        mats, vecs = synthetic.make_chain_batch(ChainShape(n, m, T), hi.BATCH, seed=hi._seed(n, m, T) % 2**31,
                                                device="cpu", cross_term=0.01)
        mats, vecs = mats.numpy().copy(), vecs.numpy().copy()
        hi.apply(axis, hi.chain_views(n, m, T, mats), hi._seed(n, m, T))
        mats, vecs = mats.astype(np.float32).astype(np.float64), vecs.astype(np.float32).astype(np.float64)
        cell = Cell32()
        cell.key, cell.axis, cell.shape, cell.mats, cell.vecs = key, axis, (n, m, T), mats, vecs
        _, _, cell.ref_status = oracle.chain_batch(n, m, T, mats, vecs)
        ext, cell.correction = [], 0.0
        for b in range(hi.BATCH):
            blocks = dense_kkt.chain_blocks_from_packed(n, m, T, mats[b], vecs[b])
            sols, last = xr.Factored(list(range(T)), list(range(1, T + 1)), [n] * (T + 1), [m] * T, blocks).solve([None])
            ext.append(xr.chain_row(*sols[0]))
            cell.correction = max(cell.correction, last)
        cell.ext = np.stack(ext)
        return cell

    return xr.cached(key, make)


@pytest.mark.parametrize("axis", hi.AXES_F32)
def test_the_fp32_cell_is_meaningful(axis):
    cell = cell_f32(axis)
    print(f"wide chain {cell.shape} {axis} f32: last correction {cell.correction:.1e}")
    assert cell.ref_status.tolist() == [0] * hi.BATCH
    assert np.isfinite(cell.ext).all() and cell.ext.shape == cell.vecs.shape
    assert cell.correction <= CORRECTION_CAP, cell.correction
    assert np.array_equal(cell.mats, cell.mats.astype(np.float32).astype(np.float64))


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


@gpu
@pytest.mark.parametrize("axis", hi.AXES_F32)
@pytest.mark.parametrize("entry", ["fused", "separate sweeps"])
def test_hard_chain_f32(entry, axis):
    cell = cell_f32(axis)
    e_general = _e_general(cell)
    separate = entry != "fused"
    name, sol, status = _run_f32(cell, {}, {"wide_controls": True, "separate_sweeps": separate},
                                 "factor_solve" if separate else "fused")
    assert name == "chain_factor_solve_mt16<32,16,mfma16x16x4>/f32" + (SEP if separate else ""), name
    np.testing.assert_array_equal(status, cell.ref_status)
    e_gpu = xr.err(sol, cell.ext)
    _report(f"mt16/f32 wide {entry} (32,16)", axis, e_gpu, e_general)
    assert e_general <= E_GENERAL_CAP, (axis, e_general)
    assert e_gpu <= cg.F32_TOL + 3 * e_general, (entry, axis, e_gpu, e_general)

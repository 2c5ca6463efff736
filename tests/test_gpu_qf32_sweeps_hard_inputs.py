"""The separate sweeps of the fused fp32 chain kernel (chain_factor_qf32, chain_solve_cols_qf32) over the fp32 axes of
tests/hard_inputs.py: delta[1e-3,1e-1], delta[1e-1,1e2], cost[1,1e2], expanding.

The rule is the project's for every fp32 path (tests/test_gpu_hard_inputs.py): with `ext` the extended-
precision solve (tests/extended_reference.py) of the fp32-rounded problem and e(v) = max over the problems of
max |v - ext| / max |ext|, e_gpu <= F32_TOL + 3 e_general, where e_general is the general fp32 engine
(tree_generic(chain layout)/f32) on the same rounded inputs through the same entry points, and e_general <= 1e-2 keeps
the cell meaningful.  Families: factor + solve at (12, 4) and (5, 3), and factor + solve_multi(3) at (12, 4), whose three
columns are N(0, 1) right-hand sides rounded to fp32, each solved in extended precision for every problem of the cell.

Every test prints "HARD | family | axis | e_gpu | e_general"; DESIGN 7.1 holds the table of one run.  The fused qf32
kernel sits at 1.2e-6 to 5.0e-6 on these axes; a cell of the sweeps more than 3x its fused neighbour is a finding for
DESIGN 4.9.1, not a failure."""
import contextlib
import os

import numpy as np
import pytest

import chain_guards as cg
import extended_reference as xr
import hard_inputs as hi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = torch.float32
GENERAL = "tree_generic(chain layout)/f32"
SUFFIX = " + chain_factor_qf32 + chain_solve_qf32"
E_GENERAL_CAP = 1e-2
NCOLS = 3
FAMILIES = {
    "qf32 separate sweeps, factor + solve (12,4)": (12, 4, "factor_solve"),
    "qf32 separate sweeps, factor + solve (5,3)": (5, 3, "factor_solve"),
    "qf32 separate sweeps, solve_multi(3) (12,4)": (12, 4, "multi"),
}


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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype=F32)


def _plan(cell, sweeps):
    from sip_optimal_control_amd import BatchedChainLQR
    n, m, T = cell.shape
    if sweeps:
        s = BatchedChainLQR(n, m, T, hi.BATCH, dtype=F32, fused_f32=True, separate_sweeps=True)
        assert s.kernel_name == f"chain_factor_solve_qf32<{n},{m},direct>/f32" + SUFFIX, s.kernel_name
    else:
        with _env(SIP_LQR_VARIANT="general"):
            s = BatchedChainLQR(n, m, T, hi.BATCH, dtype=F32)
        assert s.kernel_name == GENERAL, s.kernel_name
    return s


def _columns(cell):
    """NCOLS right-hand sides of the cell's chain (fp32-rounded, as float64) and their extended-precision solutions:
    (vecs_cols [NCOLS, BATCH, vecs_len], ext [NCOLS][BATCH, vecs_len]); once per cell."""
    def make():
        from oracle import dense_kkt
        n, m, T = cell.shape
        rng = np.random.default_rng(9000 + 16 * n + m)
        cols = rng.normal(size=(NCOLS,) + cell.vecs.shape).astype(np.float32).astype(np.float64)
        topo = (list(range(T)), list(range(1, T + 1)), [n] * (T + 1), [m] * T)
        ext = [[None] * hi.BATCH for _ in range(NCOLS)]
        for b in range(hi.BATCH):
            blocks = dense_kkt.chain_blocks_from_packed(n, m, T, cell.mats[b], cell.vecs[b])
            rhs = [dense_kkt.chain_blocks_from_packed(n, m, T, cell.mats[b], cols[c, b]) for c in range(NCOLS)]
            sols, last = xr.Factored(*topo, blocks).solve([{k: r[k] for k in ("q", "c", "r")} for r in rhs])
            assert last <= 1e-12, last          # the refinement has converged: `ext` is a reference for fp32
            for c in range(NCOLS):
                ext[c][b] = xr.chain_row(*sols[c])
        return cols, [np.stack(e) for e in ext]
    return xr.cached(("qf32 sweeps columns",) + cell.key, make)


def _run(cell, sweeps, entry):
    """-> e of the plan on the cell through the family's entry points."""
    s = _plan(cell, sweeps)
    mats, vecs = _dev(cell.mats), _dev(cell.vecs)
    assert np.array_equal(cg.host(mats), cell.mats)          # the cell is the rounded problem
    gains, status = s.factor(mats)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), cell.ref_status)
    if entry == "factor_solve":
        sol = s.solve(mats, vecs, gains)
        torch.cuda.synchronize()
        return xr.err(cg.host(sol), cell.ext)
    cols, ext = _columns(cell)
    assert (s.solve_multi_workspace_bytes(NCOLS) > 0) == sweeps
    out = s.solve_multi(mats, _dev(cols), gains)
    torch.cuda.synchronize()
    return max(xr.err(cg.host(out[c]), ext[c]) for c in range(NCOLS))


@pytest.mark.parametrize("axis", hi.AXES_F32)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_hard_chain_qf32_sweeps(family, axis):
    n, m, entry = FAMILIES[family]
    cell = hi.chain_cell(n, m, axis, "f32")
    e_general = xr.cached(("qf32 sweeps e_general", entry) + cell.key, lambda: _run(cell, False, entry))
    e_gpu = _run(cell, True, entry)
    print(f"HARD | {family} | {axis} | {e_gpu:.1e} | {e_general:.1e}")
    assert e_general <= E_GENERAL_CAP, (axis, e_general)
    assert e_gpu <= cg.F32_TOL + 3 * e_general, (family, axis, e_gpu, e_general)

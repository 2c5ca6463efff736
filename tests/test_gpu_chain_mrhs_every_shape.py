"""Every instantiation of the chain multi-right-hand-side sweep (chain_mrhs.hpp: chain_solve_mrhs_qw16) against the
oracle, taken from the manifest (csrc/gen_qw16_kernels.py): the default kernel of all 128 shapes n <= 16, m <= 8
and the direct-load alternates, which are the WPACK = false form at n < 16.

Per shape batch = 6 (one full wavefront and a ragged one: the `p = batch - 1` clamp), 11 columns (a launch of
eight, then one of three whose column workspace has stride 3, so every `col < ncols` predicate sees a full and a
partial group) and one problem with an indefinite R.  Every column of every good problem to the project's fp64
bound, 1e-9 max-abs relative per problem, against the oracle's solve of that column; the column workspace is the
size the kernel indexes; K of the gains, mats and the right-hand sides are bitwise left alone; the single-column
solve still works on the same factor state."""
import importlib.util
import os

import numpy as np
import pytest

from test_gpu_general_chain import _rel

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location(
    "gen_qw16_kernels", os.path.join(ROOT, "sip_optimal_control_amd", "csrc", "gen_qw16_kernels.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

MRHS = [e for s in gen.manifest() for e in s if e.mrhs]
# the first entry of a shape in its slice is the one find_kernel takes; the others need SIP_LQR_VARIANT
DEFAULT, ALTERNATES = {}, []
for _e in MRHS:
    if (_e.n, _e.m) in DEFAULT:
        ALTERNATES.append(_e)
    else:
        DEFAULT[(_e.n, _e.m)] = _e
TOL = 1e-9
BATCH, BAD = 6, 2
KEPT_SHAPE = (12, 4)  # its run is kept for test_the_checks_reject_...
_kept = {}


def _tag(e):
    return "staged" if e.staged else "direct"


def _bits(t):
    return t.view(torch.int64)


def _run(oracle_lib, n, m, T, cols, tag):
    """factor, solve_multi of `cols` columns and a solve of column 0 on the exact kernel of (n, m), every assertion
    of this file's docstring; returns (sol_cols, the oracle's columns, good problems, worst relative error)."""
    from sip_optimal_control_amd import BatchedChainLQR, ChainShape, synthetic
    shape = ChainShape(n, m, T)
    mats, _ = synthetic.make_chain_batch(shape, BATCH, seed=8000 + 10 * n + m, cross_term=0.01)
    off = shape.mats_off(min(1, T - 1))["R"]
    mats[BAD, off:off + m * m] = -1e4 * torch.eye(m, dtype=torch.float64).reshape(-1)  # G not positive definite
    vecs_cols = torch.randn(cols, BATCH, shape.vecs_len, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    mats_h, vecs_h = mats.numpy(), vecs_cols.numpy()
    mats, vecs_cols = mats.to("cuda:0"), vecs_cols.to("cuda:0")
    mats_before, vecs_before = mats.clone(), vecs_cols.clone()

    solver = BatchedChainLQR(n, m, T, BATCH)
    name = solver.kernel_name
    assert f"qw16<{n},{m}," in name and tag in name and "embedding" not in name, name
    for c in (1, 8, 11):  # cws[problem][node][col][g | h | k], `min(c, 8)` columns per launch
        assert solver.solve_multi_workspace_bytes(c) == BATCH * 8 * (T + 1) * min(c, 8) * (2 * n + m), (n, m, c)
    gains, status = solver.factor(mats)
    torch.cuda.synchronize()
    gains_before = gains.clone()
    sol_cols = solver.solve_multi(mats, vecs_cols, gains)
    one = solver.solve(mats, vecs_cols[0].contiguous(), gains)
    torch.cuda.synchronize()

    st = status.cpu().numpy()
    refs = []
    for col in range(cols):
        ref_sol, _, ref_status = oracle_lib.chain_batch(n, m, T, mats_h, vecs_h[col])
        np.testing.assert_array_equal(st, ref_status)
        refs.append(ref_sol)
    refs = np.stack(refs)
    ok = st == 0
    assert list(np.flatnonzero(~ok)) == [BAD], (n, m, st)
    got = sol_cols.cpu().numpy()
    worst = 0.0
    for col in range(cols):
        err = _rel(got[col][ok], refs[col][ok])
        assert err <= TOL, (n, m, col, err)
        worst = max(worst, err)
    err = _rel(one.cpu().numpy()[ok], refs[0][ok])  # the single-rhs entry point on the same factor state
    assert err <= TOL, (n, m, "solve after solve_multi", err)
    worst = max(worst, err)
    # only the k part of the gains is unspecified afterwards (include/sip_lqr_amd.h)
    K = lambda g: g.view(BATCH, T, shape.gain)[:, :, :m * n].contiguous()
    assert torch.equal(_bits(K(gains)), _bits(K(gains_before))), (n, m, "K of gains changed")
    assert torch.equal(_bits(mats), _bits(mats_before)) and torch.equal(_bits(vecs_cols), _bits(vecs_before)), (n, m)
    return got, refs, ok, worst


@pytest.mark.parametrize("n", sorted({n for n, _ in DEFAULT}))
def test_every_default_multi_rhs_kernel_matches_the_oracle(oracle_lib, n):
    worst = 0.0
    ms = sorted(m for nn, m in DEFAULT if nn == n)
    for m in ms:
        T = 3 + (n + m) % 5
        got, refs, ok, err = _run(oracle_lib, n, m, T, 11, _tag(DEFAULT[(n, m)]))
        worst = max(worst, err)
        if (n, m) == KEPT_SHAPE:
            _kept["run"] = (got, refs, ok)
    print(f"chain multi-rhs n = {n}, m in {ms}: worst relative error {worst:.2e} (bound {TOL:.0e})")


@pytest.mark.parametrize("n,m", [(e.n, e.m) for e in ALTERNATES])
def test_direct_alternates_below_16(oracle_lib, monkeypatch, n, m):
    """WPACK = false (the factor state a direct-load kernel leaves: full S squares in the spill) at n < 16."""
    (e,) = [a for a in ALTERNATES if (a.n, a.m) == (n, m)]
    assert not e.staged and n < 16
    monkeypatch.setenv("SIP_LQR_VARIANT", _tag(e))
    _, _, _, worst = _run(oracle_lib, n, m, 3 + (n + m) % 5, 11, "direct")
    print(f"chain multi-rhs direct ({n},{m}): worst relative error {worst:.2e} (bound {TOL:.0e})")


@pytest.mark.parametrize("n,m", [(16, 8), (15, 8), (1, 1)])
def test_one_edge(oracle_lib, n, m):
    """T = 1: each of the double-buffered backward and forward loops runs exactly once."""
    _, _, _, worst = _run(oracle_lib, n, m, 1, 8, _tag(DEFAULT[(n, m)]))
    print(f"chain multi-rhs ({n},{m}) T = 1: worst relative error {worst:.2e} (bound {TOL:.0e})")


def test_every_manifest_entry_is_enumerated():
    """The three tests above are parametrized from these lists: together they are the manifest's multi-rhs entries."""
    assert sorted(list(DEFAULT.values()) + ALTERNATES) == sorted(MRHS)
    assert len(DEFAULT) + len(ALTERNATES) == len(MRHS) and len(set(MRHS)) == len(MRHS)
    assert all(not e.sym for e in MRHS)  # the full layout: the plans above find them


def test_the_checks_reject_a_neighbouring_column_and_a_perturbed_entry(oracle_lib):
    """Sensitivity of the comparison itself on a run the test above made (made here when this test runs alone): the
    GPU's column c against the oracle's column c + 1 is rejected, and so is a copy of the GPU's columns with one entry
    scaled by 1 + 1e-8."""
    if "run" not in _kept:
        n, m = KEPT_SHAPE
        _kept["run"] = _run(oracle_lib, n, m, 3 + (n + m) % 5, 11, _tag(DEFAULT[KEPT_SHAPE]))[:3]
    got, refs, ok = _kept["run"]
    cols = got.shape[0]
    for col in range(cols):
        assert _rel(got[col][ok], refs[col][ok]) <= TOL
        assert _rel(got[col][ok], refs[(col + 1) % cols][ok]) > TOL, col  # a column in the wrong slot
    good = np.flatnonzero(ok)
    for col, p in ((0, good[0]), (cols - 1, good[-1])):
        k = int(np.abs(refs[col][p]).argmax())
        bad = got.copy()
        bad[col, p, k] *= 1.0 + 1e-8
        assert not (_rel(bad[col][ok], refs[col][ok]) <= TOL), (col, p)
    nan = got.copy()
    nan[3, good[1], 0] = np.nan
    assert not (_rel(nan[3][ok], refs[3][ok]) <= TOL)

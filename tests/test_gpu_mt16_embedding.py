"""fp64: every shape without an exact kernel that is embedded in the n = 32 matrix-core kernel
(chain_factor_solve_mt16<32, M>/f64): n = 17 .. 31 with m = 1 .. 8, and n = 32 with m not in {4, 8}.  The repack
around the sweep (pad_mats_kernel, pad_vecs_kernel, unpad_gains_kernel and the float-reciprocal index arithmetic of
div_small in sip_lqr_amd.hip) meets every such shape here, with failing problems in the batch: an indefinite R, an
indefinite Q and a zero delta at the LAST real state, the entry next to the padded delta = 1 ones.

Tolerance as everywhere in fp64: 1e-9 max-abs relative to the oracle's row of that problem, statuses exact."""
import numpy as np
import pytest

import chain_guards as cg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = cg.F64_TOL
F64 = torch.float64
BAD_R, BAD_DELTA, BAD_Q = 2, 4, 7        # problems of a batch of 9 that fail (rows of different wavefronts' worth)


def _solver(n, m, T, batch):
    from sip_optimal_control_amd import BatchedChainLQR
    s = BatchedChainLQR(n, m, T, batch)
    host = "mt16<32,4" if m <= 4 else "mt16<32,8"           # find_embedding_kernel: least N, then least M
    assert "embedding" in s.kernel_name and host in s.kernel_name and "/f64" in s.kernel_name, s.kernel_name
    return s


def _inject(n, m, T, mats):
    from sip_optimal_control_amd import ChainShape
    shape = ChainShape(n, m, T)
    expected = [0] * mats.shape[0]
    o = shape.mats_off(1)["R"]
    mats[BAD_R, o:o + m * m] = -1e4 * torch.eye(m, dtype=F64, device=mats.device).reshape(-1)
    expected[BAD_R] = 3
    mats[BAD_DELTA, shape.mats_off(T)["delta"] + n - 1] = 0.0          # the last real state of the last node
    expected[BAD_DELTA] = 1
    o = shape.mats_off(T)["Q"]
    mats[BAD_Q, o:o + n * n] = -1e4 * torch.eye(n, dtype=F64, device=mats.device).reshape(-1)
    expected[BAD_Q] = 2
    return expected


def _shape_against_the_oracle(oracle_lib, n, m, cols=0):
    T, batch = 3 + (n + m) % 5, 9
    mats, vecs = cg.make(n, m, T, batch, seed=8000 + 10 * n + m, dtype=F64)
    expected = _inject(n, m, T, mats)
    solver = _solver(n, m, T, batch)
    sol, gains, status = solver.factor_solve(mats, vecs)
    status = status.clone()                                 # factor() reports into the same tensor
    g2, st2 = solver.factor(mats)
    s2 = solver.solve(mats, vecs, g2)
    torch.cuda.synchronize()
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert list(ref_status) == expected, (n, m)            # the oracle agrees with the construction
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status, err_msg=str((n, m)))
    np.testing.assert_array_equal(st2.cpu().numpy(), ref_status, err_msg=str((n, m)))
    ok = ref_status == 0
    assert ok.sum() == batch - 3
    worst = 0.0
    for got_s, got_g in ((sol, gains), (s2, g2)):
        worst = max(worst, cg.assert_close(cg.host(got_s)[ok], ref_sol[ok], TOL, (n, m, "sol")),
                    cg.assert_close(cg.host(got_g)[ok], ref_gains[ok], TOL, (n, m, "gains")))
    if cols:
        gen = torch.Generator(device="cuda:0").manual_seed(n + m)
        vecs_cols = torch.randn(cols, batch, solver.shape.vecs_len, dtype=F64, device="cuda:0", generator=gen)
        assert solver.solve_multi_workspace_bytes(cols) == 0               # column by column
        sol_cols = solver.solve_multi(mats, vecs_cols, g2)
        torch.cuda.synchronize()
        for col in range(cols):
            ref_col, _, st = cg.oracle_of(oracle_lib, n, m, T, mats, vecs_cols[col])
            np.testing.assert_array_equal(st, ref_status)
            worst = max(worst, cg.assert_close(cg.host(sol_cols[col])[ok], ref_col[ok], TOL, (n, m, "column", col)))
    return worst


@pytest.mark.parametrize("n", list(range(17, 33)))
def test_every_shape_embedded_in_mt16_matches_the_oracle(oracle_lib, n):
    """Fused and split entry points of every embedded (n, m), three failing problems in each batch of nine."""
    worst = max(_shape_against_the_oracle(oracle_lib, n, m) for m in range(1, 9) if not (n == 32 and m in (4, 8)))
    print(f"mt16/f64 embedding n = {n}: worst error over m {worst:.2e}")


@pytest.mark.parametrize("n,m", [(17, 8), (25, 4), (31, 1), (32, 6)])
def test_solve_multi_on_an_embedded_shape(oracle_lib, n, m):
    worst = _shape_against_the_oracle(oracle_lib, n, m, cols=3)
    print(f"mt16/f64 embedding ({n},{m}) with 3 columns: worst error {worst:.2e}")


@pytest.mark.parametrize("T", [0, 1])
def test_embedded_shape_at_the_shortest_horizons(oracle_lib, T):
    n, m, batch = 24, 5, 1
    mats, vecs = cg.make(n, m, T, batch, seed=8900 + T, dtype=F64)
    solver = _solver(n, m, T, batch)
    sol, gains, status = (t.clone() for t in solver.factor_solve(mats, vecs))
    g2, st2 = solver.factor(mats)
    s2 = solver.solve(mats, vecs, g2)
    torch.cuda.synchronize()
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, mats, vecs)
    assert (ref_status == 0).all()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    np.testing.assert_array_equal(st2.cpu().numpy(), ref_status)
    for got_s, got_g in ((sol, gains), (s2, g2)):
        cg.assert_close(cg.host(got_s), ref_sol, TOL, (T, "sol"))
        cg.assert_close(cg.host(got_g), ref_gains, TOL, (T, "gains"))

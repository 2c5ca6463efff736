"""The refinement scheme of sip_lqr_refine restated in numpy, on the cells tests/test_gpu_refine.py runs it on: the check
that those inputs are fair.  Recursion in float32 (fp32 cells) or float64 (fp64 cells), residual and iterate in
float64 (refine_cases.model_refine), starting from zero; after the GPU test's number of rounds the iterate must meet
the GPU test's cap e <= 1e-9 + 3 e_ref against the extended-precision solve.  The model's inner solver forms
W = (I + V Delta)^-1 V, which does not cancel at a tiny delta; the kernels' W = D^-1/2 (I - F^-1) D^-1/2 does -- the
model shows what the scheme can reach on these inputs, not what a kernel does reach.

Every test prints "MODEL | dtype | (n,m) | axis | e by round | e_ref"."""
import numpy as np
import pytest

import extended_reference as xr
import hard_inputs as hi
import refine_cases as rc


def _run(n, m, axis, dtype, np_dtype, iterations):
    cell = hi.chain_cell(n, m, axis, dtype)
    iterates, norms = rc.model_refine(cell, iterations, np_dtype)
    errs = [xr.err(z, cell.ext) for z in iterates]
    print(f"MODEL | {dtype} | ({n},{m}) | {axis} | " + " ".join(f"{e:.1e}" for e in errs) + f" | {cell.e_ref:.1e}")
    assert errs[-1] <= rc.CAP + 3 * cell.e_ref, (dtype, n, m, axis, errs, cell.e_ref)
    return cell, iterates, norms


@pytest.mark.parametrize("axis", hi.AXES_F32)
@pytest.mark.parametrize("n,m", rc.CELLS_F32)
def test_model_meets_the_cap_on_the_fp32_cells(n, m, axis):
    _, _, norms = _run(n, m, axis, "f32", np.float32, rc.ITERATIONS_F32)
    assert (norms[1] <= norms[0]).all(), norms


@pytest.mark.parametrize("axis", hi.AXES_F64)
@pytest.mark.parametrize("n,m", rc.CELLS_F64)
def test_model_meets_the_cap_on_the_fp64_cells(n, m, axis):
    _run(n, m, axis, "f64", np.float64, rc.ITERATIONS_F64)


def test_the_numpy_residual_vanishes_at_the_extended_solution():
    """refine_cases.residual states the system the extended reference solves: at its solution the residual is at the
    rounding of the solution to fp64, far below the right-hand side."""
    cell = hi.chain_cell(12, 4, hi.BENIGN)
    n, m, T = cell.shape
    rho, mag = rc.residual(n, m, T, cell.mats, cell.vecs, cell.ext)
    assert (np.abs(rho) <= 4 * 2.0 ** -53 * mag).all(), float((np.abs(rho) / mag).max())
    assert np.abs(rho).max() < 1e-12 * np.abs(cell.vecs).max()


def test_scale_is_the_power_of_two_below_the_norm():
    norms = np.array([0.0, 1.0, 1.5, 2.0, 3e-7, 5e300, 4.9e-324, np.inf, np.nan])
    s = rc.scale_of(norms)
    np.testing.assert_array_equal(s, [1.0, 1.0, 1.0, 2.0, 2.0 ** -22, 2.0 ** 998, 4.9e-324, 1.0, 1.0])

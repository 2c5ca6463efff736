"""The references of tests/test_gpu_hard_inputs.py, checked without a GPU: the extended-precision solve
(tests/extended_reference.py) and, for every (shape, axis) cell the GPU tests use, the conditions that keep the cell
meaningful: the reference's last refinement correction <= 1e-12, every status of the CPU oracle 0, and
e_ref = e(oracle against the extended solve) <= 1e-7 -- the kernels are asked for 1e-9 + 3 e_ref, which says nothing
where the reference algorithm itself has lost the problem.  Likewise for the gains: e_ref_gains <= 1e-7 against the
long-double recursion, and that recursion and the dense solve, which share no code path, agree through
u_e = K_e x_parent(e) + k_e to 1e-12 of max |sol|."""
import numpy as np
import pytest

import extended_reference as xr
import hard_inputs as hi
from oracle import dense_kkt

E_REF_CAP = 1e-7
CORRECTION_CAP = 1e-12


def test_long_double_is_the_extended_type():
    assert np.finfo(np.longdouble).eps <= 1.1e-19


@pytest.mark.parametrize("kind,shape", [("chain", (12, 4)), ("chain", (32, 8)), ("tree", (15, 8))])
def test_extended_solve_agrees_with_the_fp64_dense_solve_on_the_benign_axis(kind, shape):
    cell = hi.cell_of(kind, shape, hi.BENIGN, "f64")
    for b in range(hi.BATCH):
        if kind == "chain":
            n, m, T = cell.shape
            args = (list(range(T)), list(range(1, T + 1)), [n] * (T + 1), [m] * T,
                    dense_kkt.chain_blocks_from_packed(n, m, T, cell.mats[b], cell.vecs[b]))
            dense = xr.chain_row(*dense_kkt.solve(*args))
        else:
            t = cell.topo
            dense = xr.tree_row(*dense_kkt.solve(t.parents, t.children, t.sd, t.cd, hi.fb.problem(cell.blocks, b)))
        assert xr.err(dense[None], cell.ext[b][None]) <= 1e-9


def test_lu_solves_a_matrix_that_needs_pivoting():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(40, 40))
    A[np.arange(0, 40, 3), np.arange(0, 40, 3)] = 0.0           # zero pivots without row exchanges
    X = rng.normal(size=(40, 2))
    LU, order = xr.lu_factor(A.astype(xr.LD))
    got = xr.lu_solve(LU, order, (A.astype(xr.LD) @ X.astype(xr.LD)))
    assert float(np.abs(got - X).max()) <= 1e-14


def test_axes_are_seeded_and_do_what_they_say():
    a, b = hi.chain_cell(12, 4, "cost_delta"), hi.chain_cell(12, 4, hi.BENIGN)
    n, m, T = a.shape
    va, vb = hi.chain_views(n, m, T, a.mats), hi.chain_views(n, m, T, b.mats)
    assert all(1e-9 <= d.min() and d.max() <= 1e-7 for d in va["delta"])
    assert all(np.array_equal(x, y) for k in ("A", "B", "M", "R") for x, y in zip(va[k], vb[k]))
    grown = [np.diagonal(x - y, axis1=1, axis2=2) for x, y in zip(va["Q"], vb["Q"])]
    assert min(g.min() for g in grown) > 0 and max(g.max() for g in grown) > 1e3
    e = hi.chain_views(n, m, T, hi.chain_cell(12, 4, "expanding").mats)
    for A in e["A"]:
        np.testing.assert_allclose(A.transpose(0, 2, 1) @ A, 2.25 * np.broadcast_to(np.eye(n), A.shape), atol=1e-12)
    xr._CACHE.pop(a.key)
    again = hi.chain_cell(12, 4, "cost_delta")
    assert again is not a and np.array_equal(again.mats, a.mats) and np.array_equal(again.ext, a.ext)
    f = hi.chain_cell(5, 3, "cost[1,1e2]", "f32")
    assert np.array_equal(f.mats, f.mats.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("kind,shape,axis,dtype", hi.cells(), ids=lambda v: str(v).replace(" ", ""))
def test_cell_is_meaningful(kind, shape, axis, dtype):
    cell = hi.cell_of(kind, shape, axis, dtype)
    print(f"{kind} {shape} {axis} {dtype}: e_ref {cell.e_ref:.1e}, columns {cell.e_ref_cols:.1e}, gains "
          f"{cell.e_ref_gains:.1e}, last correction {cell.correction:.1e}, u = K x + k of the references {cell.gains_tie:.1e}")
    assert cell.ref_status.tolist() == [0] * hi.BATCH
    assert np.isfinite(cell.ext).all() and cell.ext.shape == cell.ref_sol.shape
    assert cell.correction <= CORRECTION_CAP, cell.correction
    assert max(cell.e_ref, cell.e_ref_cols) <= E_REF_CAP, (cell.e_ref, cell.e_ref_cols)
    assert cell.gains_tie <= CORRECTION_CAP and cell.e_ref_gains <= E_REF_CAP, (cell.gains_tie, cell.e_ref_gains)

"""Guard bands, a poisoned workspace, inputs left alone and order independence of the chain entry points, one small
case per kernel family (tests/chain_guards.py):

* sol, gains, status and the workspace are views inside larger buffers, 64 scalars of a finite sentinel on both
  sides; the workspace view is exactly sip_lqr_workspace_bytes long.  After factor_solve, factor, solve, solve_multi
  (and factor_solve_split where the plan has it) every guard is bitwise intact;
* the workspace is filled with NaN before factor_solve, factor and factor_solve_split: the results still match the
  oracle, so nothing is read from the workspace before the call has written it (not between factor and solve: the
  factor state lives there by contract);
* mats and vecs are bitwise what they were;
* a batch run again with its problems permuted gives the same bits, permuted.  mt16 and the general engine run one
  problem per workgroup: any permutation.  qw16 runs four problems per wavefront, one per 16-lane DPP row: whole
  groups of four are permuted (same bits required), and separately two problems inside a wavefront are swapped.
  For that swap only the oracle's 1e-9 is required: the staged kernels address the four problems of a wavefront
  through row-dependent LDS images and the status logic works on wave-wide masks, and reading the code does not
  PROVE that a row's position never reaches the order of a sum; whether the bits were equal is printed.

The reference is the CPU oracle throughout; T <= 9 everywhere."""
import numpy as np
import pytest

import chain_guards as cg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# id: (n, m, T, batch, dtype, environment, symmetric, what the kernel name must contain, tolerance, problems per wavefront)
FAMILIES = {
    "mt16_f32_m4": (32, 4, 5, 3, "f32", {}, False, ("mt16<32,4", "/f32"), cg.F32_TOL, 1),
    "mt16_f32_m8": (32, 8, 4, 3, "f32", {}, False, ("mt16<32,8", "/f32"), cg.F32_TOL, 1),
    "general_f32_lds": (12, 4, 9, 5, "f32", {}, False, ("tree_generic", "/f32"), cg.F32_TOL, 1),
    "general_f32_global": (52, 4, 4, 3, "f32", {}, False, ("tree_generic", "/f32"), cg.F32_TOL, 1),
    "mt16_f64_embedded": (20, 3, 6, 5, "f64", {}, False, ("mt16<32,4", "embedding", "/f64"), cg.F64_TOL, 1),
    "qw16_staged": (12, 4, 9, 5, "f64", {}, False, ("qw16<12,4,", "staged"), cg.F64_TOL, 4),
    "qw16_direct": (16, 3, 7, 5, "f64", {}, False, ("qw16<16,3,", "direct"), cg.F64_TOL, 4),
    "qw16_embedding": (13, 5, 8, 6, "f64", {"SIP_LQR_EXTRA": "0"}, False, ("<14,8,staged>", "embedding"), cg.F64_TOL, 4),
    "qw16_symmetric": (12, 4, 9, 5, "f64", {}, True, ("qw16<12,4,", "sym"), cg.F64_TOL, 4),
}


def _plan(name, batch=None):
    from sip_optimal_control_amd import BatchedChainLQR
    n, m, T, b, dt, _, sym, tags, _, _ = FAMILIES[name]
    s = BatchedChainLQR(n, m, T, batch or b, dtype=torch.float32 if dt == "f32" else torch.float64, symmetric=sym)
    assert all(t in s.kernel_name for t in tags), (s.kernel_name, tags)
    return s


def _inputs(name, batch, seed):
    """(mats as the plan reads them, full-layout mats for the oracle, vecs)."""
    n, m, T, _, dt, _, sym, _, _, _ = FAMILIES[name]
    full, vecs = cg.make(n, m, T, batch, seed=seed, dtype=torch.float32 if dt == "f32" else torch.float64)
    if not sym:
        return full, full, vecs
    from sip_optimal_control_amd import ChainShape
    idx = torch.from_numpy(ChainShape(n, m, T).packed().pack_index()).to(full.device)
    return full[:, idx].contiguous(), full, vecs


@pytest.mark.parametrize("name", list(FAMILIES))
def test_guards_poisoned_workspace_and_inputs(oracle_lib, monkeypatch, name):
    n, m, T, batch, _, env, _, _, tol, _ = FAMILIES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mats, full, vecs = _inputs(name, batch, seed=6000 + n + m)
    solver = _plan(name)
    g, es, eg, ek = cg.guarded_entry_points(solver, mats, vecs, oracle_lib, tol, ref_mats=full)
    assert solver.workspace.numel() * 4 == g.ws_bytes
    print(f"{name}: {solver.kernel_name}: workspace {g.ws_bytes} B, guards intact after every entry point, worst sol "
          f"{es:.2e}, gains {eg:.2e}, K of factor alone {ek:.2e} from a NaN-filled workspace")


@pytest.mark.parametrize("name", list(FAMILIES))
def test_results_do_not_depend_on_the_order_of_the_batch(oracle_lib, monkeypatch, name):
    n, m, T, _, _, env, _, _, tol, per_wave = FAMILIES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    batch = 8 if per_wave == 4 else 5
    mats, full, vecs = _inputs(name, batch, seed=6100 + n + m)
    solver = _plan(name, batch)
    ref_sol, ref_gains, ref_status = cg.oracle_of(oracle_lib, n, m, T, full, vecs)
    assert (ref_status == 0).all()
    perms = [[3, 0, 4, 2, 1]] if per_wave == 1 else [[4, 5, 6, 7, 0, 1, 2, 3]]
    for perm in perms:                              # whole workgroups / whole wavefronts move: the same bits
        same, (sol, gains, status, sol_p, gains_p, status_p) = cg.permuted_runs_agree(solver, mats, vecs, perm)
        assert bool((status == 0).all()) and bool((status_p == 0).all())
        cg.assert_close(cg.host(sol), ref_sol, tol, (name, "sol"))
        cg.assert_close(cg.host(gains), ref_gains, tol, (name, "gains"))
        assert same, (name, perm, "a problem's result depends on its position in the batch")
    if per_wave == 4:                               # two problems swap their rows inside wavefronts 0 and 1
        perm = [2, 1, 0, 3, 4, 7, 6, 5]
        same, (_, _, _, sol_p, gains_p, status_p) = cg.permuted_runs_agree(solver, mats, vecs, perm)
        assert bool((status_p == 0).all())
        cg.assert_close(cg.host(sol_p), ref_sol[perm], tol, (name, "sol, rows swapped"))
        cg.assert_close(cg.host(gains_p), ref_gains[perm], tol, (name, "gains, rows swapped"))
        print(f"{name}: rows swapped inside a wavefront: bitwise equal = {same}")


@pytest.mark.parametrize("name", ["general_f32_lds", "qw16_staged"])
def test_the_checks_reject_a_perturbed_gain_and_a_touched_guard(oracle_lib, name):
    """Sensitivity of the checks themselves, without touching a kernel: a copy of the GPU's gains with one entry
    scaled by 1 + 10 tol is rejected by the comparison, and a copy of every guarded buffer with one guard scalar
    changed is rejected by the guard check (the project's "a gain entry perturbed by 1e-4 is caught")."""
    n, m, T, batch, _, _, _, _, tol, _ = FAMILIES[name]
    mats, full, vecs = _inputs(name, batch, seed=6200 + n)
    solver = _plan(name)
    g, _, _, _ = cg.guarded_entry_points(solver, mats, vecs, oracle_lib, tol, ref_mats=full)
    solver.factor_solve(mats, vecs, g.sol, g.gains)          # (the last entry point above left the k of another rhs)
    torch.cuda.synchronize()
    _, ref_gains, _ = cg.oracle_of(oracle_lib, n, m, T, full, vecs)
    got = cg.host(g.gains)
    cg.assert_close(got, ref_gains, tol, "as computed")
    p = batch - 1
    k = int(np.abs(ref_gains[p]).argmax())
    bad = got.copy()
    bad[p, k] *= 1.0 + 10.0 * tol
    with pytest.raises(AssertionError):
        cg.assert_close(bad, ref_gains, tol, "one entry perturbed")
    nan = got.copy()
    nan[0, 0] = np.nan
    with pytest.raises(AssertionError):
        cg.assert_close(nan, ref_gains, tol, "one entry NaN")
    assert g.broken() == []
    for fname, frame in g.frames.items():
        guard = g.guards(fname)
        for at in (0, guard - 1, frame.numel() - guard, frame.numel() - 1):   # both ends of both guards
            touched = frame.clone()
            touched[at] = 0
            assert cg.frame_intact(frame, guard) and not cg.frame_intact(touched, guard), (fname, at)
    keep = g.frames["sol"][cg.GUARD - 1].clone()
    g.frames["sol"][cg.GUARD - 1] = 1.0                                         # the scalar just before sol
    assert g.broken() == ["sol"]
    g.frames["sol"][cg.GUARD - 1] = keep
    assert g.broken() == []

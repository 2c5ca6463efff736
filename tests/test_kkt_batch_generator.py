"""full_batch_problems.newton_kkt_batch, the vectorised Newton-KKT problem generator of the family and full-batch
GPU tests (tests/test_gpu_kkt_family.py), on the CPU: blocks of the right shapes at the offsets of the dimension
tables, the SPD blocks SPD, problems the oracle factors, neighbours that differ, and fast enough for the batches
the GPU tests draw."""
import os
import time

import numpy as np
import pytest

import full_batch_problems as fb
from oracle.kkt import KKTDims, KKTOracle
from tests import reference_kkt_problems as rk

torch = pytest.importorskip("torch")


def _dims(n, m, T, p):
    d = rk.newton_kkt_dims(n, m, T)
    return KKTDims(d.parents, d.children, d.sd, d.cd, d.ncd, d.ngd, d.ecd, d.egd, theta_dim=p)


def _assert_spd(a):
    np.testing.assert_allclose(a, a.T, rtol=0, atol=1e-12 * np.abs(a).max())
    assert np.linalg.eigvalsh(a).min() > 0


@pytest.mark.parametrize("case", ["family_theta", "family", "branching_theta"])
def test_generated_problem_unpacks_factors_and_discriminates(oracle_lib, case):
    if case == "branching_theta":  # a tree with varying dimensions and interior constraints
        dims = KKTDims([0, 0, 1, 1, 2, 4], [1, 2, 3, 4, 5, 6], [5, 4, 6, 3, 5, 4, 6], [2, 3, 1, 2, 2, 3],
                       node_c=[0, 1, 0, 2, 0, 1, 1], node_g=[1, 0, 2, 0, 1, 0, 2], edge_c=[1, 0, 2, 1, 0, 1],
                       edge_g=[0, 2, 1, 0, 1, 1], theta_dim=3)
    else:
        dims = _dims(8, 3, 13, 8 if case == "family_theta" else 0)
    B = 9
    out = [a.numpy() for a in fb.newton_kkt_batch(dims, B, seed=4, device="cpu")]
    model, w, r1, r2, r3, rhs = out[:6]
    assert len(out) == (7 if dims.p else 6)
    want = [dims.model_len, dims.z_dim, dims.x_dim + dims.p, dims.y_dim, dims.z_dim, dims.full_dim]
    assert [a.shape for a in out[:6]] == [(B, k) for k in want] and all(a.dtype == np.float64 for a in out)
    assert (w >= 1e-2).all() and (w <= 1e3).all() and (r3 >= 1e-3).all() and (r3 <= 1e1).all()
    assert (r2 >= 1e-3).all() and (r2 <= 1e2).all() and (r1 == 1e-8).all()
    q = 4
    nodes, edges = dims.unpack_model(model[q])
    for i in range(dims.N):
        assert [nodes[i][b].shape for b in ("d2L_dx2", "dc_dx", "dg_dx")] == dims.node_shapes(i)
        _assert_spd(nodes[i]["d2L_dx2"])
    for e in range(dims.E):
        ed = edges[e]
        assert [ed[b].shape for b in ("d2L_dx2", "d2L_dxdu", "d2L_du2", "ddyn_dx", "ddyn_du", "dc_dx", "dc_du",
                                      "dg_dx", "dg_du")] == dims.edge_shapes(e)
        _assert_spd(ed["d2L_du2"])
        assert (ed["d2L_dx2"] == 0).all()
        dev = ed["ddyn_dx"] - np.eye(*ed["ddyn_dx"].shape)
        assert 0 < np.abs(dev).max() < 0.5          # I + 0.05 N(0, 1)
    o = KKTOracle(dims)
    if dims.p:
        tn, te = dims.unpack_theta(out[6][q])
        assert [[tn[i][b].shape for b in tn[i]] for i in range(dims.N)] == \
            [dims.theta_node_shapes(i) for i in range(dims.N)]
        assert [[te[e][b].shape for b in te[e]] for e in range(dims.E)] == \
            [dims.theta_edge_shapes(e) for e in range(dims.E)]
        _assert_spd(tn[dims.E]["d2L_dtheta2"])
        assert np.linalg.eigvalsh(tn[dims.E]["d2L_dtheta2"]).min() >= 100.0 - 1e-9
        assert all((tn[i]["d2L_dtheta2"] == 0).all() for i in range(dims.E))
        assert all((te[e]["d2L_dtheta2"] == 0).all() for e in range(dims.E))
        assert 0 < np.abs(te[0]["ddyn_dtheta"]).max() < 1e-2
        ref = []
        for k in range(B):
            assert o.factor_theta(model[k], out[6][k], w[k], r1[k], r2[k], r3[k]) == 0, k
            ref.append(o.solve_theta(model[k], out[6][k], rhs[k]))
        ref = np.stack(ref)
    else:
        assert o.factor(model[q], w[q], r1[q], r2[q], r3[q]) == 0
        ref, st = o.batch(model, w, r1, r2, r3, rhs)
        assert (st == 0).all()
    fb.assert_discriminates(ref, 1e-9, what=case)
    # the same seed draws the same problems
    again = fb.newton_kkt_batch(dims, B, seed=4, device="cpu")
    assert all(np.array_equal(a, b.numpy()) for a, b in zip(out, again))


def test_generator_is_fast_enough():
    """The family tests draw 1031 problems at T = 13 with p = 8 per case: a fraction of a second unloaded.  The bound
    is loose (a shared CI host) but catches a per-problem Python loop, which takes tens of seconds here."""
    dims = _dims(12, 4, 13, 8)
    t0 = time.perf_counter()
    fb.newton_kkt_batch(dims, 1031, seed=1, device="cpu")
    dt = time.perf_counter() - t0
    print(f"newton_kkt_batch (12, 4, 13) p = 8, batch 1031: {dt:.3f} s")
    assert dt < 3.0


def test_oracle_threads(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert fb.oracle_threads() == min(3, len(os.sched_getaffinity(0)))
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert 1 <= fb.oracle_threads() <= 16
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert 1 <= fb.oracle_threads() <= 16

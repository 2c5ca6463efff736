"""The theta Schur complement (K^-1 J_theta, helpers.cpp:387) of Newton-KKT plans on trees and non-uniform
chains: all columns through one sip_lqr_tree_solve_multi, against the oracle and against the column-by-column
path (SIP_KKT_THETA_TREE_MULTI=0)."""
import numpy as np
import pytest
import torch

from oracle.kkt import KKTDims, KKTOracle
from tests import reference_kkt_problems as rk

pytestmark = pytest.mark.gpu


def _make(dims, batch):
    from sip_optimal_control_amd import BatchedNewtonKKT
    return BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                            batch=batch, root=dims.root, theta_dim=dims.p)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


def _dims(topology, p):
    if topology == "nonuniform_chain":
        T = 6
        sd, cd = [4, 6, 5, 3, 6, 4, 5], [2, 3, 1, 2, 3, 2]
        return KKTDims(list(range(T)), list(range(1, T + 1)), sd, cd, node_c=[1, 0, 2, 0, 1, 0, 2],
                       node_g=[0, 2, 0, 1, 0, 0, 3], edge_c=[1, 2, 0, 1, 1, 0], edge_g=[2, 0, 1, 1, 0, 2], theta_dim=p)
    parents, children = [0, 0, 1, 1, 2, 4], [1, 2, 3, 4, 5, 6]  # a branching tree
    sd, cd = [5, 4, 6, 3, 5, 4, 6], [2, 3, 1, 2, 2, 3]
    return KKTDims(parents, children, sd, cd, node_c=[0, 1, 0, 2, 0, 1, 1], node_g=[1, 0, 2, 0, 1, 0, 2],
                   edge_c=[1, 0, 2, 1, 0, 1], edge_g=[0, 2, 1, 0, 1, 1], theta_dim=p)


@pytest.mark.parametrize("topology", ["nonuniform_chain", "branching_tree"])
@pytest.mark.parametrize("p", [1, 3, 8, 11])
def test_theta_on_trees(monkeypatch, topology, p):
    dims = _dims(topology, p)
    batch = 5
    model, w, r1, r2, r3, rhs, theta_model = rk.newton_kkt_problem(dims, seed=13 + p, batch=batch, r2_max=1e2)
    theta_model[3] = rk.initialize_theta_model(dims, -50.0)  # an indefinite Schur complement: status 7
    d = _dev(model, theta_model, w, r1, r2, r3, rhs)
    got = {}
    for multi in ("1", "0"):
        monkeypatch.setenv("SIP_KKT_THETA_TREE_MULTI", multi)
        kkt = _make(dims, batch)
        assert kkt.kernel_name.startswith("tree:general")
        assert ("tree multi-rhs" in kkt.kernel_name) == (multi == "1")
        assert kkt.factor_theta(*d[:6]).cpu().tolist() == [0, 0, 0, 7, 0]
        sentinel = torch.full((batch, dims.full_dim), 3.0, dtype=torch.float64, device="cuda")
        got[multi] = kkt.solve_theta(d[0], d[1], d[6], sol=sentinel).cpu().numpy()
        assert (got[multi][3] == 3.0).all()
    o = KKTOracle(dims)
    for q in (0, 1, 2, 4):
        assert o.factor_theta(model[q], theta_model[q], w[q], r1[q], r2[q], r3[q]) == 0
        ref = o.solve_theta(model[q], theta_model[q], rhs[q])
        assert np.abs(got["1"][q] - ref).max() <= 1e-8 * np.abs(ref).max()
        assert np.abs(got["1"][q] - got["0"][q]).max() <= 1e-11 * np.abs(got["0"][q]).max()


def test_kernel_name_without_theta_is_unchanged():
    from sip_optimal_control_amd import BatchedNewtonKKT
    dims = _dims("branching_tree", 0)
    kkt = BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                           batch=2, root=dims.root)
    assert "tree multi-rhs" not in kkt.kernel_name

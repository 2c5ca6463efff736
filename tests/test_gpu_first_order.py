"""sip_kkt_gather_first_order (f, grad f, c, g from the first-order model outputs, on the device) against a numpy
restatement of the reference's loops (sip_optimal_control.cpp:47-125), bit for bit.

Equality is derived, not measured: every output entry is a fixed-order chain of fp64 adds (or one subtraction, or a
copy) with nothing to contract, so np.array_equal is the assertion.  The inputs span twelve decades per entry
(randn * 10**uniform(-6, 6)): another order of addition changes bits.  Every run writes into sentinel-filled buffers
between 64-double guard bands: the outputs are overwritten (no sentinel left, nothing accumulated into) and nothing
outside them is touched."""
import numpy as np
import pytest
import torch

from oracle.kkt import KKTDims
from tests import reference_kkt_problems as rk

pytestmark = pytest.mark.gpu
SENTINEL = -3.0e33
GUARD = 64
INVALID_ARGUMENT = -1
(X_STATE, X_CONTROL, Y_DYN, Y_NODE_C, Y_EDGE_C, Z_NODE, Z_EDGE) = range(7)
(N_F, N_DX, N_DTH, N_C, N_G, E_F, E_DX, E_DU, E_DTH, E_DYN, E_C, E_G) = range(12)


def _nonuniform_chain(p=0):  # the dims of tests/test_gpu_kkt_tree_fused.py: odd dims, zero constraint dims
    sd, cd = [4, 6, 5, 3, 6, 4, 5], [2, 3, 1, 2, 3, 2]
    return KKTDims(list(range(6)), list(range(1, 7)), sd, cd, node_c=[1, 0, 2, 0, 1, 0, 2],
                   node_g=[0, 2, 0, 1, 0, 0, 3], edge_c=[1, 2, 0, 1, 1, 0], edge_g=[2, 0, 1, 1, 0, 2], theta_dim=p)


def _branching_tree(zero_state=True):
    """Five nodes, root 2; node 2 is the parent of edges 0 and 2 and node 0 of edges 1 and 3 (not adjacent); edge 1
    has no control, node 3 (a leaf) no state."""
    return KKTDims(parents=[2, 0, 2, 0], children=[0, 3, 1, 4], state_dims=[3, 5, 4, 0 if zero_state else 1, 2],
                   control_dims=[2, 0, 3, 1], node_c=[1, 0, 2, 1, 0], node_g=[0, 2, 1, 0, 3], edge_c=[1, 0, 2, 1],
                   edge_g=[2, 1, 0, 1], root=2)


def _with_theta(dims, p):
    return KKTDims(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                   root=dims.root, theta_dim=p)


def _plan(dims, batch):
    from sip_optimal_control_amd import BatchedNewtonKKT
    return BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                            batch=batch, root=dims.root, theta_dim=dims.p)


def _inputs(kkt, dims, seed):
    rng = np.random.default_rng(seed)
    shape = (kkt.batch, kkt.first_order_len)
    first = rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 6, shape)
    x = rng.standard_normal((kkt.batch, kkt.x_dim + dims.p))
    init = rng.standard_normal((kkt.batch, dims.sd[dims.root]))
    return first, x, init


def _reference(kkt, dims, first, x, init):
    """sip_optimal_control.cpp:47-125 for every problem: explicit loops of scalar +=, in the reference's order, over
    the plan's own offset tables."""
    N, E, p = dims.N, dims.E, dims.p
    vo = [[kkt.vector_offset(t, k) for k in range(E if t in (X_CONTROL, Y_EDGE_C, Z_EDGE) else N)] for t in range(7)]
    fo = [[kkt.first_order_offset(b, k) for k in range(N if b <= N_G else E)] for b in range(12)]
    batch, xs = first.shape[0], kkt.x_dim
    f = np.zeros(batch)
    grad, c, g = np.zeros((batch, xs + p)), np.zeros((batch, kkt.y_dim)), np.zeros((batch, kkt.z_dim))
    for q in range(batch):
        m, acc = first[q], np.float64(0.0)
        for node in range(N):                                                   # :47-53
            acc += m[fo[N_F][node]]
        for edge in range(E):
            acc += m[fo[E_F][edge]]
        f[q] = acc
        gq, cq, zq = grad[q], c[q], g[q]                                        # (zero-filled, :57)
        for node in range(N):                                                   # :58-69
            for row in range(dims.sd[node]):
                gq[vo[X_STATE][node] + row] += m[fo[N_DX][node] + row]
            for row in range(p):
                gq[xs + row] += m[fo[N_DTH][node] + row]
        for edge in range(E):                                                   # :70-87
            parent = dims.parents[edge]
            for row in range(dims.sd[parent]):
                gq[vo[X_STATE][parent] + row] += m[fo[E_DX][edge] + row]
            for row in range(dims.cd[edge]):
                gq[vo[X_CONTROL][edge] + row] += m[fo[E_DU][edge] + row]
            for row in range(p):
                gq[xs + row] += m[fo[E_DTH][edge] + row]
        root = dims.root                                                        # :91-97
        for row in range(dims.sd[root]):
            cq[vo[Y_DYN][root] + row] = init[q, row] - x[q, vo[X_STATE][root] + row]
        for node in range(N):                                                   # :98-102
            for row in range(dims.ncd[node]):
                cq[vo[Y_NODE_C][node] + row] = m[fo[N_C][node] + row]
        for edge in range(E):                                                   # :103-111
            child = dims.children[edge]
            for row in range(dims.sd[child]):
                cq[vo[Y_DYN][child] + row] = m[fo[E_DYN][edge] + row]
            for row in range(dims.ecd[edge]):
                cq[vo[Y_EDGE_C][edge] + row] = m[fo[E_C][edge] + row]
        for node in range(N):                                                   # :115-119
            for row in range(dims.ngd[node]):
                zq[vo[Z_NODE][node] + row] = m[fo[N_G][node] + row]
        for edge in range(E):                                                   # :120-124
            for row in range(dims.egd[edge]):
                zq[vo[Z_EDGE][edge] + row] = m[fo[E_G][edge] + row]
    return f, grad, c, g


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


class _Guarded:
    """[guard | batch x length | guard], all sentinel."""

    def __init__(self, batch, length):
        self.buf = torch.full((2 * GUARD + batch * length,), SENTINEL, dtype=torch.float64, device="cuda")
        self.n = batch * length
        self.view = self.buf[GUARD:GUARD + self.n].view((batch, length) if length != 1 else (batch,))

    def check(self, written=True):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + self.n:] == SENTINEL).all(), "guard band touched"
        inside = host[GUARD:GUARD + self.n]
        assert (inside != SENTINEL).all() if written else (inside == SENTINEL).all()
        return inside.reshape(self.view.shape)


def _outputs(kkt, dims):
    return (_Guarded(kkt.batch, 1), _Guarded(kkt.batch, kkt.x_dim + dims.p), _Guarded(kkt.batch, kkt.y_dim),
            _Guarded(kkt.batch, kkt.z_dim))


def _check_case(dims, batch, seed, name_starts=None):
    kkt = _plan(dims, batch)
    assert kkt.input_status == 0
    if name_starts is not None:
        assert kkt.kernel_name.startswith(name_starts), kkt.kernel_name
    first, x, init = _inputs(kkt, dims, seed)
    ref = _reference(kkt, dims, first, x, init)
    outs = _outputs(kkt, dims)
    got = kkt.gather_first_order(_dev(first), _dev(x), _dev(init), *[o.view for o in outs])
    torch.cuda.synchronize()
    assert all(a is o.view for a, o in zip(got, outs))
    for what, o, r in zip(("f", "grad_f", "c", "g"), outs, ref):
        assert np.array_equal(o.check(), r), what
    # allocated by the call: the same, and of the stated shapes
    f, grad, c, g = kkt.gather_first_order(_dev(first), _dev(x), _dev(init))
    assert f.shape == (batch,) and grad.shape == (batch, kkt.x_dim + dims.p)
    assert c.shape == (batch, kkt.y_dim) and g.shape == (batch, kkt.z_dim)
    for what, a, r in zip(("f", "grad_f", "c", "g"), (f, grad, c, g), ref):
        assert np.array_equal(a.cpu().numpy(), r), what
    return kkt


@pytest.mark.parametrize("n,m,T,batch", [(6, 2, 5, 1), (6, 2, 5, 5), (12, 4, 3, 67)])
def test_uniform_chain_of_the_benchmark_family(n, m, T, batch):
    """(12, 4): the f1 dims (c 6, g 8).  These plans run the chain kernels, and so the arithmetic-offset form."""
    kkt = _check_case(rk.newton_kkt_dims(n, m, T), batch, seed=300 + batch, name_starts="chain:")
    assert "chain condensation" in kkt.kernel_name


def test_uniform_chain_with_theta():
    """Offsets and length are read after set_theta (the constructor makes that call): df_dtheta has p rows."""
    dims = _with_theta(rk.newton_kkt_dims(4, 1, 4), 3)
    kkt = _check_case(dims, 9, seed=311, name_starts="chain:")
    assert kkt.first_order_offset(N_C, 0) - kkt.first_order_offset(N_DTH, 0) == 3
    assert kkt.first_order_offset(E_DYN, 0) - kkt.first_order_offset(E_DTH, 0) == 3
    assert kkt.first_order_len == _plan(rk.newton_kkt_dims(4, 1, 4), 9).first_order_len + 3 * (dims.N + dims.E)


@pytest.mark.parametrize("p", [0, 2])
def test_nonuniform_chain(p):
    _check_case(_nonuniform_chain(p), 7, seed=320 + p, name_starts="tree:")


def test_branching_tree_whose_root_is_not_node_zero():
    dims = _branching_tree()
    if _plan(dims, 1).input_status != 0:   # a node without state is not a valid plan: that one zero goes, the rest stays
        dims = _branching_tree(zero_state=False)
    print("state dims:", dims.sd)
    kkt = _check_case(dims, 515, seed=330, name_starts="tree:")   # 515: whole workgroups plus a partial one
    assert kkt.first_order_offset(E_DU, 2) == kkt.first_order_offset(E_DX, 2) + dims.sd[2]
    assert kkt.first_order_offset(E_DTH, 1) == kkt.first_order_offset(E_DU, 1)       # edge 1: no control, no theta
    with pytest.raises(IndexError):
        kkt.first_order_offset(E_F, dims.E)
    with pytest.raises(IndexError):
        kkt.first_order_offset(12, 0)
    kkt.first_order_offset(N_F, dims.E)    # the last node


@pytest.mark.parametrize("dims", [rk.newton_kkt_dims(6, 2, 5), _nonuniform_chain(2)], ids=["uniform", "tables"])
def test_outputs_are_overwritten_not_accumulated_into(dims):
    """Two calls into the same buffers, the second with other inputs: what is left is the second call's result alone."""
    kkt = _plan(dims, 5)
    outs = _outputs(kkt, dims)
    for seed in (340, 341):
        first, x, init = _inputs(kkt, dims, seed)
        kkt.gather_first_order(_dev(first), _dev(x), _dev(init), *[o.view for o in outs])
    torch.cuda.synchronize()
    for o, r in zip(outs, _reference(kkt, dims, first, x, init)):
        assert np.array_equal(o.check(), r)


def _raw(kkt, first, x, init, f, grad, c, g):
    ptr = lambda t: None if t is None else t.data_ptr()
    return kkt._lib.sip_kkt_gather_first_order(kkt._plan, ptr(first), ptr(x), ptr(init), ptr(f), ptr(grad), ptr(c),
                                               ptr(g), kkt._stream())


@pytest.mark.parametrize("dims", [rk.newton_kkt_dims(6, 2, 5), _with_theta(_branching_tree(zero_state=False), 2)],
                         ids=["uniform", "tables"])
def test_only_f_when_x_is_not_new(dims):
    kkt = _plan(dims, 5)
    first, x, init = _inputs(kkt, dims, seed=350)
    ref = _reference(kkt, dims, first, x, init)
    f = _Guarded(kkt.batch, 1)
    got = kkt.gather_first_order(_dev(first), None, None, f.view, new_x=False)
    torch.cuda.synchronize()
    assert got[0] is f.view and got[1:] == (None, None, None)
    assert np.array_equal(f.check(), ref[0])
    # the C level: grad_f, c, g all NULL is that case; any other mix is an error and writes nothing
    d_first, d_x, d_init = _dev(first), _dev(x), _dev(init)
    outs = _outputs(kkt, dims)
    fv, gv, cv, zv = [o.view for o in outs]
    assert _raw(kkt, d_first, None, None, fv, None, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].check(), ref[0])
    outs = _outputs(kkt, dims)
    fv, gv, cv, zv = [o.view for o in outs]
    for mix in ((gv, None, zv), (None, cv, zv), (gv, cv, None), (gv, None, None), (None, None, zv)):
        assert _raw(kkt, d_first, d_x, d_init, fv, *mix) == INVALID_ARGUMENT
    assert _raw(kkt, d_first, d_x, d_init, None, gv, cv, zv) == INVALID_ARGUMENT
    assert _raw(kkt, None, d_x, d_init, fv, gv, cv, zv) == INVALID_ARGUMENT
    assert _raw(kkt, d_first, None, d_init, fv, gv, cv, zv) == INVALID_ARGUMENT
    assert _raw(kkt, d_first, d_x, None, fv, gv, cv, zv) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    for o in outs:
        o.check(written=False)


def test_an_empty_space_needs_no_buffer():
    """z_dim == 0: g may be NULL next to real grad_f and c."""
    dims = KKTDims([0, 1], [1, 2], [3, 3, 3], [2, 2], node_c=[0, 1, 2], edge_c=[1, 0])
    kkt = _plan(dims, 3)
    assert kkt.z_dim == 0 and kkt.input_status == 0
    first, x, init = _inputs(kkt, dims, seed=360)
    ref = _reference(kkt, dims, first, x, init)
    outs = _outputs(kkt, dims)
    assert _raw(kkt, _dev(first), _dev(x), _dev(init), outs[0].view, outs[1].view, outs[2].view, None) == 0
    torch.cuda.synchronize()
    for o, r in zip(outs[:3], ref[:3]):
        assert np.array_equal(o.check(), r)


@pytest.mark.parametrize("dims", [rk.newton_kkt_dims(6, 2, 5), _with_theta(_nonuniform_chain(), 2)],
                         ids=["uniform", "tables"])
def test_first_call_of_a_plan_can_be_the_captured_one(dims):
    """The offset tables are uploaded by sip_kkt_plan_create / sip_kkt_plan_set_theta, the call only enqueues kernels:
    the very first gather of a plan may run under stream capture.  (The code object is loaded beforehand through
    another plan.)"""
    batch = 6
    warm = _plan(dims, batch)
    first, x, init = _inputs(warm, dims, seed=370)
    d_first, d_x, d_init = _dev(first), _dev(x), _dev(init)
    warm.gather_first_order(d_first, d_x, d_init)
    torch.cuda.synchronize()
    kkt = _plan(dims, batch)                            # a fresh plan: nothing of it has run yet
    outs = _outputs(kkt, dims)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        kkt.gather_first_order(d_first, d_x, d_init, *[o.view for o in outs])
    torch.cuda.synchronize()
    for o in outs:
        o.check(written=False)                          # captured, not executed
    graph.replay()
    torch.cuda.synchronize()
    for o, r in zip(outs, _reference(kkt, dims, first, x, init)):
        assert np.array_equal(o.check(), r)


def test_a_plan_with_a_latched_invalid_input_launches_nothing():
    from sip_optimal_control_amd import BatchedNewtonKKT
    kkt = BatchedNewtonKKT([0, 1], [1, 2], [3, -1, 3], [2, 2], batch=4)
    assert kkt.input_status != 0 and kkt.first_order_len == 0
    with pytest.raises(IndexError):
        kkt.first_order_offset(N_F, 0)
    outs = [_Guarded(4, k) for k in (1, 13, 9, 1)]
    d_in = torch.zeros(4, 32, dtype=torch.float64, device="cuda")
    assert _raw(kkt, d_in, d_in, d_in, *[o.view for o in outs]) == INVALID_ARGUMENT
    assert _raw(kkt, d_in, None, None, outs[0].view, None, None, None) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    for o in outs:
        o.check(written=False)


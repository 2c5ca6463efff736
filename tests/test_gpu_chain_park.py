"""The parked fused sweep of the (12, 4) chain kernels (chain_qw16.hpp, PARK): the spill slots of nodes 1 .. KEEP
stay in accumulation registers between the backward sweep and the rollout instead of travelling through the workspace.

The arithmetic is the plain kernel's, so sol, gains and status must be BITWISE what the plain kernel of the shape
(SIP_LQR_PARK=0 at plan creation; 1 parks at any batch, the default only from four wavefronts per CU on, batch 4096 on an MI355X) gives, for horizons on both sides of KEEP (16 in the full layout, 15 in the
symmetric-packed one: T covers KEEP - 1 .. KEEP + 2 of both), for a full wavefront (batch 4) and for a second one with
one valid problem and three clamped rows (batch 5); both are within the chain tests' tolerance of the oracle (1e-9,
tests/test_gpu_chain_parity.py).  Two calls with different inputs on one plan and workspace show that nothing of the
first call survives in the registers' image; the second call of batch 5 carries an indefinite R and a non-positive
delta.  sip_lqr_factor + sip_lqr_solve on the same workspace afterwards run on the plain kernel and still match."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TOL = 1e-9
N, M = 12, 4
KEEP = {False: 16, True: 15}  # chain_qw16.hpp (tests/test_park_regs.py holds the listing to it)
HORIZONS = sorted({1, 2} | {k + d for k in KEEP.values() for d in (-1, 0, 1, 2)})


def _rel(a, b):
    scale = np.abs(b).max(axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    return float((np.abs(a - b) / scale).max())


def _bits(t):
    return t.contiguous().view(torch.int64)


def _inputs(shape, batch, seed, symmetric, failures):
    """(full mats for the oracle, mats in the plan's layout, vecs)"""
    from sip_optimal_control_amd import synthetic
    mats, vecs = synthetic.make_chain_batch(shape, batch, seed=seed, device="cuda:0", cross_term=0.01)
    if failures:  # inside the parked range: an indefinite R on edge 1 and a non-positive delta at node 1
        off = shape.mats_off(1)
        mats[2, off["R"]:off["R"] + M * M] = -1e4 * torch.eye(M, dtype=torch.float64, device="cuda:0").reshape(-1)
        mats[batch - 1, off["delta"] + 1] = 0.0
    own = mats[:, torch.from_numpy(shape.packed().pack_index()).to("cuda:0")].contiguous() if symmetric else mats
    return mats, own, vecs


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("batch", [4, 5])
@pytest.mark.parametrize("symmetric", [False, True], ids=["full", "sym"])
def test_parked_sweep_gives_the_plain_kernels_bits(oracle_lib, monkeypatch, symmetric, batch, T):
    from sip_optimal_control_amd import BatchedChainLQR, ChainShape
    shape = ChainShape(N, M, T)
    monkeypatch.setenv("SIP_LQR_PARK", "1")  # read when a plan is created; 1: parked at any batch
    parked = BatchedChainLQR(N, M, T, batch, symmetric=symmetric)
    monkeypatch.setenv("SIP_LQR_PARK", "0")
    plain = BatchedChainLQR(N, M, T, batch, symmetric=symmetric)
    monkeypatch.delenv("SIP_LQR_PARK")
    assert parked.kernel_name == plain.kernel_name + ",park", (parked.kernel_name, plain.kernel_name)
    assert ("sym" in plain.kernel_name) == symmetric and "qw16<12,4,staged" in plain.kernel_name

    # two consecutive calls on the same plans (and so the same workspaces); the second one fails two problems
    for call, seed in enumerate((4100 + T, 4200 + T)):
        failures = call == 1 and batch == 5 and T >= 2
        full, own, vecs = _inputs(shape, batch, seed, symmetric, failures)
        s1, g1, st1 = (t.clone() for t in parked.factor_solve(own, vecs))
        s0, g0, st0 = (t.clone() for t in plain.factor_solve(own, vecs))
        torch.cuda.synchronize()
        ref_sol, ref_gains, ref_status = oracle_lib.chain_batch(N, M, T, full.cpu().numpy(), vecs.cpu().numpy())
        assert torch.equal(st1, st0)
        np.testing.assert_array_equal(st1.cpu().numpy(), ref_status)
        assert (ref_status != 0).sum() == (2 if failures else 0)
        assert torch.equal(_bits(s1), _bits(s0)) and torch.equal(_bits(g1), _bits(g0))  # every problem, failed ones too
        ok = ref_status == 0
        for sol, gains in ((s1, g1), (s0, g0)):
            assert _rel(sol.cpu().numpy()[ok], ref_sol[ok]) <= TOL
            assert _rel(gains.cpu().numpy()[ok], ref_gains[ok]) <= TOL

    # the parked call left no complete factor state; factor + solve write their own on the same workspace
    full, own, vecs = _inputs(shape, batch, 4300 + T, symmetric, False)
    parked.factor_solve(own, vecs)
    gains, status = parked.factor(own)
    sol = parked.solve(own, vecs, gains)
    torch.cuda.synchronize()
    ref_sol, ref_gains, ref_status = oracle_lib.chain_batch(N, M, T, full.cpu().numpy(), vecs.cpu().numpy())
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    assert (ref_status == 0).all()
    assert _rel(sol.cpu().numpy(), ref_sol) <= TOL
    assert _rel(gains.cpu().numpy(), ref_gains) <= TOL  # K from the factor sweep, k from the solve sweep


@pytest.mark.parametrize("symmetric", [False, True], ids=["full", "sym"])
def test_parked_sweep_at_the_headline_size(monkeypatch, symmetric):
    """Batch 4096, T = 50 (C3): four wavefronts per CU, where a stage's LDS-DMA takes long enough that a counted wait
    which leaves part of it in flight shows (a first version waited vmcnt(M) behind a parked node while the compiler
    had paired the M gain stores into M / 2 instructions: right at batch 5, wrong here).  Bitwise against the plain
    kernel, twice on the same plans with different right-hand sides."""
    from sip_optimal_control_amd import BatchedChainLQR, ChainShape
    T, batch = 50, 4096
    shape = ChainShape(N, M, T)
    monkeypatch.setenv("SIP_LQR_PARK", "1")  # (the default at this batch on an MI355X)
    parked = BatchedChainLQR(N, M, T, batch, symmetric=symmetric)
    monkeypatch.setenv("SIP_LQR_PARK", "0")
    plain = BatchedChainLQR(N, M, T, batch, symmetric=symmetric)
    monkeypatch.delenv("SIP_LQR_PARK")
    assert parked.kernel_name == plain.kernel_name + ",park"
    for seed in (31, 32):
        _, own, vecs = _inputs(shape, batch, seed, symmetric, False)
        s1, g1, st1 = (t.clone() for t in parked.factor_solve(own, vecs))
        s0, g0, st0 = plain.factor_solve(own, vecs)
        torch.cuda.synchronize()
        assert bool((st0 == 0).all()) and torch.equal(st1, st0)
        assert torch.equal(_bits(s1), _bits(s0)) and torch.equal(_bits(g1), _bits(g0))


def test_embedded_shapes_stay_on_the_plain_kernel(monkeypatch):
    """A shape embedded in the (12, 4) kernel does not park; the plan of the shape itself does -- by default from
    16 problems per CU on, where the launch is bound by its bytes -- and keeps its split form."""
    from sip_optimal_control_amd import BatchedChainLQR
    monkeypatch.setenv("SIP_LQR_PARK", "1")
    monkeypatch.setenv("SIP_LQR_EXTRA", "0")  # hides the exact (11, 4) kernel
    name = BatchedChainLQR(11, 4, 6, 3).kernel_name
    assert "<12,4,staged>" in name and "embedding (11,4)" in name and ",park" not in name
    monkeypatch.delenv("SIP_LQR_EXTRA")
    s = BatchedChainLQR(N, M, 6, 3)
    assert s.kernel_name.endswith(",park") and s.has_split
    monkeypatch.delenv("SIP_LQR_PARK")
    # four wavefronts of four problems per CU: batch 4096 on the 256 CUs of an MI355X
    least = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    assert ",park" not in BatchedChainLQR(N, M, 2, least - 1).kernel_name
    assert BatchedChainLQR(N, M, 2, least).kernel_name.endswith(",park")
    assert BatchedChainLQR(N, M, 2, least, symmetric=True).kernel_name.endswith("sym>/f64,park")

#!/usr/bin/env python3
"""The backward pass of the chain solve (sip_lqr_vjp) and its gradient kernel (sip_lqr_vjp_mats) against the forward
pass they accompany: for the default fp64 plan and the `fused_f32` + `separate_sweeps` fp32 plan at C3's shape
(12, 4, T = 50) and the `separate_sweeps` fp32 plan at C4's shape (32, 8, T = 100), at batch 4096 and 1024, the time of
    vjp_mats            the kernel alone: sol and adj read, grad_mats written, in the plan's dtype
    vjp                 sip_lqr_vjp: the adjoint solve, the status mask and the kernel
    vjp_vecs_only       sip_lqr_vjp with d_grad_mats = NULL
    forward             sip_lqr_factor + sip_lqr_solve of the same plan
    shape <w>,<r>       the kernel alone with <w> wavefronts per workgroup and <r> stages per workgroup (0: the
                        default run; more than fits: the longest that fits), through SIP_LQR_VJP_SHAPE: the
                        candidates of the launch shape, DESIGN 4.11
Next to the kernel the bytes it has to move (sol and adj once, grad_mats written) and what those bytes take at
6.3 TB/s, the streaming rate measured on an MI355X.

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the calls alternate.  `range_ms` is max - min over the blocks.  One JSON record per plan and batch, printed and
written to --out as a JSON list.

    python tools/bench_vjp.py [--batches 4096,1024] [--blocks 9] [--launches 8] [--shapes "8,0;4,0;8,1000;8,13"]
                              [--out profiles/vjp_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from sip_optimal_control_amd import BatchedChainLQR, ChainShape, synthetic
from sip_optimal_control_amd._lib import load_library

STREAM_TBPS = 6.3
PLANS = [("C3 fp64", 12, 4, 50, torch.float64, {}),
         ("C3 fp32 fused_f32 + separate_sweeps", 12, 4, 50, torch.float32, {"fused_f32": True, "separate_sweeps": True}),
         ("C4 fp32 separate_sweeps", 32, 8, 100, torch.float32, {"separate_sweeps": True})]


def block_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def alternating(fns, blocks, launches):
    """fns: {name: callable}; (median, max - min) of `blocks` blocks each, the blocks taken in turn."""
    for fn in fns.values():  # warm-up: code objects, the allocator, the clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(block_ms(fn, launches))
    return {name: (statistics.median(t), max(t) - min(t)) for name, t in times.items()}


def with_shape(shape, fn):
    """fn under SIP_LQR_VJP_SHAPE=shape (the library reads it per call)."""
    def call():
        os.environ["SIP_LQR_VJP_SHAPE"] = shape
        try:
            fn()
        finally:
            del os.environ["SIP_LQR_VJP_SHAPE"]
    return call


def one(args, label, n, m, T, dtype, kwargs, batch):
    shape = ChainShape(n, m, T)
    mats64, vecs64 = synthetic.make_chain_batch(shape, batch, seed=1, device="cuda:0", dtype=torch.float64,
                                                cross_term=0.01)
    mats, vecs = mats64.to(dtype), vecs64.to(dtype)
    del mats64, vecs64
    s = BatchedChainLQR(n, m, T, batch, dtype=dtype, **kwargs)
    gains, status = s.factor(mats)
    sol = s.solve(mats, vecs, gains)
    g = torch.randn(batch, shape.vecs_len, dtype=torch.float64, device="cuda:0",
                    generator=torch.Generator(device="cuda:0").manual_seed(2)).to(dtype)
    grad_mats, lam = s.vjp(mats, sol, g, gains)
    torch.cuda.synchronize()
    assert (status == 0).all().item() and torch.isfinite(grad_mats).all().item()
    kernel = lambda: s.vjp_mats(sol, lam, grad_mats=grad_mats)

    def forward():
        s.factor(mats, gains)
        s.solve(mats, vecs, gains, sol)

    calls = {"vjp_mats": kernel,
             "vjp": lambda: s.vjp(mats, sol, g, gains),
             "vjp_vecs_only": lambda: s.vjp(mats, sol, g, gains, want_mats=False),
             "forward": forward}
    for cand in args.shapes.split(";"):
        calls["shape " + cand] = with_shape(cand, kernel)
    reference = grad_mats.clone()
    for cand in args.shapes.split(";"):  # every candidate computes the same bits
        grad_mats.fill_(float("nan"))
        calls["shape " + cand]()
        assert torch.equal(grad_mats, reference), cand
    got = alternating(calls, args.blocks, args.launches)
    esize = mats.element_size()
    moved = batch * (shape.mats_len + 2 * shape.vecs_len) * esize
    ms = {k: round(v[0], 4) for k, v in got.items()}
    return {"plan": label, "shape": [n, m, T, batch], "kernel": s.kernel_name, "blocks": args.blocks,
            "launches": args.launches, "library": load_library().sip_lqr_version().decode(), "ms": ms,
            "range_ms": {k: round(v[1], 4) for k, v in got.items()},
            "vjp_mats_bytes": moved,
            "vjp_mats_ms_at_%.1f_TBps" % STREAM_TBPS: round(moved / (STREAM_TBPS * 1e12) * 1e3, 4),
            "vjp_mats_TBps": round(moved / (ms["vjp_mats"] * 1e-3) / 1e12, 3),
            "vjp_over_forward": round(ms["vjp"] / ms["forward"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--shapes", default="8,0;4,0;6,0;8,1000;4,1000;8,13")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vjp_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vjp.py needs a GPU"
    records = []
    for label, n, m, T, dtype, kwargs in PLANS:
        for batch in (int(b) for b in args.batches.split(",")):
            records.append(one(args, label, n, m, T, dtype, kwargs, batch))
            print(json.dumps(records[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

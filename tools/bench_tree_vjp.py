#!/usr/bin/env python3
"""The backward pass of the tree solve (sip_lqr_tree_vjp) and its gradient kernel (sip_lqr_tree_vjp_input) against the
forward pass they accompany, on the reference's three variable-shape benchmark trees (BM_LQRVariableFactorSolve,
benchmarks/lqr_benchmark.cpp:209-310) at T = 63, batch 4096 and 1024: the time of
    vjp_input           the kernel alone: output and adj read, grad_input written
    vjp                 sip_lqr_tree_vjp: the one-column adjoint solve, the status mask and the kernel
    vjp_lambda_only     sip_lqr_tree_vjp with d_grad_input = NULL
    forward             sip_lqr_tree_factor_fused + sip_lqr_tree_solve_fused of the same plan
    shape <w>,<r>       the kernel alone with <w> wavefronts per workgroup and <r> entries of the input arena per
                        workgroup (0: one run per problem), through SIP_LQR_TREE_VJP_SHAPE: the candidates of the launch
                        shape, DESIGN 4.11.1
Next to the kernel its traffic floor: one input-arena-sized write plus two output-arena-sized reads, and what those
bytes take at 6.3 TB/s, the streaming rate measured on an MI355X.  (The table, 8 bytes per input-arena scalar, is the
same for every problem and stays in cache: it is not part of the floor.)

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the calls alternate.  `range_ms` is max - min over the blocks.  One JSON record per tree and batch, printed and
written to --out as a JSON list.

    python tools/bench_tree_vjp.py [--batches 4096,1024] [--blocks 9] [--launches 8] [--shapes "8,0;4,0;8,4096"]
                                   [--out profiles/tree_vjp_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from sip_optimal_control_amd._lib import load_library
from sip_optimal_control_amd.tree import BatchedTreeLQR

STREAM_TBPS = 6.3
TREES = ("heterogeneous_chain", "shallow_wide_tree", "binary_tree")


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
    """fn under SIP_LQR_TREE_VJP_SHAPE=shape (the library reads it per call)."""
    def call():
        os.environ["SIP_LQR_TREE_VJP_SHAPE"] = shape
        try:
            fn()
        finally:
            del os.environ["SIP_LQR_TREE_VJP_SHAPE"]
    return call


def one(args, shape, batch):
    import full_batch_problems as fb
    topo = fb.variable_benchmark_topology(shape, T=args.T)
    blocks = fb.make_blocks(topo, batch, np.random.default_rng(17 + 31 * shape), "variable_benchmark")  # distinct problems
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    maps = fb.PlanMaps(s, topo)
    s.input.copy_(torch.from_numpy(maps.pack_input(s, *fb.to_oracle(topo, blocks))))
    del blocks
    status = s.factor_fused()
    s.solve_fused()
    solved = s.output.clone()
    g = torch.randn(batch, s.out_len, dtype=torch.float64, device=s.device,
                    generator=torch.Generator(device=s.device).manual_seed(2))
    grad_input, lam = s.vjp(g, output=solved)
    torch.cuda.synchronize()
    assert (status == 0).all().item() and torch.isfinite(grad_input).all().item()
    kernel = lambda: s.vjp_input(solved, lam, grad_input=grad_input)

    def forward():
        s.factor_fused()
        s.solve_fused()

    calls = {"vjp_input": kernel,
             "vjp": lambda: s.vjp(g, output=solved),
             "vjp_lambda_only": lambda: s.vjp(g, output=solved, want_input=False),
             "forward": forward}
    for cand in args.shapes.split(";"):
        calls["shape " + cand] = with_shape(cand, kernel)
    reference = grad_input.clone()
    for cand in args.shapes.split(";"):  # every candidate computes the same bits
        grad_input.fill_(float("nan"))
        calls["shape " + cand]()
        assert torch.equal(grad_input, reference), cand
    got = alternating(calls, args.blocks, args.launches)
    floor_bytes = batch * 8 * (s.in_len + 2 * s.out_len)
    ms = {k: round(v[0], 4) for k, v in got.items()}
    return {"tree": TREES[shape], "T": args.T, "batch": batch, "input_len": s.in_len, "output_len": s.out_len,
            "kernel": s.split_kernel_name, "multi_kernel": s.multi_kernel_name, "vjp_kernel": s.vjp_kernel_name,
            "blocks": args.blocks, "launches": args.launches, "library": load_library().sip_lqr_version().decode(),
            "ms": ms, "range_ms": {k: round(v[1], 4) for k, v in got.items()},
            "vjp_input_floor_bytes": floor_bytes,
            "vjp_input_floor_ms_at_%.1f_TBps" % STREAM_TBPS: round(floor_bytes / (STREAM_TBPS * 1e12) * 1e3, 4),
            "vjp_input_TBps": round(floor_bytes / (ms["vjp_input"] * 1e-3) / 1e12, 3),
            "vjp_input_over_floor": round(ms["vjp_input"] / (floor_bytes / (STREAM_TBPS * 1e12) * 1e3), 3),
            "vjp_over_forward": round(ms["vjp"] / ms["forward"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--T", type=int, default=63)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--shapes", default="8,0;4,0;2,0;8,4096;4,4096;4,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_vjp_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tree_vjp.py needs a GPU"
    records = []
    for shape in range(len(TREES)):
        for batch in (int(b) for b in args.batches.split(",")):
            records.append(one(args, shape, batch))
            print(json.dumps(records[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The tree KKT residual (sip_lqr_tree_residual) and the refinement built on it (sip_lqr_tree_refine) against the solves
they accompany, on the reference's three variable-shape benchmark trees (BM_LQRVariableFactorSolve,
benchmarks/lqr_benchmark.cpp:209-310) at T = 63, batch 4096 and 1024: the time of
    residual            norms only
    residual_vector     with the residual vector written as well
    solve_fused         sip_lqr_tree_solve_fused against the factor state (a kernel this change does not touch)
    solve_multi_1       sip_lqr_tree_solve_multi with one column: the correction solve of a refinement round
    refine_1, _2, _3    sip_lqr_tree_refine from zero with 1, 2 and 3 rounds (each round: scaled residual, one-column
                        solve, update; then one more residual)
Next to each residual the bytes it has to move (the input arena and the two vector arrays once; + the vector written),
what those bytes take at 6.3 TB/s, the streaming rate measured on an MI355X, and the rate achieved.

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the calls alternate.  `range_ms` is max - min over the blocks.  One JSON record per tree and batch, printed and
written to --out as a JSON list.

    python tools/bench_tree_refine.py [--batches 4096,1024] [--blocks 9] [--launches 8] [--out profiles/tree_refine_bench.json]"""
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


def one(args, shape, batch):
    import full_batch_problems as fb
    topo = fb.variable_benchmark_topology(shape, T=args.T)
    blocks = fb.make_blocks(topo, batch, np.random.default_rng(17 + 31 * shape), "variable_benchmark")  # distinct problems
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    maps = fb.PlanMaps(s, topo)
    s.input.copy_(torch.from_numpy(maps.pack_input(s, *fb.to_oracle(topo, blocks))))
    rhs = torch.from_numpy(maps.pack_rhs(s, {k: blocks[k] for k in ("q", "c", "r")})).to(s.device)[None].contiguous()
    del blocks
    status = s.factor_fused()
    s.solve_fused()
    solved = s.output.clone()
    col_out = torch.zeros(1, batch, s.out_len, dtype=torch.float64, device=s.device)
    torch.cuda.synchronize()
    assert (status == 0).all().item()
    calls = {"residual": lambda: s.residual(solved, want_vector=False),
             "residual_vector": lambda: s.residual(solved),
             "solve_fused": s.solve_fused,
             "solve_multi_1": lambda: s.solve_multi(rhs, out_cols=col_out),
             "refine_1": lambda: s.refine(iterations=1),
             "refine_2": lambda: s.refine(iterations=2),
             "refine_3": lambda: s.refine(iterations=3)}
    got = alternating(calls, args.blocks, args.launches)
    moved = {"residual": batch * 8 * (s.in_len + 2 * s.out_len), "residual_vector": batch * 8 * (s.in_len + 3 * s.out_len)}
    ms = {k: round(v[0], 4) for k, v in got.items()}
    # what three rounds reach: the norms by round and the change of the solution against the plain solve
    ref, norms = s.refine(iterations=3)
    torch.cuda.synchronize()
    return {"tree": TREES[shape], "T": args.T, "batch": batch, "kernel": s.split_kernel_name,
            "multi_kernel": s.multi_kernel_name, "residual_kernel": s.residual_kernel_name, "blocks": args.blocks,
            "launches": args.launches, "library": load_library().sip_lqr_version().decode(), "ms": ms,
            "range_ms": {k: round(v[1], 4) for k, v in got.items()},
            "residual_bytes": moved,
            "residual_ms_at_%.1f_TBps" % STREAM_TBPS: {k: round(b / (STREAM_TBPS * 1e12) * 1e3, 4) for k, b in moved.items()},
            "residual_TBps": {k: round(b / (ms[k] * 1e-3) / 1e12, 3) for k, b in moved.items()},
            "residual_over_solve_fused": round(ms["residual"] / ms["solve_fused"], 4),
            "residual_over_solve_multi_1": round(ms["residual"] / ms["solve_multi_1"], 4),
            "refine_3_over_solve_fused": round(ms["refine_3"] / ms["solve_fused"], 4),
            "worst_norm_by_round": [float(v) for v in norms.max(dim=1).values.tolist()],
            "max_rel_change_of_the_solution": float(((ref - solved).abs().max() / solved.abs().max()).item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--T", type=int, default=63)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_refine_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tree_refine.py needs a GPU"
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

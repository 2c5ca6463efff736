#!/usr/bin/env python3
"""The multi-column tree KKT residual (sip_lqr_tree_residual_multi) and the refinement around sip_lqr_tree_solve_multi
(sip_lqr_tree_refine_multi) against the same work done column by column with sip_lqr_tree_residual /
sip_lqr_tree_refine, which the library still has: the reference's three variable-shape benchmark trees
(BM_LQRVariableFactorSolve, benchmarks/lqr_benchmark.cpp:209-310) at T = 63, distinct problems, batch 4096 and 1024,
8 columns.  Per tree and batch the time of
    residual_multi       norms only: one call
    residual_x8          8 calls of sip_lqr_tree_residual, the same arguments column by column
    refine_multi_1,2,3   sip_lqr_tree_refine_multi from zero with 1, 2 and 3 rounds
    refine_1,2,3_x8      8 calls of sip_lqr_tree_refine
    solve_multi          sip_lqr_tree_solve_multi on the 8 columns
Next to the residual the bytes the multi-column form has to move (the input arena once per group of columns a launch
carries, the right-hand side and the iterate of every column once) and what those take at 6.3 TB/s, the streaming rate
measured on an MI355X.

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the calls alternate.  `range_ms` is max - min over the blocks.  One JSON record per tree and batch, printed and
written to --out as a JSON list.  --residual-only leaves the refinement out (for a library built with another
SIP_TREE_RESIDUAL_COLS_PREFER_SPLIT, loaded through SIP_LQR_LIB).

    python tools/bench_tree_refine_multi.py [--batches 4096,1024] [--blocks 9] [--launches 8] [--trees shallow]
                                            [--residual-only] [--out profiles/tree_refine_multi_bench.json]"""
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
C = 8


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
    rhs = torch.from_numpy(maps.pack_rhs(s, {k: blocks[k] for k in ("q", "c", "r")})).to(s.device)
    del blocks
    # columns: the right-hand side scaled by powers of two, so that every column is a problem of the same kind
    f = torch.tensor([(-1.0) ** c * 2.0 ** (c - C // 2) for c in range(C)], dtype=torch.float64, device=s.device)
    rhs_cols = (f[:, None, None] * rhs[None]).contiguous()
    status = s.factor_fused()
    sol_cols = s.solve_multi(rhs_cols)
    torch.cuda.synchronize()
    assert (status == 0).all().item()
    group = s.residual_multi_columns

    def each(fn):
        def run():
            for c in range(C):
                fn(c)
        return run

    calls = {"residual_multi": lambda: s.residual_multi(sol_cols, rhs_cols, want_vector=False),
             "residual_x%d" % C: each(lambda c: s.residual(sol_cols[c], rhs=rhs_cols[c], want_vector=False)),
             "solve_multi": lambda: s.solve_multi(rhs_cols, out_cols=sol_cols)}
    if not args.residual_only:
        for it in (1, 2, 3):
            calls["refine_multi_%d" % it] = lambda it=it: s.refine_multi(rhs_cols, iterations=it)
            calls["refine_%d_x%d" % (it, C)] = each(lambda c, it=it: s.refine(iterations=it, rhs=rhs_cols[c]))
    got = alternating(calls, args.blocks, args.launches)
    ms = {k: round(v[0], 4) for k, v in got.items()}
    launches = -(-C // group)
    moved = batch * 8 * (launches * s.in_len + C * 2 * s.out_len)
    rec = {"tree": TREES[shape], "T": args.T, "batch": batch, "columns": C, "multi_kernel": s.multi_kernel_name,
           "residual_kernel": s.residual_kernel_name, "residual_multi_kernel": s.residual_multi_kernel_name,
           "residual_multi_columns_per_launch": group, "residual_multi_launches": launches, "blocks": args.blocks,
           "launches": args.launches, "library": load_library().sip_lqr_version().decode(), "ms": ms,
           "range_ms": {k: round(v[1], 4) for k, v in got.items()},
           "residual_multi_bytes": moved,
           "residual_multi_ms_at_%.1f_TBps" % STREAM_TBPS: round(moved / (STREAM_TBPS * 1e12) * 1e3, 4),
           "residual_multi_TBps": round(moved / (ms["residual_multi"] * 1e-3) / 1e12, 3),
           "residual_multi_over_singles": round(ms["residual_multi"] / ms["residual_x%d" % C], 4)}
    if not args.residual_only:
        for it in (1, 2, 3):
            rec["refine_multi_%d_over_singles" % it] = round(ms["refine_multi_%d" % it] / ms["refine_%d_x%d" % (it, C)], 4)
        # what three rounds reach, and that the two ways agree: norms by round, worst over problems and columns relative
        # to each column's right-hand side
        ref, norms = s.refine_multi(rhs_cols, iterations=3)
        single = torch.stack([s.refine(iterations=3, rhs=rhs_cols[c])[0].clone() for c in range(C)])
        torch.cuda.synchronize()
        scale = rhs_cols.abs().amax(dim=(1, 2))
        rec["worst_relative_norm_by_round"] = [float(v) for v in (norms / scale[None, :, None]).amax(dim=(1, 2)).tolist()]
        rec["max_rel_difference_to_column_by_column"] = float(
            ((ref - single).abs().amax(dim=(1, 2)) / single.abs().amax(dim=(1, 2))).max().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--T", type=int, default=63)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--trees", default="", help="only the trees whose name contains this")
    ap.add_argument("--residual-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_refine_multi_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tree_refine_multi.py needs a GPU"
    records = []
    for shape in range(len(TREES)):
        if args.trees not in TREES[shape]:
            continue
        for batch in (int(b) for b in args.batches.split(",")):
            records.append(one(args, shape, batch))
            print(json.dumps(records[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The multi-column KKT residual (sip_lqr_residual_multi) and the refinement around sip_lqr_solve_multi
(sip_lqr_refine_multi) against the same work done column by column with sip_lqr_residual / sip_lqr_refine, which the
library still has: for the three plans of tools/bench_refine.py (default fp64 and `fused_f32` + `separate_sweeps` fp32
at (12, 4, T = 50), `separate_sweeps` fp32 at (32, 8, T = 100)) and, for the column / wavefront choice of the residual
at n = 32 in fp64, the default fp64 plan at (32, 8, T = 100); batch 4096 and 1024; 8 columns, and 16 too on the n = 32
plans.  Per plan, batch and column count C the time of
    residual_multi       norms only, float64 vecs and sol (what a refinement round reads): one call
    residual_xC          C calls of sip_lqr_residual, the same arguments column by column
    refine_multi_1,2,3   sip_lqr_refine_multi from zero with 1, 2 and 3 rounds
    refine_1,2,3_xC      C calls of sip_lqr_refine
    solve_multi          sip_lqr_solve_multi on the C columns
Next to the residual the bytes the multi-column form has to move (mats once per group of columns a launch carries,
vecs and sol of every column once) and what those take at 6.3 TB/s, the streaming rate measured on an MI355X.

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the calls alternate.  `range_ms` is max - min over the blocks.  One JSON record per plan, batch and column count,
printed and written to --out as a JSON list.

    python tools/bench_refine_multi.py [--batches 4096,1024] [--blocks 9] [--launches 8] [--plans "C4 fp64"]
                                       [--out profiles/refine_multi_bench.json]"""
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
# (label, n, m, T, dtype, constructor arguments, column counts, with the refinement)
PLANS = [("C3 fp64", 12, 4, 50, torch.float64, {}, (8,), True),
         ("C3 fp32 fused_f32 + separate_sweeps", 12, 4, 50, torch.float32, {"fused_f32": True, "separate_sweeps": True},
          (8,), True),
         ("C4 fp32 separate_sweeps", 32, 8, 100, torch.float32, {"separate_sweeps": True}, (8, 16), True),
         ("C4 fp64 (residual only)", 32, 8, 100, torch.float64, {}, (8,), False)]


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


def one(args, label, n, m, T, dtype, kwargs, batch, C, with_refine):
    shape = ChainShape(n, m, T)
    mats64, vecs64 = synthetic.make_chain_batch(shape, batch, seed=1, device="cuda:0", dtype=torch.float64,
                                                cross_term=0.01)
    mats = mats64.to(dtype)
    del mats64
    s = BatchedChainLQR(n, m, T, batch, dtype=dtype, **kwargs)
    gains, status = s.factor(mats)
    # columns: the right-hand side scaled by powers of two, so that every column is a problem of the same kind
    f = torch.tensor([(-1.0) ** c * 2.0 ** (c - C // 2) for c in range(C)], dtype=torch.float64, device="cuda:0")
    cols64 = (f[:, None, None] * vecs64[None]).contiguous()
    cols = cols64.to(dtype)
    sol = s.solve_multi(mats, cols, gains)
    sol64 = sol.double()
    torch.cuda.synchronize()
    assert (status == 0).all().item()
    group = s.residual_multi_columns

    def each(fn):
        def run():
            for c in range(C):
                fn(c)
        return run

    calls = {"residual_multi": lambda: s.residual_multi(mats, cols64, sol64, want_vector=False),
             "residual_x%d" % C: each(lambda c: s.residual(mats, cols64[c], sol64[c], want_vector=False)),
             "solve_multi": lambda: s.solve_multi(mats, cols, gains, sol)}
    if with_refine:
        for it in (1, 2, 3):
            calls["refine_multi_%d" % it] = lambda it=it: s.refine_multi(mats, cols64, gains, iterations=it)
            calls["refine_%d_x%d" % (it, C)] = each(lambda c, it=it: s.refine(mats, cols64[c], gains, iterations=it))
    got = alternating(calls, args.blocks, args.launches)
    ms = {k: round(v[0], 4) for k, v in got.items()}
    esize = mats.element_size()
    launches = -(-C // group)
    moved = batch * (launches * shape.mats_len * esize + C * 2 * shape.vecs_len * 8)
    rec = {"plan": label, "shape": [n, m, T, batch], "columns": C, "kernel": s.kernel_name,
           "residual_multi_columns_per_launch": group, "residual_multi_launches": launches,
           "blocks": args.blocks, "launches": args.launches, "library": load_library().sip_lqr_version().decode(),
           "ms": ms, "range_ms": {k: round(v[1], 4) for k, v in got.items()},
           "residual_multi_bytes": moved,
           "residual_multi_ms_at_%.1f_TBps" % STREAM_TBPS: round(moved / (STREAM_TBPS * 1e12) * 1e3, 4),
           "residual_multi_TBps": round(moved / (ms["residual_multi"] * 1e-3) / 1e12, 3),
           "residual_multi_over_singles": round(ms["residual_multi"] / ms["residual_x%d" % C], 4)}
    if with_refine:
        for it in (1, 2, 3):
            rec["refine_multi_%d_over_singles" % it] = round(ms["refine_multi_%d" % it] / ms["refine_%d_x%d" % (it, C)], 4)
        # what three rounds reach, and that the two ways agree: norms by round, worst over problems and columns
        # relative to each column's right-hand side
        ref, norms = s.refine_multi(mats, cols64, gains, iterations=3)
        single = torch.stack([s.refine(mats, cols64[c], gains, iterations=3)[0] for c in range(C)])
        torch.cuda.synchronize()
        scale = cols64.abs().amax(dim=(1, 2))
        rec["worst_relative_norm_by_round"] = [float(v) for v in (norms / scale[None, :, None]).amax(dim=(1, 2)).tolist()]
        rec["max_rel_difference_to_column_by_column"] = float(
            ((ref - single).abs().amax(dim=(1, 2)) / single.abs().amax(dim=(1, 2))).max().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--plans", default="", help="only the plans whose label contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_multi_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_refine_multi.py needs a GPU"
    records = []
    for label, n, m, T, dtype, kwargs, counts, with_refine in PLANS:
        if args.plans not in label:
            continue
        for batch in (int(b) for b in args.batches.split(",")):
            for C in counts:
                records.append(one(args, label, n, m, T, dtype, kwargs, batch, C, with_refine))
                print(json.dumps(records[-1]), flush=True)
                torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Separate factor / solve sweeps of the fused fp32 chain kernel (chain_factor_qf32, chain_solve_cols_qf32) against
the fused_f32-only plan, on which every split call re-runs the full sweep and solve_multi goes column by column:
sip_lqr_factor, sip_lqr_solve and sip_lqr_solve_multi with 1, 8 and 16 columns on a `fused_f32` plan and on a
`fused_f32` + `separate_sweeps` plan in one process, at (12, 4), T = 50, batch 4096 and batch 1024.  Next to them the
full sweep (sip_lqr_factor_solve, the same kernel on both plans) and the default fp64 plan's factor, solve and
solve_multi(8).

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the plans alternate, so that a drift of the machine hits all of them.  `range_ms` is max - min over the blocks: the
run-to-run spread.  One JSON record per batch with the times (ms), the ratios opt-in / fused_f32-only and, at batch
4096, the conditions the feature was asked to meet:
    solve_multi(8) <= fused_f32-only solve_multi(8) / 2,
    factor, solve  <= one full sweep of the fused kernel + the spread of that sweep over its blocks.
The records are printed and written to --out as a JSON list.

    python tools/bench_qf32_sweeps.py [--n 12] [--m 4] [--T 50] [--batches 4096,1024] [--blocks 9] [--launches 8]
                                      [--out profiles/qf32_sweeps_bench.json]"""
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


def one_batch(args, batch):
    n, m, T = args.n, args.m, args.T
    shape = ChainShape(n, m, T)
    f32, f64 = torch.float32, torch.float64
    mats64, vecs64 = synthetic.make_chain_batch(shape, batch, seed=1, device="cuda:0", dtype=f64, cross_term=0.01)
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    cols64 = torch.randn(16, batch, shape.vecs_len, dtype=f64, device="cuda:0", generator=gen)
    data = {f32: (mats64.to(f32), vecs64.to(f32), cols64.to(f32)), f64: (mats64, vecs64, cols64)}
    plans = {"fused_f32": BatchedChainLQR(n, m, T, batch, dtype=f32, fused_f32=True),
             "separate": BatchedChainLQR(n, m, T, batch, dtype=f32, fused_f32=True, separate_sweeps=True),
             "fp64": BatchedChainLQR(n, m, T, batch, dtype=f64)}
    assert plans["fused_f32"].has_fused_f32 and not plans["fused_f32"].has_separate_sweeps
    assert plans["separate"].has_fused_f32 and plans["separate"].has_separate_sweeps
    of = {k: data[s.dtype] for k, s in plans.items()}
    gains = {k: s.factor(of[k][0])[0] for k, s in plans.items()}
    sol = {k: s.empty_sol() for k, s in plans.items()}
    sol_cols = {k: torch.empty_like(of[k][2]) for k in plans}
    torch.cuda.synchronize()
    assert all((s.status == 0).all().item() for s in plans.values())
    calls = {"factor_solve": lambda k: plans[k].factor_solve(of[k][0], of[k][1], sol[k], gains[k]),
             "solve": lambda k: plans[k].solve(of[k][0], of[k][1], gains[k], sol[k]),
             "solve_multi_1": lambda k: plans[k].solve_multi(of[k][0], of[k][2][:1], gains[k], sol_cols[k][:1]),
             "solve_multi_8": lambda k: plans[k].solve_multi(of[k][0], of[k][2][:8], gains[k], sol_cols[k][:8]),
             "solve_multi_16": lambda k: plans[k].solve_multi(of[k][0], of[k][2], gains[k], sol_cols[k]),
             "factor": lambda k: plans[k].factor(of[k][0], gains[k])}
    ms, spread, ratio = {}, {}, {}
    # (factor_solve first and factor last: the solves in between need the state a factor call left)
    for what in ("factor_solve", "solve", "solve_multi_1", "solve_multi_8", "solve_multi_16", "factor"):
        who = [k for k in plans if k != "fp64" or what in ("factor", "solve", "solve_multi_8", "factor_solve")]
        launches = max(1, args.launches // 4) if what in ("solve_multi_8", "solve_multi_16") else args.launches
        got = alternating({k: (lambda k=k: calls[what](k)) for k in who}, args.blocks, launches)
        if what == "factor_solve":          # factor() restores the state the split solves read
            for k in who:
                plans[k].factor(of[k][0], gains[k])
        ms[what] = {k: round(v[0], 4) for k, v in got.items()}
        spread[what] = {k: round(v[1], 4) for k, v in got.items()}
        ratio[what] = round(got["separate"][0] / got["fused_f32"][0], 4)
    out = {"shape": [n, m, T, batch], "kernels": {k: s.kernel_name for k, s in plans.items()}, "blocks": args.blocks,
           "launches": args.launches, "library": load_library().sip_lqr_version().decode(), "ms": ms, "range_ms": spread,
           "separate_over_fused_f32": ratio}
    sweep, sweep_range = ms["factor_solve"]["fused_f32"], spread["factor_solve"]["fused_f32"]
    out["full_sweep_ms"], out["full_sweep_range_ms"] = sweep, sweep_range
    if batch == 4096:
        out["conditions"] = {"solve_multi_8<=fused_f32/2": ratio["solve_multi_8"] <= 0.5,
                             "factor<=full_sweep+range": ms["factor"]["separate"] <= sweep + sweep_range,
                             "solve<=full_sweep+range": ms["solve"]["separate"] <= sweep + sweep_range}
    # the same state, the same answers: the two fp32 plans agree on a solve to rounding
    a, b = (plans[k].solve(of[k][0], of[k][1], gains[k], sol[k]).double() for k in ("fused_f32", "separate"))
    out["max_rel_difference_of_the_two_solves"] = float(((a - b).abs().max() / a.abs().max()).item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qf32_sweeps_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qf32_sweeps.py needs a GPU"
    records = []
    for batch in (int(b) for b in args.batches.split(",")):
        records.append(one_batch(args, batch))
        print(json.dumps(records[-1]), flush=True)
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The n = 32 matrix-core chain kernels for 12 and 16 controls (opt-in: sip_lqr_plan_set_wide_controls) against what
the same plan runs on without the opt-in (the general engine: a factor launch and a solve launch), in one process and
one library:

  factor_solve   (32, 16) and (32, 12), T = 100, batch 4096 and 1024, fp64 and fp32 (the exact rows)
  factor_solve   (24, 12), (17, 9), (16, 16), (12, 12), T = 50, batch 4096, fp64 (embedded in a row)
  with separate sweeps at (32, 16), T = 100, batch 4096, fp64 and fp32: factor, solve, solve_multi(16)

Per cell both plans are warmed, then their blocks alternate within every repetition (so that a drift of the machine hits
both); a block is a number of launches between two device events -- `--launches` for the opt-in plan, `--base-launches`
for the general engine, which takes two orders of magnitude longer per launch.  Reported per plan: the median block time
(ms per launch) and the spread (min, max) over the repetitions; per cell the ratio, whether the opt-in is the faster
plan -- the condition the rows were accepted on at n > 16 -- and, for factor_solve, the bytes no scheme can avoid (inputs
read once, outputs written once) as a fraction of 8 TB/s at the opt-in plan's time.  (16, 16) and (12, 12) are a
32 x 32 embedding of a small problem: their figures say when not to opt in.  One JSON document on stdout (and in --out).

    python tools/bench_wide_controls.py [--blocks 5] [--launches 10] [--base-launches 2] [--out profiles/wide_controls_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sip_optimal_control_amd import BatchedChainLQR, ChainShape, synthetic
from sip_optimal_control_amd._lib import load_library

PEAK_BYTES_PER_S = 8e12
F64, F32 = torch.float64, torch.float32
FUSED = [(n, m, 100, batch, dtype) for n, m in ((32, 16), (32, 12)) for batch in (4096, 1024) for dtype in (F64, F32)]
FUSED += [(n, m, 50, 4096, F64) for n, m in ((24, 12), (17, 9), (16, 16), (12, 12))]
SEPARATE = [(32, 16, 100, 4096, dtype) for dtype in (F64, F32)]
MULTI_COLUMNS = 16


def block_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def alternating(fns, launches, blocks):
    """fns: {name: callable}; launches: {name: launches per block}; the block times of `blocks` repetitions, the plans
    taken in turn within each."""
    for name, fn in fns.items():  # warm-up: code objects, the allocator, the clocks
        for _ in range(min(3, launches[name])):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(block_ms(fn, launches[name]))
    return times


def algorithmic_bytes(n, m, T, batch, esize):
    """Inputs read once, outputs written once (mats, vecs; sol, gains, status): what no scheme can avoid."""
    mats = (T + 1) * (n * n + n) + T * (n * n + 2 * n * m + m * m)
    vecs = (T + 1) * 2 * n + T * m
    return batch * (esize * (mats + 2 * vecs + T * (m * n + m)) + 4)


def record(what, shape, dtype, plans, fns, args):
    n, m, T, batch = shape
    launches = {"wide": args.launches, "general": args.base_launches}
    times = alternating(fns, launches, args.blocks)
    assert all(bool((s.status == 0).all().item()) for s in plans.values())
    med = {k: statistics.median(t) for k, t in times.items()}
    out = {"call": what, "shape": [n, m, T, batch], "dtype": str(dtype).replace("torch.", ""),
           "kernels": {k: s.kernel_name for k, s in plans.items()},
           "launches_per_block": launches,
           "ms": {k: {"median": round(med[k], 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                  for k, t in times.items()},
           "general_over_wide": round(med["general"] / med["wide"], 2),
           "wide_faster_than_general": med["wide"] < med["general"]}
    if what == "factor_solve":
        esize = 8 if dtype == F64 else 4
        need = algorithmic_bytes(n, m, T, batch, esize)
        out["algorithmic_bytes"] = need
        out["wide_algorithmic_fraction_of_8TBps"] = round(need / (med["wide"] * 1e-3) / PEAK_BYTES_PER_S, 4)
    return out


def make(n, m, T, batch, dtype):
    mats, vecs = synthetic.make_chain_batch(ChainShape(n, m, T), batch, seed=1, device="cuda:0", dtype=F64, cross_term=0.01)
    return mats.to(dtype), vecs.to(dtype)


def fused_cell(n, m, T, batch, dtype, args):
    mats, vecs = make(n, m, T, batch, dtype)
    plans = {"wide": BatchedChainLQR(n, m, T, batch, dtype=dtype, wide_controls=True),
             "general": BatchedChainLQR(n, m, T, batch, dtype=dtype)}
    assert plans["wide"].has_wide_controls and "tree_generic" in plans["general"].kernel_name
    out = {k: (s.empty_sol(), s.empty_gains()) for k, s in plans.items()}
    fns = {k: (lambda k=k: plans[k].factor_solve(mats, vecs, *out[k])) for k in plans}
    rec = record("factor_solve", (n, m, T, batch), dtype, plans, fns, args)
    a, b = out["wide"][0].double(), out["general"][0].double()
    rec["max_rel_difference_wide_vs_general"] = float(((a - b).abs().max() / b.abs().max()).item())
    return rec


def separate_cells(n, m, T, batch, dtype, args):
    mats, vecs = make(n, m, T, batch, dtype)
    plans = {"wide": BatchedChainLQR(n, m, T, batch, dtype=dtype, wide_controls=True, separate_sweeps=True),
             "general": BatchedChainLQR(n, m, T, batch, dtype=dtype)}
    assert plans["wide"].has_separate_sweeps and "tree_generic" in plans["general"].kernel_name
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    cols = torch.randn(MULTI_COLUMNS, batch, plans["wide"].shape.vecs_len, dtype=F64, device="cuda:0", generator=gen).to(dtype)
    gains = {k: s.empty_gains() for k, s in plans.items()}
    sol = {k: s.empty_sol() for k, s in plans.items()}
    sol_cols = {k: torch.empty_like(cols) for k in plans}
    for k, s in plans.items():  # the state the solves run against
        s.factor(mats, gains[k])
    calls = {"factor": lambda k: plans[k].factor(mats, gains[k]),
             "solve": lambda k: plans[k].solve(mats, vecs, gains[k], sol[k]),
             "solve_multi(%d)" % MULTI_COLUMNS: lambda k: plans[k].solve_multi(mats, cols, gains[k], sol_cols[k])}
    return [record(what, (n, m, T, batch), dtype, plans, {k: (lambda k=k, call=call: call(k)) for k in plans}, args)
            for what, call in calls.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--base-launches", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wide_controls.py needs a GPU"
    doc = {"library": load_library().sip_lqr_version().decode(), "device": torch.cuda.get_device_name(0),
           "blocks": args.blocks, "cells": []}

    def add(rec):
        doc["cells"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    for cell in FUSED:
        add(fused_cell(*cell, args))
    for cell in SEPARATE:
        for rec in separate_cells(*cell, args):
            add(rec)
    doc["wide_faster_than_general_in_every_cell_with_n_above_16"] = all(
        c["wide_faster_than_general"] for c in doc["cells"] if c["shape"][0] > 16)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fused fp32 chain kernel (chain_factor_solve_qf32, opt-in: sip_lqr_plan_set_fused_f32) against what an fp32 plan
runs on without the opt-in (the general engine: a factor launch and a solve launch) and against the default fp64 plan
of the same shape, in one process and one library: sip_lqr_factor_solve at every shape of the benchmark grid
n in {4, 6, 8, 12} x m in {1, 2, 3, 4} at batch 4096, T = 50, and at (12, 4) also at batch 1024.

Per shape the three plans are warmed, then their blocks alternate within every repetition (so that a drift of the
machine hits all three); a block is LAUNCHES launches between two device events.  Reported per plan: the median block
time (ms per launch) and the spread (min, max) over the repetitions.  Per shape also: the ratios, the bytes the sweep
has to move at the least (inputs once per sweep direction where a direction reads them, outputs and the spill once
each way) and the fraction of 8 TB/s that is at the fused plan's time, and whether the fused plan beats the general
engine -- the condition the kernel was accepted on at batch 4096.  One JSON document on stdout (and in --out).

    python tools/bench_fused_f32.py [--T 50] [--blocks 9] [--launches 10] [--out profiles/fused_f32_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sip_optimal_control_amd import BatchedChainLQR, ChainShape, synthetic
from sip_optimal_control_amd._lib import load_library

GRID = [(n, m) for n in (4, 6, 8, 12) for m in (1, 2, 3, 4)]
PEAK_BYTES_PER_S = 8e12


def block_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def alternating(fns, blocks, launches):
    """fns: {name: callable}; the block times of `blocks` repetitions, the plans taken in turn within each."""
    for fn in fns.values():  # warm-up: code objects, the allocator, the clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(block_ms(fn, launches))
    return times


def sweep_bytes(n, m, T, batch, esize):
    """Least traffic of one fused sweep: the backward sweep reads mats and vecs and writes the gains and the spill
    [S | g | h]; the rollout re-reads A | B and delta, reads the gains and the spill and writes sol."""
    mats = (T + 1) * (n * n + n) + T * (n * n + 2 * n * m + m * m)
    vecs = (T + 1) * 2 * n + T * m
    gains = T * (m * n + m)
    spill = (T + 1) * (n * n + 2 * n)
    again = T * (n * n + n * m) + (T + 1) * n
    return batch * esize * (mats + vecs + 2 * gains + 2 * spill + again + vecs)


def algorithmic_bytes(n, m, T, batch, esize):
    """Inputs read once, outputs written once (mats, vecs; sol, gains, status): what no scheme can avoid."""
    mats = (T + 1) * (n * n + n) + T * (n * n + 2 * n * m + m * m)
    vecs = (T + 1) * 2 * n + T * m
    return batch * (esize * (mats + 2 * vecs + T * (m * n + m)) + 4)


def shape_record(n, m, T, batch, args):
    shape = ChainShape(n, m, T)
    mats64, vecs64 = synthetic.make_chain_batch(shape, batch, seed=1, device="cuda:0", dtype=torch.float64, cross_term=0.01)
    mats32, vecs32 = mats64.float(), vecs64.float()
    plans = {"f32_fused": BatchedChainLQR(n, m, T, batch, dtype=torch.float32, fused_f32=True),
             "f32_general": BatchedChainLQR(n, m, T, batch, dtype=torch.float32),
             "f64_default": BatchedChainLQR(n, m, T, batch, dtype=torch.float64)}
    assert plans["f32_fused"].has_fused_f32 and not plans["f32_general"].has_fused_f32
    data = {"f32_fused": (mats32, vecs32), "f32_general": (mats32, vecs32), "f64_default": (mats64, vecs64)}
    out = {k: (s.empty_sol(), s.empty_gains()) for k, s in plans.items()}
    fns = {k: (lambda k=k: plans[k].factor_solve(*data[k], *out[k])) for k in plans}
    times = alternating(fns, args.blocks, args.launches)
    assert all(bool((s.status == 0).all().item()) for s in plans.values())
    med = {k: statistics.median(t) for k, t in times.items()}
    need = sweep_bytes(n, m, T, batch, 4)
    a, b = out["f32_fused"][0].double(), out["f64_default"][0]
    return {"shape": [n, m, T, batch], "kernels": {k: s.kernel_name for k, s in plans.items()},
            "ms": {k: {"median": round(med[k], 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                   for k, t in times.items()},
            "fused_over_general": round(med["f32_fused"] / med["f32_general"], 4),
            "fused_over_f64": round(med["f32_fused"] / med["f64_default"], 4),
            "f32_sweep_bytes": need, "f64_sweep_bytes": 2 * need,
            "f32_algorithmic_bytes": algorithmic_bytes(n, m, T, batch, 4),
            "fused_algorithmic_fraction_of_8TBps": round(
                algorithmic_bytes(n, m, T, batch, 4) / (med["f32_fused"] * 1e-3) / PEAK_BYTES_PER_S, 4),
            "fused_fraction_of_8TBps": round(need / (med["f32_fused"] * 1e-3) / PEAK_BYTES_PER_S, 4),
            "fused_faster_than_general": med["f32_fused"] < med["f32_general"],
            "max_rel_difference_fused_f32_vs_f64": float(((a - b).abs().max() / b.abs().max()).item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fused_f32.py needs a GPU"
    doc = {"library": load_library().sip_lqr_version().decode(), "device": torch.cuda.get_device_name(0),
           "blocks": args.blocks, "launches": args.launches, "shapes": []}
    for n, m, batch in [(n, m, 4096) for n, m in GRID] + [(12, 4, 1024)]:
        doc["shapes"].append(shape_record(n, m, args.T, batch, args))
        print(json.dumps(doc["shapes"][-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    doc["fused_faster_than_general_at_every_grid_shape_at_batch_4096"] = all(
        s["fused_faster_than_general"] for s in doc["shapes"] if s["shape"][3] == 4096)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

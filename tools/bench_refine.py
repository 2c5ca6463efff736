#!/usr/bin/env python3
"""The KKT residual (sip_lqr_residual) and the refinement built on it (sip_lqr_refine) against the solve they
accompany: for the default fp64 plan and the `fused_f32` + `separate_sweeps` fp32 plan at C3's shape (12, 4, T = 50)
and the `separate_sweeps` fp32 plan at C4's shape (32, 8, T = 100), at batch 4096 and 1024, the time of
    residual            norms only, vecs and sol in the plan's dtype
    residual_wide       the same with float64 vecs and sol (what a refinement round reads)
    residual_vector     with the fp64 residual vector written as well
    solve               sip_lqr_solve against the factor state (the kernel this change does not touch)
    refine_1, _2, _3    sip_lqr_refine from zero with 1, 2 and 3 rounds (each round: scaled residual, solve, update;
                        then one more residual)
Next to each residual the bytes it has to move (mats, vecs and sol once; + the vector written) and what those bytes
take at 6.3 TB/s, the streaming rate measured on an MI355X.

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the calls alternate.  `range_ms` is max - min over the blocks.  One JSON record per plan and batch, printed and
written to --out as a JSON list.

    python tools/bench_refine.py [--batches 4096,1024] [--blocks 9] [--launches 8] [--out profiles/refine_bench.json]"""
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


def one(args, label, n, m, T, dtype, kwargs, batch):
    shape = ChainShape(n, m, T)
    mats64, vecs64 = synthetic.make_chain_batch(shape, batch, seed=1, device="cuda:0", dtype=torch.float64,
                                                cross_term=0.01)
    mats, vecs = mats64.to(dtype), vecs64.to(dtype)
    del mats64
    s = BatchedChainLQR(n, m, T, batch, dtype=dtype, **kwargs)
    gains, status = s.factor(mats)
    sol = s.solve(mats, vecs, gains)
    sol64 = sol.double()
    torch.cuda.synchronize()
    assert (status == 0).all().item()
    calls = {"residual": lambda: s.residual(mats, vecs, sol, want_vector=False),
             "residual_wide": lambda: s.residual(mats, vecs64, sol64, want_vector=False),
             "residual_vector": lambda: s.residual(mats, vecs, sol),
             "solve": lambda: s.solve(mats, vecs, gains, sol),
             "refine_1": lambda: s.refine(mats, vecs64, gains, iterations=1),
             "refine_2": lambda: s.refine(mats, vecs64, gains, iterations=2),
             "refine_3": lambda: s.refine(mats, vecs64, gains, iterations=3)}
    got = alternating(calls, args.blocks, args.launches)
    esize = mats.element_size()
    moved = {"residual": batch * (shape.mats_len * esize + 2 * shape.vecs_len * esize),
             "residual_wide": batch * (shape.mats_len * esize + 2 * shape.vecs_len * 8),
             "residual_vector": batch * (shape.mats_len * esize + 2 * shape.vecs_len * esize + shape.vecs_len * 8)}
    ms = {k: round(v[0], 4) for k, v in got.items()}
    # what three rounds reach: the norms by round and the change of the solution against the plain solve
    ref, norms = s.refine(mats, vecs64, gains, iterations=3)
    torch.cuda.synchronize()
    return {"plan": label, "shape": [n, m, T, batch], "kernel": s.kernel_name, "blocks": args.blocks,
            "launches": args.launches, "library": load_library().sip_lqr_version().decode(), "ms": ms,
            "range_ms": {k: round(v[1], 4) for k, v in got.items()},
            "residual_bytes": moved,
            "residual_ms_at_%.1f_TBps" % STREAM_TBPS: {k: round(b / (STREAM_TBPS * 1e12) * 1e3, 4) for k, b in moved.items()},
            "residual_TBps": {k: round(b / (ms[k] * 1e-3) / 1e12, 3) for k, b in moved.items()},
            "residual_over_solve": round(ms["residual"] / ms["solve"], 4),
            "refine_3_over_solve": round(ms["refine_3"] / ms["solve"], 4),
            "worst_norm_by_round": [float(v) for v in norms.max(dim=1).values.tolist()],
            "max_rel_change_of_the_solution": float(((ref - sol64).abs().max() / sol64.abs().max()).item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_refine.py needs a GPU"
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

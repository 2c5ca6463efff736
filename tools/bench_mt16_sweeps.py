#!/usr/bin/env python3
"""Separate factor / solve sweeps of the n = 32 matrix-core chain kernels against the plans' default (every split
call re-runs the fused sweep; solve_multi column by column): sip_lqr_factor, sip_lqr_solve and sip_lqr_solve_multi
with 8 and 16 columns on a default plan and on an opt-in plan (sip_lqr_plan_set_separate_sweeps) in one process, in
fp32 and fp64, at BASELINE's C4 shape (batch 4096, T = 100, n = 32, m = 8).

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the two plans alternate, so that a drift of the machine hits both.  One JSON line per dtype with the times (ms), the
ratios opt-in / default and the three conditions the feature was accepted on:
    factor <= default factor,   solve <= default solve,   solve_multi(8) <= default solve_multi(8) / 3.
--kkt adds the sip_kkt_factor_theta time of a (32, 8), T = 20, batch 1024, p = 8 Newton-KKT plan with
sip_kkt_plan_set_chain_separate_sweeps off and on (reported, no condition).

    python tools/bench_mt16_sweeps.py [--batch 4096] [--T 100] [--m 8] [--blocks 7] [--launches 8] [--dtypes float32,float64] [--kkt]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sip_optimal_control_amd import BatchedChainLQR, BatchedNewtonKKT, ChainShape, synthetic

N = 32


def block_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def alternating_medians(fns, blocks, launches):
    """fns: {name: callable}; medians of `blocks` blocks each, the blocks taken in turn."""
    for fn in fns.values():  # warm-up: code objects, the allocator, the clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(block_ms(fn, launches))
    return {name: statistics.median(t) for name, t in times.items()}


def chain(dtype, args):
    shape = ChainShape(N, args.m, args.T)
    mats, vecs = synthetic.make_chain_batch(shape, args.batch, seed=1, device="cuda:0", dtype=dtype, cross_term=0.01)
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    cols = torch.randn(16, args.batch, shape.vecs_len, dtype=dtype, device="cuda:0", generator=gen)
    sol_cols = torch.empty_like(cols)
    plans = {"default": BatchedChainLQR(N, args.m, args.T, args.batch, dtype=dtype),
             "separate": BatchedChainLQR(N, args.m, args.T, args.batch, dtype=dtype, separate_sweeps=True)}
    assert plans["separate"].has_separate_sweeps and not plans["default"].has_separate_sweeps
    gains = {k: s.factor(mats)[0] for k, s in plans.items()}
    sol = {k: s.empty_sol() for k, s in plans.items()}
    torch.cuda.synchronize()
    assert all((s.status == 0).all().item() for s in plans.values())
    out = {"dtype": str(dtype).replace("torch.", ""), "shape": [N, args.m, args.T, args.batch],
           "kernels": {k: s.kernel_name for k, s in plans.items()}, "blocks": args.blocks, "launches": args.launches}
    calls = {"factor": lambda k: plans[k].factor(mats, gains[k]),
             "solve": lambda k: plans[k].solve(mats, vecs, gains[k], sol[k]),
             "solve_multi_8": lambda k: plans[k].solve_multi(mats, cols[:8], gains[k], sol_cols[:8]),
             "solve_multi_16": lambda k: plans[k].solve_multi(mats, cols, gains[k], sol_cols)}
    ms, ratio = {}, {}
    for what in ("solve", "solve_multi_8", "solve_multi_16", "factor"):  # (factor last: the others need its state)
        launches = max(1, args.launches // 4) if what.startswith("solve_multi") else args.launches
        med = alternating_medians({k: (lambda k=k: calls[what](k)) for k in plans}, args.blocks, launches)
        ms[what] = {k: round(v, 4) for k, v in med.items()}
        ratio[what] = round(med["separate"] / med["default"], 4)
    out["ms"], out["separate_over_default"] = ms, ratio
    out["conditions"] = {"factor<=default": ratio["factor"] <= 1.0, "solve<=default": ratio["solve"] <= 1.0,
                         "solve_multi_8<=default/3": ratio["solve_multi_8"] <= 1.0 / 3.0}
    # the same state, the same answers: the two plans agree on a solve to rounding
    a, b = (plans[k].solve(mats, vecs, gains[k], sol[k]).double() for k in ("default", "separate"))
    out["max_rel_difference_of_the_two_solves"] = float(((a - b).abs().max() / a.abs().max()).item())
    return out


def kkt_theta(args):
    n, m, T, batch, p = N, 8, 20, 1024, 8
    c, g = n // 2, 2 * m
    dims = dict(parents=list(range(T)), children=list(range(1, T + 1)), state_dims=[n] * (T + 1),
                control_dims=[m] * T, node_c_dims=[0] * T + [c], node_g_dims=[0] * T + [g],
                edge_c_dims=[c] * T, edge_g_dims=[g] * T)
    out = {"kkt_factor_theta": {"shape": [n, m, T, batch], "p": p}}
    fns, plans = {}, {}
    for name, on in (("default", False), ("separate", True)):
        kkt = BatchedNewtonKKT(batch=batch, theta_dim=p, chain_separate_sweeps=on, **dims)
        model, w, r1, r2, r3, _ = synthetic.make_newton_kkt_batch(kkt, seed=1, r2_max=1e2, **dims)
        gen = torch.Generator(device=kkt.device).manual_seed(3)
        theta_model = 1e-3 * torch.randn(batch, kkt.theta_len, dtype=torch.float64, device=kkt.device, generator=gen)
        r1 = torch.cat([r1, torch.full((batch, p), 100.0, dtype=torch.float64, device=kkt.device)], dim=1)
        plans[name] = kkt
        fns[name] = lambda kkt=kkt, a=(model, theta_model, w, r1, r2, r3): kkt.factor_theta(*a)
        out["kkt_factor_theta"][name + "_kernel"] = kkt.kernel_name
    med = alternating_medians(fns, args.blocks, args.launches)
    out["kkt_factor_theta"]["ms"] = {k: round(v, 4) for k, v in med.items()}
    out["kkt_factor_theta"]["separate_over_default"] = round(med["separate"] / med["default"], 4)
    out["kkt_factor_theta"]["problems_with_nonzero_status"] = {k: int((s.status != 0).sum().item()) for k, s in plans.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--m", type=int, default=8, choices=(4, 8))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--kkt", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mt16_sweeps.py needs a GPU"
    for name in args.dtypes.split(","):
        print(json.dumps(chain(getattr(torch, name), args)), flush=True)
        torch.cuda.empty_cache()
    if args.kkt:
        print(json.dumps(kkt_theta(args)), flush=True)


if __name__ == "__main__":
    main()

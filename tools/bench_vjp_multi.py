#!/usr/bin/env python3
"""The backward pass of solve_multi (sip_lqr_vjp_multi) and its gradient kernel (sip_lqr_vjp_mats_multi) against the
single-column route they replace and the forward pass they accompany: for the default fp64 plan and the `fused_f32` +
`separate_sweeps` fp32 plan at C3's shape (12, 4, T = 50) and the `separate_sweeps` fp32 plan at C4's shape
(32, 8, T = 100), at batch 4096 and 1024, with 8 columns (and 16 at C4), the time of
    vjp_mats_multi      the kernel alone: num_rhs columns of sol and adj read, ONE grad_mats written
    singles_mats        num_rhs x sip_lqr_vjp_mats and num_rhs - 1 in-place additions into a preallocated buffer
    vjp_multi           sip_lqr_vjp_multi: the adjoint solve_multi, the status mask and the kernel
    singles_vjp         num_rhs x sip_lqr_vjp and the num_rhs - 1 additions
    forward             sip_lqr_factor + sip_lqr_solve_multi of the same plan
    shape <w>,<KiB>     the kernel alone with <w> wavefronts per workgroup and the run that <KiB> KiB of operands hold
                        (through SIP_LQR_VJP_COLS_SHAPE): the candidates of the launch shape, DESIGN 4.11.2
    columns <c>         the kernel alone in groups of <c> columns (SIP_LQR_VJP_MULTI_COLUMNS)
Next to the kernel the bytes it has to move (2 num_rhs vecs-sized reads, one mats-sized write) and what those bytes
take at 6.3 TB/s, the streaming rate measured on an MI355X.

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the calls alternate.  `range_ms` is max - min over the blocks.  One JSON record per plan, batch and column count,
printed and written to --out as a JSON list (--append: added to the list already there).

    python tools/bench_vjp_multi.py [--plans 0,1,2] [--batches 4096,1024] [--blocks 7] [--launches 4]
                                    [--shapes "8,16;8,32;8,64;4,16;4,32;4,64"] [--columns "4;2"] [--append]
                                    [--out profiles/vjp_multi_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from bench_vjp import PLANS, STREAM_TBPS, alternating
from sip_optimal_control_amd import BatchedChainLQR, ChainShape, synthetic
from sip_optimal_control_amd._lib import load_library


def with_env(name, value, fn):
    """fn under name=value (the library reads both aids per call)."""
    def call():
        os.environ[name] = value
        try:
            fn()
        finally:
            del os.environ[name]
    return call


def run_for(n, m, T, columns, kib):
    """The longest run whose `columns` columns of pairs fit kib KiB (at least one stage)."""
    fixed, stage = columns * 2 * n * 16, columns * (2 * n + m) * 16
    return max(1, min((kib * 1024 - fixed) // stage, T + 1))


def one(args, label, n, m, T, dtype, kwargs, batch, cols):
    shape = ChainShape(n, m, T)
    mats64, _ = synthetic.make_chain_batch(shape, batch, seed=1, device="cuda:0", dtype=torch.float64, cross_term=0.01)
    mats = mats64.to(dtype)
    del mats64
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    draw = lambda: torch.randn(cols, batch, shape.vecs_len, dtype=torch.float64, device="cuda:0", generator=gen).to(dtype)
    vecs_cols, g_cols = draw(), draw()
    s = BatchedChainLQR(n, m, T, batch, dtype=dtype, **kwargs)
    gains, status = s.factor(mats)
    sol_cols = s.solve_multi(mats, vecs_cols, gains)
    grad_mats, lam_cols = s.vjp_multi(mats, sol_cols, g_cols, gains)
    torch.cuda.synchronize()
    assert (status == 0).all().item() and torch.isfinite(grad_mats).all().item()
    per_launch = min(cols, s.vjp_multi_columns)
    kernel = lambda: s.vjp_mats_multi(sol_cols, lam_cols, grad_mats=grad_mats)
    total, part = torch.empty_like(grad_mats), torch.empty_like(grad_mats)

    def singles_mats():
        s.vjp_mats(sol_cols[0], lam_cols[0], grad_mats=total)
        for c in range(1, cols):
            s.vjp_mats(sol_cols[c], lam_cols[c], grad_mats=part)
            total.add_(part)

    def singles_vjp():
        first, _ = s.vjp(mats, sol_cols[0], g_cols[0], gains)
        for c in range(1, cols):
            more, _ = s.vjp(mats, sol_cols[c], g_cols[c], gains)
            first.add_(more)

    def forward():
        s.factor(mats, gains)
        s.solve_multi(mats, vecs_cols, gains, sol_cols)

    calls = {"vjp_mats_multi": kernel, "singles_mats": singles_mats,
             "vjp_multi": lambda: s.vjp_multi(mats, sol_cols, g_cols, gains),
             "singles_vjp": singles_vjp, "forward": forward}
    aids = {}
    for cand in filter(None, args.shapes.split(";")):
        waves, kib = (int(v) for v in cand.split(","))
        aids["shape " + cand] = with_env("SIP_LQR_VJP_COLS_SHAPE", "%d,%d" % (waves, run_for(n, m, T, per_launch, kib)),
                                         kernel)
    for cand in filter(None, args.columns.split(";")):
        aids["columns " + cand] = with_env("SIP_LQR_VJP_MULTI_COLUMNS", cand, kernel)
    reference = grad_mats.clone()
    for name, call in aids.items():  # every candidate computes the same bits in fp64, and is finite in fp32
        grad_mats.fill_(float("nan"))
        call()
        assert torch.isfinite(grad_mats).all().item(), name
        assert name.startswith("columns") and dtype == torch.float32 or torch.equal(grad_mats, reference), name
    singles_mats()
    torch.cuda.synchronize()
    scale = reference.abs().max().item()
    assert (total - reference).abs().max().item() <= (1e-5 if dtype == torch.float32 else 1e-13) * scale
    calls.update(aids)
    got = alternating(calls, args.blocks, args.launches)
    esize = mats.element_size()
    moved = batch * (shape.mats_len + 2 * cols * shape.vecs_len) * esize
    ms = {k: round(v[0], 4) for k, v in got.items()}
    floor = moved / (STREAM_TBPS * 1e12) * 1e3
    return {"plan": label, "shape": [n, m, T, batch], "columns": cols, "columns_per_launch": s.vjp_multi_columns,
            "kernel": s.kernel_name, "blocks": args.blocks, "launches": args.launches,
            "library": load_library().sip_lqr_version().decode(), "ms": ms,
            "range_ms": {k: round(v[1], 4) for k, v in got.items()},
            "vjp_mats_multi_bytes": moved,
            "vjp_mats_multi_ms_at_%.1f_TBps" % STREAM_TBPS: round(floor, 4),
            "vjp_mats_multi_over_floor": round(ms["vjp_mats_multi"] / floor, 3),
            "vjp_mats_multi_TBps": round(moved / (ms["vjp_mats_multi"] * 1e-3) / 1e12, 3),
            "singles_mats_over_vjp_mats_multi": round(ms["singles_mats"] / ms["vjp_mats_multi"], 3),
            "singles_vjp_over_vjp_multi": round(ms["singles_vjp"] / ms["vjp_multi"], 3),
            "vjp_multi_over_forward": round(ms["vjp_multi"] / ms["forward"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", default="0,1,2")
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--shapes", default="8,16;8,32;8,64;4,16;4,32;4,64")
    ap.add_argument("--columns", default="4;2")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vjp_multi_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vjp_multi.py needs a GPU"
    records = []
    if args.append and os.path.exists(args.out):
        with open(args.out) as f:
            records = json.load(f)
    for index in (int(i) for i in args.plans.split(",")):
        label, n, m, T, dtype, kwargs = PLANS[index]
        for batch in (int(b) for b in args.batches.split(",")):
            for cols in (8, 16) if n == 32 else (8,):
                records.append(one(args, label, n, m, T, dtype, kwargs, batch, cols))
                print(json.dumps(records[-1]), flush=True)
                torch.cuda.empty_cache()
                with open(args.out, "w") as f:
                    json.dump(records, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()

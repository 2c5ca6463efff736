#!/usr/bin/env python3
"""The backward pass of the tree solve_multi (sip_lqr_tree_vjp_multi) and its gradient kernel
(sip_lqr_tree_vjp_input_multi) against the single-column route they replace and the forward pass they accompany, on the
reference's three variable-shape benchmark trees (BM_LQRVariableFactorSolve, benchmarks/lqr_benchmark.cpp:209-310) at
T = 63, batch 4096 and 1024, with 8 columns: the time of
    vjp_input_multi     the kernel alone: num_rhs columns of out and adj read, ONE grad_input written
    singles_input       num_rhs x sip_lqr_tree_vjp_input and num_rhs - 1 in-place additions into a preallocated buffer
    vjp_multi           sip_lqr_tree_vjp_multi: the adjoint solve_multi, the status mask and the kernel
    singles_vjp         num_rhs x sip_lqr_tree_vjp and the num_rhs - 1 additions
    forward             sip_lqr_tree_factor_fused + sip_lqr_tree_solve_multi of the same plan
    lds <KiB>           the kernel alone with <KiB> KiB of LDS for the staged columns (64: the rule; 147 or what 8 columns
                        need: the kernel's limit raised; 0: the direct form with 8 columns), through the third field of
                        SIP_LQR_TREE_VJP_COLS_SHAPE: the candidates of the launch shape, DESIGN 4.11.3
    columns <c>         the kernel alone in groups of at most <c> columns (SIP_LQR_TREE_VJP_MULTI_COLUMNS), staged, with
                        the kernel's limit raised where <c> columns need more than 64 KiB
Next to the kernel the bytes it has to move (2 num_rhs output-arena-sized reads, one input-arena-sized write) and what
those bytes take at 6.3 TB/s, the streaming rate measured on an MI355X.  (The table, 8 bytes per input-arena scalar,
is the same for every problem and stays in cache: it is not part of the floor.)

Each time is the median over BLOCKS blocks of LAUNCHES launches between two device events, after a warm-up; the blocks
of the calls alternate.  `range_ms` is max - min over the blocks.  One JSON record per tree and batch, printed and
written to --out as a JSON list.

    python tools/bench_tree_vjp_multi.py [--batches 4096,1024] [--columns-total 8] [--blocks 7] [--launches 4]
                                         [--lds "64;raised;0"] [--columns "4;2"]
                                         [--out profiles/tree_vjp_multi_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
from bench_tree_vjp import STREAM_TBPS, TREES, alternating
from sip_optimal_control_amd._lib import load_library
from sip_optimal_control_amd.tree import BatchedTreeLQR


def with_env(env, fn):
    """fn under the variables of `env` (the library reads both aids per call)."""
    def call():
        os.environ.update(env)
        try:
            fn()
        finally:
            for name in env:
                del os.environ[name]
    return call


def one(args, shape, batch):
    import full_batch_problems as fb
    cols = args.columns_total
    topo = fb.variable_benchmark_topology(shape, T=args.T)
    blocks = fb.make_blocks(topo, batch, np.random.default_rng(17 + 31 * shape), "variable_benchmark")  # distinct problems
    s = BatchedTreeLQR(topo.parents, topo.children, topo.sd, topo.cd, batch=batch)
    maps = fb.PlanMaps(s, topo)
    s.input.copy_(torch.from_numpy(maps.pack_input(s, *fb.to_oracle(topo, blocks))))
    del blocks
    gen = torch.Generator(device=s.device).manual_seed(2)
    draw = lambda: torch.randn(cols, batch, s.out_len, dtype=torch.float64, device=s.device, generator=gen)
    rhs_cols, g_cols = draw(), draw()
    status = s.factor_fused()
    out_cols = s.solve_multi(rhs_cols)
    grad_input, lam_cols = s.vjp_multi(g_cols, out_cols)
    torch.cuda.synchronize()
    assert (status == 0).all().item() and torch.isfinite(grad_input).all().item()
    kernel = lambda: s.vjp_input_multi(out_cols, lam_cols, grad_input=grad_input)
    total, part = torch.empty_like(grad_input), torch.empty_like(grad_input)

    def singles_input():
        s.vjp_input(out_cols[0], lam_cols[0], grad_input=total)
        for c in range(1, cols):
            s.vjp_input(out_cols[c], lam_cols[c], grad_input=part)
            total.add_(part)

    def singles_vjp():
        first, _ = s.vjp(g_cols[0], output=out_cols[0])
        for c in range(1, cols):
            more, _ = s.vjp(g_cols[c], output=out_cols[c])
            first.add_(more)

    def forward():
        s.factor_fused()
        s.solve_multi(rhs_cols, out_cols)

    calls = {"vjp_input_multi": kernel, "singles_input": singles_input,
             "vjp_multi": lambda: s.vjp_multi(g_cols, out_cols), "singles_vjp": singles_vjp, "forward": forward}
    raised = -(-min(cols, 8) * 16 * s.out_len // 1024)       # KiB that hold a full group of 8 columns
    aids, lds_kib = {}, {}
    for cand in filter(None, args.lds.split(";")):
        kib = raised if cand == "raised" else int(cand)
        if kib > 160:
            continue                                         # beyond what a workgroup may declare: no such candidate here
        lds_kib[cand] = kib
        aids["lds " + cand] = with_env({"SIP_LQR_TREE_VJP_COLS_SHAPE": "0,0,%d" % kib}, kernel)
    for cand in filter(None, args.columns.split(";")):       # staged: with the limit raised where <c> columns need it
        kib = max(64, -(-int(cand) * 16 * s.out_len // 1024))
        lds_kib["columns " + cand] = kib
        aids["columns " + cand] = with_env({"SIP_LQR_TREE_VJP_MULTI_COLUMNS": cand,
                                            "SIP_LQR_TREE_VJP_COLS_SHAPE": "0,0,%d" % kib}, kernel)
    reference = grad_input.clone()
    refused = {}
    for name, call in list(aids.items()):  # every candidate computes the same bits, or is refused by the runtime
        grad_input.fill_(float("nan"))
        try:
            call()
        except Exception as e:  # (the limit of dynamic LDS could not be raised that far: recorded, not timed)
            refused[name] = str(e)
            del aids[name]
            continue
        assert torch.equal(grad_input, reference), name
    singles_input()
    torch.cuda.synchronize()
    copy = torch.from_numpy(maps_copy_slots(topo)).to(s.device)
    scale = reference.abs().max().item()
    assert (total - reference)[:, ~copy].abs().max().item() <= 1e-13 * scale      # the same sum, grouped otherwise
    calls.update(aids)
    got = alternating(calls, args.blocks, args.launches)
    moved = batch * 8 * (s.in_len + 2 * cols * s.out_len)
    ms = {k: round(v[0], 4) for k, v in got.items()}
    floor = moved / (STREAM_TBPS * 1e12) * 1e3
    return {"tree": TREES[shape], "T": args.T, "batch": batch, "columns": cols, "input_len": s.in_len,
            "output_len": s.out_len, "columns_per_launch": s.vjp_multi_columns, "lds_kib": lds_kib, "refused": refused,
            "kernel": s.split_kernel_name, "multi_kernel": s.multi_kernel_name, "vjp_kernel": s.vjp_kernel_name,
            "vjp_multi_kernel": s.vjp_multi_kernel_name, "blocks": args.blocks, "launches": args.launches,
            "library": load_library().sip_lqr_version().decode(), "ms": ms,
            "range_ms": {k: round(v[1], 4) for k, v in got.items()},
            "vjp_input_multi_bytes": moved,
            "vjp_input_multi_ms_at_%.1f_TBps" % STREAM_TBPS: round(floor, 4),
            "vjp_input_multi_over_floor": round(ms["vjp_input_multi"] / floor, 3),
            "vjp_input_multi_TBps": round(moved / (ms["vjp_input_multi"] * 1e-3) / 1e12, 3),
            "singles_input_over_vjp_input_multi": round(ms["singles_input"] / ms["vjp_input_multi"], 3),
            "singles_vjp_over_vjp_multi": round(ms["singles_vjp"] / ms["vjp_multi"], 3),
            "vjp_multi_over_forward": round(ms["vjp_multi"] / ms["forward"], 4)}


def maps_copy_slots(topo):
    """[input_len] bool: the q, c, r slots of the input arena (where the single kernel writes lambda and this one 0)."""
    import tree_vjp_cases as tv
    zero = np.zeros((1, topo.layout.sol_len))
    return tv.grad_input(topo, zero, zero, dt=np.float64)[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,1024")
    ap.add_argument("--T", type=int, default=63)
    ap.add_argument("--columns-total", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--lds", default="64;raised;0")
    ap.add_argument("--columns", default="4;2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_vjp_multi_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tree_vjp_multi.py needs a GPU"
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

#!/usr/bin/env python3
"""The factorization and the single-right-hand-side solve of trees as separate sweeps (sip_lqr_tree_factor_fused /
sip_lqr_tree_solve_fused) against the general engine's sip_lqr_tree_factor / sip_lqr_tree_solve and the fused
factor + solve, on the reference's variable-shape benchmark trees (BM_LQRVariableFactorSolve,
benchmarks/lqr_benchmark.cpp:209-310); and sip_kkt_factor + sip_kkt_solve on a tree Newton-KKT plan of the same
shape with sip_kkt_plan_set_tree_fused off and on.  Every entry point is timed on its own (CUDA events over
--steps back-to-back launches).

    python tools/bench_tree_split.py [--batch 4096] [--T 63] [--n 8] [--steps 10] [--out f.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, steps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--T", type=int, default=63)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import reference_problems as rp
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    lqr = []
    for shape, name in enumerate(("heterogeneous_chain", "shallow_wide_tree", "binary_tree")):
        rng = np.random.default_rng(17 + 31 * shape)
        prob = rp.variable_benchmark_problem(shape, args.T, args.n, 2, rng)
        s = BatchedTreeLQR(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"],
                           batch=args.batch)
        s.pack([prob["blocks"]])                       # one instance ...
        s.input[1:] = s.input[0:1]                     # ... replicated over the batch
        t = {"general_factor_ms": timed(s.factor, args.steps),
             "general_solve_ms": timed(s.solve, args.steps)}
        ref = s.output.clone()
        t["factor_fused_ms"] = timed(s.factor_fused, args.steps)
        assert int((s.status != 0).sum()) == 0
        t["solve_fused_ms"] = timed(s.solve_fused, args.steps)
        err = float((s.output - ref).abs().max() / ref.abs().max())
        t["fused_factor_solve_ms"] = timed(lambda: s.factor_solve(), args.steps)
        t["general_total_ms"] = t["general_factor_ms"] + t["general_solve_ms"]
        t["split_total_ms"] = t["factor_fused_ms"] + t["solve_fused_ms"]
        t["split_over_general"] = t["split_total_ms"] / t["general_total_ms"]
        lqr.append({"shape": name, "T": args.T, "base_n": args.n, "batch": args.batch,
                    "split_kernel": s.split_kernel_name, "fused_kernel": s.kernel_name, **t,
                    "split_vs_general_max_rel_diff": err})
        print(json.dumps(lqr[-1]), flush=True)
    # sip_kkt_factor + sip_kkt_solve on a tree plan (the binary tree of the family, one constraint row of each kind)
    from oracle.kkt import KKTDims
    import reference_kkt_problems as rk
    from sip_optimal_control_amd import BatchedNewtonKKT
    prob = rp.variable_benchmark_problem(2, args.T, args.n, 2, np.random.default_rng(5))
    N, E = args.T + 1, args.T
    dims = KKTDims(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"],
                   node_c=[1] * N, node_g=[2] * N, edge_c=[1] * E, edge_g=[1] * E)
    model, w, r1, r2, r3, rhs = rk.newton_kkt_problem(dims, seed=3, batch=1, r2_max=1e2)
    B = args.batch
    d = [torch.from_numpy(np.ascontiguousarray(np.repeat(a, B, axis=0))).cuda() for a in (model, w, r1, r2, r3, rhs)]
    kkt_res = {}
    for fused in (False, True):
        kkt = BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                               batch=B, tree_fused=fused)
        sol = torch.zeros(B, kkt.kkt_dim, dtype=torch.float64, device=kkt.device)
        r = {"kernel": kkt.kernel_name, "factor_ms": timed(lambda: kkt.factor(*d[:5]), args.steps)}
        assert int((kkt.status != 0).sum()) == 0
        r["solve_ms"] = timed(lambda: kkt.solve(d[0], d[5], sol=sol), args.steps)
        r["total_ms"] = r["factor_ms"] + r["solve_ms"]
        r["sol"] = sol.clone()
        kkt_res["tree_fused" if fused else "general"] = r
    diff = float((kkt_res["tree_fused"].pop("sol") - kkt_res["general"]["sol"]).abs().max()
                 / kkt_res["general"].pop("sol").abs().max())
    res = {"metric": "tree factor / solve as separate sweeps: split size-class kernels vs the general engine",
           "lqr": lqr, "kkt_tree": {"T": args.T, "batch": B, **kkt_res, "max_rel_diff": diff}}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

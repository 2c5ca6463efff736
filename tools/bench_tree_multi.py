#!/usr/bin/env python3
"""Multi-right-hand-side tree solve (sip_lqr_tree_solve_multi, csrc/tree_mrhs_qw16.hpp) against the column
loop of sip_lqr_tree_solve, on the reference's variable-shape benchmark trees (BM_LQRVariableFactorSolve,
benchmarks/lqr_benchmark.cpp:209-310), and sip_kkt_factor_theta on a tree plan with the multi-rhs path on and
off (SIP_KKT_THETA_TREE_MULTI).

    python tools/bench_tree_multi.py [--batch 4096] [--T 63] [--n 8] [--cols 8] [--kkt-batch 1024] [--out f.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, steps, check=None):
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
    if check is not None:
        check()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--T", type=int, default=63)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kkt-batch", type=int, default=1024)
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
        s.factor()
        rhs = s.pack_rhs([[{k: prob["blocks"][k] for k in ("q", "c", "r")}] for _ in range(args.cols)])
        rhs = rhs.expand(args.cols, args.batch, rhs.shape[2]).contiguous()
        out = torch.zeros(args.cols, args.batch, s.out_len, dtype=torch.float64, device=s.device)

        def ok():
            assert int((s.status != 0).sum()) == 0
        ms_multi = timed(lambda: s.solve_multi(rhs, out_cols=out), args.steps, ok)

        def loop():
            for _ in range(args.cols):
                s.solve()
        ms_loop = timed(loop, args.steps, ok)
        lqr.append({"shape": name, "T": args.T, "base_n": args.n, "batch": args.batch, "cols": args.cols,
                    "multi_kernel": s.multi_kernel_name, "solve_multi_ms": ms_multi,
                    "column_loop_ms": ms_loop, "speedup": ms_loop / ms_multi})
        print(json.dumps(lqr[-1]), flush=True)
    # factor_theta at p = 8 on a branching tree plan, the multi-rhs path on and off
    from oracle.kkt import KKTDims
    import reference_kkt_problems as rk
    from sip_optimal_control_amd import BatchedNewtonKKT
    prob = rp.variable_benchmark_problem(2, 15, args.n, 2, np.random.default_rng(5))
    dims = KKTDims(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"],
                   node_c=[1] * 16, node_g=[2] * 16, edge_c=[1] * 15, edge_g=[1] * 15, theta_dim=8)
    model, w, r1, r2, r3, rhs_k, theta_model = rk.newton_kkt_problem(dims, seed=3, batch=1, r2_max=1e2)
    B = args.kkt_batch
    d = [torch.from_numpy(np.ascontiguousarray(np.repeat(a, B, axis=0))).cuda()
         for a in (model, theta_model, w, r1, r2, r3)]
    theta = {}
    for multi in ("1", "0"):
        os.environ["SIP_KKT_THETA_TREE_MULTI"] = multi
        kkt = BatchedNewtonKKT(dims.parents, dims.children, dims.sd, dims.cd, dims.ncd, dims.ngd, dims.ecd, dims.egd,
                               batch=B, theta_dim=8)
        st = {}

        def run():
            st["s"] = kkt.factor_theta(*d)
        theta[multi] = {"kernel": kkt.kernel_name,
                        "factor_theta_ms": timed(run, args.steps, lambda: None)}
        assert int((st["s"] != 0).sum()) == 0
    res = {"metric": "tree multi-rhs solve (sip_lqr_tree_solve_multi) vs column loop; factor_theta on a tree",
           "lqr": lqr, "factor_theta_p8": {"T": 15, "batch": B, "multi_on": theta["1"], "multi_off": theta["0"]}}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

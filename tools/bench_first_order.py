#!/usr/bin/env python3
"""Time sip_kkt_gather_first_order (f, grad f, c, g from the first-order model outputs) on the f1 chain:
n 12, m 4, c 6, g 8, T = 50, batch 4096 by default.

Prints the milliseconds per call (device events around every timed launch, after a pre-heat) and the achieved
bytes/s over the bytes the call has to move: the first-order arena read once plus the four outputs written once.
The calls rotate over `--buffers` input arenas (4 x 80 MB by default, more than the 256 MB of Infinity Cache
together with the outputs), so that a call does not find its input left in cache by the call before it.

    python tools/bench_first_order.py [--batch 4096] [--T 50] [--launches 20] [--form uniform|tables] [--theta P]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--preheat", type=int, default=10)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--theta", type=int, default=0)
    ap.add_argument("--form", choices=("uniform", "tables"), default="uniform",
                    help="tables: the plan without the chain kernels (SIP_KKT_VARIANT=tables), so the table-driven form")
    ap.add_argument("--f-only", action="store_true", help="new_x = False: f alone")
    args = ap.parse_args()
    if args.form == "tables":
        os.environ["SIP_KKT_VARIANT"] = "tables"
    import torch
    from sip_optimal_control_amd import BatchedNewtonKKT
    if not torch.cuda.is_available():
        sys.exit("bench_first_order.py needs a GPU: a time taken anywhere else says nothing")
    n, m, c, g, T = 12, 4, 6, 8, args.T
    kkt = BatchedNewtonKKT(list(range(T)), list(range(1, T + 1)), [n] * (T + 1), [m] * T, [0] * T + [c],
                           [0] * T + [g], [c] * T, [g] * T, batch=args.batch, theta_dim=args.theta)
    xt = kkt.x_dim + args.theta
    gen = torch.Generator(device="cuda").manual_seed(5)
    firsts = [torch.randn(args.batch, kkt.first_order_len, dtype=torch.float64, device="cuda", generator=gen)
              for _ in range(args.buffers)]
    x = torch.randn(args.batch, xt, dtype=torch.float64, device="cuda", generator=gen)
    init = torch.randn(args.batch, n, dtype=torch.float64, device="cuda", generator=gen)
    f = torch.zeros(args.batch, dtype=torch.float64, device="cuda")
    outs = () if args.f_only else tuple(torch.zeros(args.batch, k, dtype=torch.float64, device="cuda")
                                         for k in (xt, kkt.y_dim, kkt.z_dim))

    def call(k):
        kkt.gather_first_order(firsts[k % args.buffers], x, init, f, *outs, new_x=not args.f_only)

    for k in range(args.preheat):
        call(k)
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
    for k, (start, stop) in enumerate(events):
        start.record()
        call(k)
        stop.record()
    torch.cuda.synchronize()
    ms = sorted(start.elapsed_time(stop) for start, stop in events)
    window_ms = events[0][0].elapsed_time(events[-1][1]) / args.launches
    median = ms[len(ms) // 2]
    # what the call must move: (f only: the f entries alone are needed, but they come a cache line each)
    moved = 8 * args.batch * (kkt.first_order_len + 1 + (0 if args.f_only else xt + kkt.y_dim + kkt.z_dim))
    print(f"{kkt.kernel_name}")
    print(f"form {args.form}, batch {args.batch}, T {T}, theta {args.theta}: first-order arena "
          f"{8 * kkt.first_order_len} B per problem, {moved / 1e6:.1f} MB per call")
    print(f"ms per call: median {median:.4f}  min {ms[0]:.4f}  max {ms[-1]:.4f}  (window / launches {window_ms:.4f})")
    print(f"achieved: {moved / (median * 1e-3) / 1e12:.3f} TB/s at the median, {moved / (ms[0] * 1e-3) / 1e12:.3f} TB/s "
          "at the fastest")
    print(json.dumps({"workload": "gather_first_order", "form": args.form, "batch": args.batch, "T": T,
                      "theta": args.theta, "f_only": args.f_only, "launches": args.launches, "ms_median": median,
                      "ms_min": ms[0], "ms_max": ms[-1], "ms_window": window_ms, "bytes": moved,
                      "tbps_median": moved / (median * 1e-3) / 1e12}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Print which kernel every chain plan gets: per dtype, n <= 33, m <= 9, layout and dispatch environment one line
for a refused plan and four for a created one: as created, with the separate sweeps, with the fused fp32 kernel and
with the fused fp32 kernel and then its separate sweeps asked for.  Needs no GPU (plans are created host-side); SIP_LQR_LIB picks the library.  Two builds
dispatch alike exactly when their outputs are equal:  tools/dispatch_table.py > a.txt ; diff a.txt b.txt"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sip_optimal_control_amd._lib import load_library  # noqa: E402

ENVS = [{}] + [{"SIP_LQR_VARIANT": v} for v in ("direct", "staged", "general", "mf32")]
ENVS += [{"SIP_LQR_EXTRA": "0"}, {"SIP_LQR_EXTRA": "0", "SIP_LQR_PAD": "0"}, {"SIP_LQR_SPLIT": "general"}]
KEYS = ("SIP_LQR_VARIANT", "SIP_LQR_EXTRA", "SIP_LQR_PAD", "SIP_LQR_SPLIT")

lib = load_library()
for env in ENVS:
    for key in KEYS:  # the library reads them at plan creation
        os.environ.pop(key, None)
    os.environ.update(env)
    tag = " ".join(f"{k}={v}" for k, v in env.items()) or "default"
    for dtype, layout, n, m in ((d, l, n, m) for d in (0, 1) for l in (0, 1) for n in range(1, 34) for m in range(1, 10)):
        for optin in ("as created", "sip_lqr_plan_set_separate_sweeps", "sip_lqr_plan_set_fused_f32",
                      "sip_lqr_plan_set_fused_f32 + sip_lqr_plan_set_separate_sweeps"):
            plan = ctypes.c_void_p()  # a fresh plan for each opt-in
            rc = lib.sip_lqr_plan_create_layout(dtype, 5, 7, n, m, 0, layout, ctypes.byref(plan))
            row = [tag, "f32" if dtype else "f64", "sym" if layout else "full", n, m, rc]
            if rc != 0:
                print(*row, sep="\t")
                break
            calls = [c for c in optin.split(" + ") if c.startswith("sip_")]  # in this order, on the one plan
            row += [optin, max([abs(getattr(lib, c)(plan, 1)) for c in calls], default=0)]
            row += [lib.sip_lqr_has_separate_sweeps(plan), lib.sip_lqr_has_fused_f32(plan)]
            row += [lib.sip_lqr_kernel_name(plan).decode(), lib.sip_lqr_workspace_bytes(plan), lib.sip_lqr_has_split(plan),
                    lib.sip_lqr_split_mats_len(plan)]
            row += [lib.sip_lqr_solve_multi_workspace_bytes(plan, cols) for cols in (1, 8, 16, 20)]
            lib.sip_lqr_plan_destroy(plan)
            print(*row, sep="\t")

#!/usr/bin/env python3
"""Print what every Newton-KKT plan comes out as: per environment, dimension set and opt-in sequence one block of
lines after sip_kkt_plan_create and after each opt-in call -- return code, input status, kernel name, the lengths,
the workspace sizes and every model, vector, theta and first-order offset.  Needs a GPU (a plan uploads its tables);
SIP_LQR_LIB picks the library.  Two builds plan alike exactly when their outputs are equal:
tools/kkt_plan_table.py > a.txt ; diff a.txt b.txt"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sip_optimal_control_amd._lib import load_library  # noqa: E402

KEYS = ("SIP_KKT_VARIANT", "SIP_KKT_PIPE", "SIP_KKT_FAMILY", "SIP_KKT_SPLIT", "SIP_KKT_SYM", "SIP_KKT_THETA_FUSED",
        "SIP_KKT_THETA_TREE_MULTI")
ENVS = [{}, {"SIP_KKT_VARIANT": "direct"}, {"SIP_KKT_VARIANT": "tables"}, {"SIP_KKT_PIPE": "0"}, {"SIP_KKT_PIPE": "2"}]
ENVS += [{key: "0"} for key in KEYS[2:]]
BATCH = 3


def chain(n, m, T, cn=0, gn=0, cT=0, gT=0, ce=0, ge=0):
    return dict(root=0, parents=list(range(T)), children=list(range(1, T + 1)), sd=[n] * (T + 1), cd=[m] * T,
                ncd=[cn] * T + [cT], ngd=[gn] * T + [gT], ecd=[ce] * T, egd=[ge] * T)


def family(n, m, T):
    c, g = max(1, n // 2), max(1, 2 * m)
    return chain(n, m, T, 0, 0, c, g, c, g)


def with_(dims, **changed):
    return dict(dims, **changed)


DIM_SETS = [
    ("family (4, 1)", family(4, 1, 3)),
    ("uniform chain, interior constraints", chain(5, 3, 4, 1, 2, 3, 2, 2, 3)),
    ("one-edge chain", chain(3, 2, 1, 1, 0, 2, 1, 1, 2)),
    ("single node", dict(root=0, parents=[], children=[], sd=[3], cd=[], ncd=[2], ngd=[1], ecd=[], egd=[])),
    ("non-uniform chain", dict(root=0, parents=list(range(6)), children=list(range(1, 7)), sd=[4, 6, 5, 3, 6, 4, 5],
                               cd=[2, 3, 1, 2, 3, 2], ncd=[1, 0, 2, 0, 1, 0, 2], ngd=[0, 2, 0, 1, 0, 0, 3],
                               ecd=[1, 2, 0, 1, 1, 0], egd=[2, 0, 1, 1, 0, 2])),
    ("branching tree, root 2", dict(root=2, parents=[2, 0, 2, 0], children=[0, 3, 1, 4], sd=[3, 5, 4, 0, 2],
                                    cd=[2, 0, 3, 1], ncd=[1, 0, 2, 1, 0], ngd=[0, 2, 1, 0, 3], ecd=[1, 0, 2, 1],
                                    egd=[2, 1, 0, 1])),
    ("family (12, 4)", family(12, 4, 5)),
    ("family (12, 3)", family(12, 3, 5)),
    ("chain n = 32, m = 8", family(32, 8, 3)),
    ("chain n = 33", chain(33, 2, 3, 0, 0, 2, 1, 1, 2)),
    ("chain, non-uniform edge constraints", with_(chain(4, 2, 4, 0, 0, 2, 1, 1, 2), ecd=[1, 2, 1, 1])),
    ("negative dimension", with_(chain(4, 2, 3), ncd=[0, -1, 0, 0])),
    ("cyclic edge list", dict(root=0, parents=[0, 1, 2], children=[1, 2, 1], sd=[2, 2, 2, 2], cd=[1, 1, 1],
                              ncd=[0] * 4, ngd=[0] * 4, ecd=[0] * 3, egd=[0] * 3)),
]
TREE_FUSED, SEPARATE, THETA = "sip_kkt_plan_set_tree_fused", "sip_kkt_plan_set_chain_separate_sweeps", "sip_kkt_plan_set_theta"
OPT_INS = [[(TREE_FUSED, 1)], [(SEPARATE, 1)], [(THETA, 1)], [(THETA, 3)], [(THETA, 9)], [(TREE_FUSED, 1), (THETA, 3)],
           [(SEPARATE, 1), (THETA, 3)]]


def ints(values):
    return (ctypes.c_int * max(1, len(values)))(*values)


def describe(lib, plan, d):
    N, E = len(d["sd"]), len(d["cd"])
    yield "status %d name %s" % (lib.sip_kkt_input_status(plan), lib.sip_kkt_kernel_name(plan).decode())
    yield "len x %d y %d z %d model %d" % tuple(lib.sip_kkt_len(plan, which) for which in range(4))
    yield "work %d theta_work %d theta_len %d first_len %d" % (
        lib.sip_kkt_work_bytes(plan), lib.sip_kkt_theta_work_bytes(plan), lib.sip_kkt_theta_len(plan),
        lib.sip_kkt_first_order_len(plan))
    for what, fn, blocks, node_blocks in (("model", lib.sip_kkt_model_offset, 12, (0, 1, 2)),
                                         ("vector", lib.sip_kkt_vector_offset, 7, (0, 2, 3, 5)),
                                         ("theta", lib.sip_kkt_theta_offset, 10, (0, 1, 2, 3)),
                                         ("first", lib.sip_kkt_first_order_offset, 12, (0, 1, 2, 3, 4))):
        for block in range(blocks):
            row = [fn(plan, block, i) for i in range(N if block in node_blocks else E)]
            yield "%s %d: %s" % (what, block, " ".join("%d" % v for v in row))


def main():
    lib = load_library()
    for env in ENVS:
        for key in KEYS:  # the library reads them when a plan is created or given its theta
            os.environ.pop(key, None)
        os.environ.update(env)
        tag = " ".join(f"{k}={v}" for k, v in env.items()) or "default"
        for name, d in DIM_SETS:
            for calls in OPT_INS:
                plan = ctypes.c_void_p()  # a fresh plan for each sequence
                rc = lib.sip_kkt_plan_create(BATCH, len(d["cd"]), d["root"], ints(d["parents"]), ints(d["children"]),
                                             ints(d["sd"]), ints(d["cd"]), ints(d["ncd"]), ints(d["ngd"]),
                                             ints(d["ecd"]), ints(d["egd"]), 0, ctypes.byref(plan))
                head = "%s | %s | " % (tag, name)
                print(head + "sip_kkt_plan_create rc %d" % rc)
                if rc != 0:
                    continue
                done = []
                for line in describe(lib, plan, d):
                    print("  " + line)
                for call, arg in calls:
                    done.append("%s(%d)" % (call, arg))
                    print(head + " + ".join(done) + " rc %d" % getattr(lib, call)(plan, arg))
                    for line in describe(lib, plan, d):
                        print("  " + line)
                lib.sip_kkt_plan_destroy(plan)


if __name__ == "__main__":
    main()

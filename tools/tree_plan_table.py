#!/usr/bin/env python3
"""Print what every tree plan comes out as, through the C ABI only: per environment (default, SIP_LQR_TREE=general,
SIP_LQR_TREE=global) and topology the creation code, the topology status and arrays, the lengths, every
sip_lqr_tree_offset and sip_lqr_tree_rhs_offset, the three kernel names and the scratch sizes; then, on a valid plan,
a plan beyond the size classes and a latched-invalid one, the return code of each of the seven compute entry points
with each pointer argument in turn NULL.  Needs a GPU (a plan uploads its tables); SIP_LQR_LIB picks the library.  Two
builds plan alike exactly when their outputs are equal:  tools/tree_plan_table.py > a.txt ; diff a.txt b.txt

The entry points get real, zero-filled buffers of the plan's sizes and a status array of failures: the few calls that
a NULL does not stop (d_work of sip_lqr_tree_factor_solve on a fused plan, d_scratch on the general engine) factor a
zero problem, which fails with a status, and every solve skips every instance."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sip_optimal_control_amd._lib import load_library  # noqa: E402

ENVS = [None, "general", "global"]
BATCH = 3


def chain(n, m, T):
    return dict(root=0, parents=list(range(T)), children=list(range(1, T + 1)), sd=[n] * (T + 1), cd=[m] * T)


def mixed_tree(nodes, seed):
    """A random tree with random labels, root and dimensions (zero ones among them)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nodes)
    parents = [int(perm[rng.integers(0, k)]) for k in range(1, nodes)]
    children = [int(perm[k]) for k in range(1, nodes)]
    return dict(root=int(perm[0]), parents=parents, children=children,
                sd=[int(v) for v in rng.integers(0, 10, nodes)], cd=[int(v) for v in rng.integers(0, 5, nodes - 1)])


FIVE_NODE = dict(root=0, parents=[0, 0, 1, 1], children=[1, 2, 3, 4], sd=[3, 2, 0, 4, 1], cd=[2, 1, 0, 3])
WIDE_CHAIN = chain(16, 2, 1)
CYCLIC = dict(root=0, parents=[0, 1, 2], children=[1, 2, 1], sd=[2, 2, 2, 2], cd=[1, 1, 1])
TOPOLOGIES = [
    ("single node", dict(root=0, parents=[], children=[], sd=[3], cd=[])),
    ("one-edge chain", dict(root=0, parents=[0], children=[1], sd=[2, 3], cd=[1])),
    ("uniform four-node chain", chain(3, 2, 3)),
    ("five-node tree", FIVE_NODE),
    ("branching tree, root 2", dict(root=2, parents=[2, 0, 2, 0], children=[0, 3, 1, 4], sd=[3, 5, 4, 0, 2],
                                    cd=[2, 0, 3, 1])),
    ("two-node chain, n = 16", WIDE_CHAIN),
    ("chain (3, 2, 2)", chain(3, 2, 2)),
    ("mixed tree of 30 nodes", mixed_tree(30, 7)),
    ("cyclic edge list", CYCLIC),
]
NULL_CHECKS = [("five-node tree", FIVE_NODE), ("two-node chain, n = 16", WIDE_CHAIN), ("cyclic edge list", CYCLIC)]


def ints(values):
    return (ctypes.c_int * max(1, len(values)))(*values)


def create(lib, d):
    plan = ctypes.c_void_p()
    rc = lib.sip_lqr_tree_plan_create(BATCH, len(d["cd"]), d["root"], ints(d["parents"]), ints(d["children"]),
                                      ints(d["sd"]), ints(d["cd"]), 0, ctypes.byref(plan))
    return rc, plan


def row(values):
    return " ".join("%d" % v for v in values)


def describe(lib, plan, d):
    N, E = len(d["sd"]), len(d["cd"])
    status = lib.sip_lqr_tree_topology_status(plan)
    yield "topology status %d" % status
    if status == 0:
        for which, count in enumerate((N + 1, E, N, N)):
            array = lib.sip_lqr_tree_topology_array(plan, which)
            yield "topology array %d: %s" % (which, row(array[i] for i in range(count)))
    yield "len input %d work %d output %d rhs %d" % (lib.sip_lqr_tree_input_len(plan), lib.sip_lqr_tree_work_len(plan),
                                                     lib.sip_lqr_tree_output_len(plan), lib.sip_lqr_tree_rhs_len(plan))
    for arena in range(3):
        for kind, count in enumerate((N, E)):
            yield "offset %d %d: %s" % (arena, kind, row(lib.sip_lqr_tree_offset(plan, arena, kind, i)
                                                         for i in range(count)))
    for kind, count in enumerate((N, E)):
        yield "rhs offset %d: %s" % (kind, row(lib.sip_lqr_tree_rhs_offset(plan, kind, i) for i in range(count)))
    yield "kernel %s | split %s | multi %s" % (lib.sip_lqr_tree_kernel_name(plan).decode(),
                                               lib.sip_lqr_tree_split_kernel_name(plan).decode(),
                                               lib.sip_lqr_tree_multi_kernel_name(plan).decode())
    yield "fused scratch %d multi scratch %s" % (lib.sip_lqr_tree_fused_scratch_bytes(plan), row(
        lib.sip_lqr_tree_solve_multi_scratch_bytes(plan, cols) for cols in (1, 3, 9)))


def null_checks(lib, plan):
    """Return codes of the compute entry points, each pointer argument in turn NULL (and none)."""
    def doubles(count):
        return torch.zeros(max(32, BATCH * count), dtype=torch.float64, device="cuda:0")

    def scratch(nbytes):
        return torch.zeros(max(256, nbytes), dtype=torch.uint8, device="cuda:0")

    out_len = lib.sip_lqr_tree_output_len(plan)
    buffers = dict(input=doubles(lib.sip_lqr_tree_input_len(plan)), work=doubles(lib.sip_lqr_tree_work_len(plan)),
                   output=doubles(out_len), rhs=doubles(out_len), out_cols=doubles(out_len),
                   status=torch.ones(BATCH, dtype=torch.int32, device="cuda:0"),
                   scratch=scratch(lib.sip_lqr_tree_fused_scratch_bytes(plan)),
                   cols=scratch(lib.sip_lqr_tree_solve_multi_scratch_bytes(plan, 1)))
    entry_points = [
        ("sip_lqr_tree_factor", ("input", "work", "status")),
        ("sip_lqr_tree_solve", ("input", "work", "output", "status")),
        ("sip_lqr_tree_solve_multi", ("input", "work", "rhs", "out_cols", 1, "status", "cols")),
        ("sip_lqr_tree_factor_solve", ("input", "work", "output", "status", "scratch")),
        ("sip_lqr_tree_factor_solve_workspace", ("input", "work", "output", "status", "scratch")),
        ("sip_lqr_tree_factor_fused", ("input", "work", "status", "scratch")),
        ("sip_lqr_tree_solve_fused", ("input", "work", "output", "status", "scratch")),
    ]
    for name, args in entry_points:
        pointers = [a for a in args if isinstance(a, str)]
        codes = []
        for null in ["plan", None] + pointers:
            buffers["status"].fill_(1)  # nothing factored: every solve skips every instance
            argv = [a if not isinstance(a, str) else None if a == null else buffers[a].data_ptr() for a in args]
            codes.append("%s %d" % (null or "none", getattr(lib, name)(None if null == "plan" else plan, *argv, None)))
            torch.cuda.synchronize()
        yield "%s NULL: %s" % (name, " | ".join(codes))


def main():
    lib = load_library()
    for env in ENVS:
        os.environ.pop("SIP_LQR_TREE", None)  # the library reads it when a plan is created (and at a launch: global)
        if env is not None:
            os.environ["SIP_LQR_TREE"] = env
        tag = "SIP_LQR_TREE=%s" % env if env else "default"
        for name, d in TOPOLOGIES:
            rc, plan = create(lib, d)
            print("%s | %s | sip_lqr_tree_plan_create rc %d" % (tag, name, rc))
            if rc != 0:
                continue
            for line in describe(lib, plan, d):
                print("  " + line)
            lib.sip_lqr_tree_plan_destroy(plan)
        for name, d in NULL_CHECKS:
            rc, plan = create(lib, d)
            print("%s | %s | NULL arguments, rc %d" % (tag, name, rc))
            for line in null_checks(lib, plan):
                print("  " + line)
            lib.sip_lqr_tree_plan_destroy(plan)


if __name__ == "__main__":
    main()

"""What a tree plan decides on the host: the offset tables of the general engine's plan (csrc/generic_plan.hpp) and
the size class, flattened traversal and scratch partition of the fused tree kernels (csrc/tree_plan.hpp).
tests/cpp/test_tree_plan.cpp prints all of it for a fixed list of small cases, on the host.  Held here against
statements written independently of the C++: the offsets against a walk of the arena order include/sip_lqr_amd.h
documents ("Arenas", "Packed chain layout"), the records against the rule in the header comments of
csrc/tree_qw16.hpp and csrc/tree_schedule.hpp, over the traversal arrays of the oracle."""
import subprocess

import numpy as np
import pytest

BATCH = 3                 # of the printed scratch partition
TS_LOAD_V, TS_CHILD_LIVE = 1, 2
# fused size classes, sorted by cost: the first that holds the largest state and control dimension serves the tree
CLASSES = [(4, 2), (6, 3), (8, 4), (9, 3), (10, 4), (12, 4), (15, 4), (15, 8)]


def _chain(n, m, T):
    return dict(root=0, parents=list(range(T)), children=list(range(1, T + 1)), sd=[n] * (T + 1), cd=[m] * T)


CASES = [
    ("single node", dict(root=0, parents=[], children=[], sd=[3], cd=[])),
    ("one-edge chain", dict(root=0, parents=[0], children=[1], sd=[2, 3], cd=[1])),
    ("uniform four-node chain", _chain(3, 2, 3)),
    ("five-node tree", dict(root=0, parents=[0, 0, 1, 1], children=[1, 2, 3, 4], sd=[3, 2, 0, 4, 1], cd=[2, 1, 0, 3])),
    ("branching tree, root 2", dict(root=2, parents=[2, 0, 2, 0], children=[0, 3, 1, 4], sd=[3, 5, 4, 0, 2],
                                    cd=[2, 0, 3, 1])),
    ("two-node chain, n = 16", _chain(16, 2, 1)),
]
CHAIN_LAYOUT = (3, 2, 2)  # (n, m, T) of the packed chain layout


class _Walk:
    """Hands out consecutive blocks of one arena."""

    def __init__(self):
        self.at = 0

    def take(self, size):
        at, self.at = self.at, self.at + size
        return at


def _node_work_and_scratch(tab, work, sd, max_n, max_m):
    """The end of every work arena: node blocks V (n*n) | F_factor (n*n) | sqrt_delta (n) | sqrt_delta_inv (n) |
    v (n), then the scratch H (max_m x max_n) | F (max_n^2) | g (max_n) | h (max_m) | f (max_n)
    (csrc/tree_generic.hpp, struct Meta)."""
    for n in sd:
        for name, size in (("oV", n * n), ("oF", n * n), ("osd", n), ("osdi", n), ("ov", n)):
            tab[name].append(work.take(size))
    scratch_ws = work.at
    work.take(max_m * max_n + max_n * max_n + max_n + max_m + max_n)
    return scratch_ws


def _tree_native_walk(d):
    """include/sip_lqr_amd.h, "Arenas":
    input  : node blocks Q (n*n) | q (n) | c (n) | delta (n);
             edge blocks A (nc*np) | B (nc*m) | M (np*m) | R (m*m) | r (m)
    work   : edge blocks W (max_n^2) | K (m*np) | G_factor (m*m) | k (m); node blocks ...; scratch
    output : node blocks x (n) | y (n); edge blocks u (m)"""
    sd, cd = d["sd"], d["cd"]
    max_n, max_m = max(sd), max(cd, default=0)
    tab = {name: [] for name in FIELDS}
    inp, work, out = _Walk(), _Walk(), _Walk()
    for n in sd:
        for name, size in (("oQ", n * n), ("oq", n), ("oc", n), ("od", n)):
            tab[name].append(inp.take(size))
        tab["ox"].append(out.take(n))
        tab["oy"].append(out.take(n))
    for e, m in enumerate(cd):
        n_p, n_c = sd[d["parents"][e]], sd[d["children"][e]]
        for name, size in (("oA", n_c * n_p), ("oB", n_c * m), ("oM", n_p * m), ("oR", m * m), ("orr", m)):
            tab[name].append(inp.take(size))
        tab["ou"].append(out.take(m))
    for e, m in enumerate(cd):
        n_p = sd[d["parents"][e]]
        for name, size in (("oW", max_n * max_n), ("oK", m * n_p), ("oG", m * m), ("ok", m)):
            tab[name].append(work.take(size))
    scratch_ws = _node_work_and_scratch(tab, work, sd, max_n, max_m)
    # one input arena (in1 is in0); the gains live in the work arena; a column of the general engine's multi-rhs
    # solve: the output layout, then g | h | f
    lens = dict(in0=inp.at, in1=inp.at, out=out.at, gain=work.at, ws=work.at, scratch_ws=scratch_ws,
                cols=out.at + 2 * max_n + max_m)
    return tab, lens


def _chain_walk(n, m, T):
    """include/sip_lqr_amd.h, "Packed chain layout": stages i = 0..T one after the other;
    mats : Q (n*n) | delta (n), and if i < T: A (n*n) | B (n*m) | M (n*m) | R (m*m)
    vecs : q (n) | c (n), if i < T: r (m);  sol: x | y, u likewise;  gains: K (m*n) | k (m) for i < T
    work (csrc/tree_generic.hpp): edge blocks W (n^2) | G_factor (m*m); node blocks ...; scratch"""
    tab = {name: [] for name in FIELDS}
    mats, vecs, gains, work = _Walk(), _Walk(), _Walk(), _Walk()
    for i in range(T + 1):
        tab["oQ"].append(mats.take(n * n))
        tab["od"].append(mats.take(n))
        for name in (("oq", "ox"), ("oc", "oy")):   # sol has the layout of vecs
            at = vecs.take(n)
            tab[name[0]].append(at)
            tab[name[1]].append(at)
        if i < T:
            for name, size in (("oA", n * n), ("oB", n * m), ("oM", n * m), ("oR", m * m)):
                tab[name].append(mats.take(size))
            at = vecs.take(m)
            tab["orr"].append(at)
            tab["ou"].append(at)
            tab["oK"].append(gains.take(m * n))
            tab["ok"].append(gains.take(m))
    for _ in range(T):
        tab["oW"].append(work.take(n * n))
        tab["oG"].append(work.take(m * m))
    scratch_ws = _node_work_and_scratch(tab, work, [n] * (T + 1), n, m)
    lens = dict(in0=mats.at, in1=vecs.at, out=vecs.at, gain=gains.at, ws=work.at, scratch_ws=scratch_ws,
                cols=vecs.at + 2 * n + m)
    return tab, lens


PER_EDGE = ("oA", "oB", "oM", "oR", "orr", "ou", "oK", "ok", "oW", "oG")
FIELDS = ("oQ", "od", "oA", "oB", "oM", "oR", "oq", "oc", "orr", "ox", "oy", "ou", "oK", "ok", "oW", "oG", "oV", "oF",
          "osd", "osdi", "ov")


def _steps(d, tab, topo):
    """The rule of csrc/tree_qw16.hpp / tree_schedule.hpp.  Backward: per node in postorder one EDGE step per child
    edge in CSR order, then the NODE step; TS_LOAD_V on the first edge step, or on the node step of a leaf;
    TS_CHILD_LIVE exactly when the child is the node the previous step finished.  Forward: one step per edge, parents
    in preorder, live when the parent's x is what the previous step produced (the root's comes first)."""
    sd, cd, children = d["sd"], d["cd"], d["children"]
    offsets, edges = topo["child_offsets"], topo["child_edges"]

    def record(sweep, kind, node, edge, flags, work_of, v_of):
        r = dict(sweep=sweep, kind=kind, node=node, n=sd[node], flags=flags,
                 oQ=tab["oQ"][node], oq=tab["oq"][node], oc=tab["oc"][node], od=tab["od"][node],
                 oV=tab["oV"][work_of], oF=tab["oF"][work_of], osd=tab["osd"][work_of], osdi=tab["osdi"][work_of],
                 ov=tab["ov"][v_of], oxp=tab["ox"][node])  # x of `node`: the parent in edge steps
        edge_keys = ("oA", "oB", "oM", "oR", "orr", "oK", "ok", "oW", "oG", "ou")
        if edge is None:  # a node step: nothing of an edge or a child
            r.update(dict.fromkeys(edge_keys + ("edge", "child", "nc", "m", "odc", "oxc", "oyc"), 0))
        else:
            ch = children[edge]
            r.update({key: tab[key][edge] for key in edge_keys})
            r.update(edge=edge, child=ch, nc=sd[ch], m=cd[edge], odc=tab["od"][ch], oxc=tab["ox"][ch],
                     oyc=tab["oy"][ch])
        return r

    steps, finished = [], None
    for node in topo["postorder_nodes"]:
        mine = edges[offsets[node]:offsets[node + 1]]
        for k, e in enumerate(mine):
            flags = (TS_LOAD_V if k == 0 else 0) | (TS_CHILD_LIVE if children[e] == finished else 0)
            # the work fields of the parent, but v of the child
            steps.append(record("backward", 0, node, e, flags, node, children[e]))
            finished = None
        steps.append(record("backward", 1, node, None, 0 if mine else TS_LOAD_V, node, node))
        finished = node
    produced = d["root"]
    for node in topo["preorder_nodes"]:
        for e in edges[offsets[node]:offsets[node + 1]]:
            ch = children[e]
            # every work field of the child
            steps.append(record("forward", 0, node, e, TS_CHILD_LIVE if node == produced else 0, ch, ch))
            produced = ch
    return steps


def _parse(text):
    cases = []
    for line in text.splitlines():
        word = line.split()
        if word[0] == "case":
            cases.append(dict(header=line, ints={}, tab={}, kind={}, steps=[]))
            continue
        cur = cases[-1]
        if word[0] == "ints":
            cur["ints"][word[1]] = [int(v) for v in word[2:]]
        elif word[0] == "tab":
            cur["tab"][word[1]] = [int(v) for v in word[3:]]
            cur["kind"][word[1]] = word[2]
        elif word[0] == "len":
            cur["len"] = {k: int(v) for k, v in zip(word[1::2], word[2::2])}
        elif word[0] == "class":
            cur["class"] = None if word[1] == "none" else dict(
                n=int(word[1]), m=int(word[2]), **{k: int(v) for k, v in zip(word[3:11:2], word[4:11:2])},
                name=" ".join(word[12:]))
        elif word[0] == "step":
            cur["steps"].append(dict(sweep=word[1], **{k: int(v) for k, v in zip(word[2::2], word[3::2])}))
        else:
            assert word[0] == "sched", line
            cur["sched"] = {k: int(v) for k, v in zip(word[1::2], word[2::2])}
    return cases


@pytest.fixture(scope="module")
def printed():
    import __graft_entry__ as entry
    entry.build_hip()
    exe = entry.build_tree_plan_test()
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, (proc.stdout[-3000:], proc.stderr[-3000:])
    cases = _parse(proc.stdout)
    assert len(cases) == len(CASES) + 1
    return cases


def _check_layout(got, tab, lens, header):
    assert tuple(got["tab"]) == FIELDS, header
    assert got["kind"] == {name: "edge" if name in PER_EDGE else "node" for name in FIELDS}, header
    assert got["tab"] == tab, header
    assert got["len"] == lens, header


@pytest.mark.parametrize("k", range(len(CASES)), ids=[name for name, _ in CASES])
def test_tree_plan(printed, oracle_lib, k):
    name, d = CASES[k]
    got = printed[k]
    N, E = len(d["sd"]), len(d["cd"])
    assert got["header"] == f"case {name} | tree-native | root {d['root']} | topology 0"
    blocks = {key: [np.zeros((1, 1))] * (N if key == "Q" else E) for key in ("Q", "M", "R", "A", "B")}
    blocks.update({key: [np.zeros(1)] * N for key in ("q", "c", "delta")})
    blocks["r"] = [np.zeros(1)] * E
    lqr = oracle_lib.TreeLQR(d["parents"], d["children"], [1] * N, [1] * E, blocks, root=d["root"])
    assert lqr.topology_status == 0
    topo = lqr.topology_arrays()
    assert got["ints"] == dict(parents=d["parents"], children=d["children"], sd=d["sd"], cd=d["cd"],
                               child_offsets=topo["child_offsets"], child_edges=topo["child_edges"],
                               preorder=topo["preorder_nodes"], postorder=topo["postorder_nodes"]), name
    # offsets and lengths
    tab, lens = _tree_native_walk(d)
    _check_layout(got, tab, lens, name)
    # size class and scratch: padded gains K (M x N) | k (M) per edge at 0, then the spill S (N x N) | g | h | t | v
    # per node, each part rounded up to 256 bytes (csrc/tree_qw16.hpp)
    fits = [(n, m) for n, m in CLASSES if n >= max(1, max(d["sd"])) and m >= max(1, max(d["cd"], default=0))]
    if not fits:
        assert got["class"] is None, name
    else:
        n, m = fits[0]
        up = lambda v: (v + 255) // 256 * 256  # noqa: E731
        at_spill = up(BATCH * 8 * E * (m * n + m))
        assert got["class"] == dict(n=n, m=m, gain=m * n + m, spill=n * n + 4 * n, at_spill=at_spill,
                                    bytes=up(at_spill + BATCH * 8 * N * (n * n + 4 * n)),
                                    name=f"tree_factor_solve_qw16<{n},{m}>/f64"), name
    # records and the scalars of the schedule
    want = _steps(d, tab, topo)
    assert len(got["steps"]) == len(want) == N + 2 * E, name
    for i, (g, w) in enumerate(zip(got["steps"], want)):
        assert g == w, (name, i)
    root = d["root"]
    assert got["sched"] == dict(n_backward=N + E, n_forward=E, Nn=N, E=E, root=root, root_n=d["sd"][root],
                                root_od=tab["od"][root], root_ox=tab["ox"][root], root_oy=tab["oy"][root],
                                in_len=lens["in0"], out_len=lens["out"], ws_len=lens["ws"]), name


def test_cases_reach_every_rule(printed):
    """The cases are the smallest at which each rule can go wrong: they must really have those steps."""
    by_name = {name: got for (name, _), got in zip(CASES, printed)}
    chain = by_name["uniform four-node chain"]["steps"]
    assert all(s["flags"] & TS_CHILD_LIVE for s in chain if s["kind"] == 0)           # every first child is live
    tree = [s for s in by_name["five-node tree"]["steps"] if s["sweep"] == "backward" and s["kind"] == 0]
    assert [s["flags"] for s in tree] == [TS_LOAD_V | TS_CHILD_LIVE, 0] * 2         # second children: not live
    assert by_name["two-node chain, n = 16"]["class"] is None
    assert by_name["single node"]["class"]["n"] == 4


def test_every_size_class_is_in_the_multi_column_gpu_test():
    """The TREE_CLASS(N, M) list of csrc/tree_qw16.hip, read from the source, is the list this file states and the
    list tests/test_gpu_tree_multi.py runs with more than one column: a new class cannot arrive untested.  Each
    enumerated case lands in its own class and not in a cheaper one."""
    import os
    import re
    import test_gpu_tree_multi as multi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "sip_optimal_control_amd", "csrc", "tree_qw16.hip")) as f:
        text = f.read()
    (table,) = re.findall(r"kClasses\[\]\s*=\s*\{(.*?)\};", text, flags=re.S)
    in_source = [(int(n), int(m)) for n, m in re.findall(r"TREE_CLASS\(\s*(\d+)\s*,\s*(\d+)\s*\)", table)]
    assert len(in_source) == len(set(in_source)) and in_source == CLASSES
    assert [(n, m) for n, m, _ in multi.CLASSES] == in_source
    for max_n, max_m, tag in multi.CLASSES:
        first = [(n, m) for n, m in in_source if n >= max_n and m >= max_m][0]
        assert tag == "<%d,%d>" % first == "<%d,%d>" % (max_n, max_m)


def test_chain_layout(printed):
    n, m, T = CHAIN_LAYOUT
    got = printed[-1]
    assert got["header"] == f"case chain ({n}, {m}, {T}) | packed chain | root 0 | topology 0"
    tab, lens = _chain_walk(n, m, T)
    _check_layout(got, tab, lens, got["header"])

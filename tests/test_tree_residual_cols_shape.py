"""The launch shape of the multi-column tree residual (csrc/tree_residual_cols_shape.hpp), without a GPU: the host
program tests/cpp/test_tree_residual_cols_shape.cpp prints columns, wavefronts, staged, split and LDS bytes for a fixed
list of topologies, and every line is recomputed here from the rules the header states:

  never more than 64 KiB of dynamic LDS; staged needs `input` 16-byte aligned and the largest item's image plus the NC
  vector sets of one wavefront to fit; staged with fewer columns before unstaged with more; the widest instantiation
  tried is the least of 1, 2, 4, 8 that holds the request; split is wanted where max_children * 4 > N + E and taken at a
  column count only where the parts and two wavefronts fit; with the preference set, the largest column count at which
  split can be taken wins, without it the largest count that fits with nodes in turn, split only if it can be taken
  there; columns first, wavefronts second; no more wavefronts than items."""
import subprocess

import numpy as np
import pytest

BUDGET = 65536
NAMES = ("nonuniform_delta_chain", "branch", "variable_branch", "five_node", "single_node", "random<9,3>", "random<15,8>",
         "star_of_12", "star_of_63", "parts_beyond_lds", "n91_pair", "empty_nodes", "n500_pair")


def _z_bytes(max_n, max_m, nc):
    return max(2, (nc * (9 * max_n + 2 * max_m) + max_n + 1) // 2 * 2) * 8


def _image_bytes(scalars):
    return (scalars * 8 + 16 + 15) // 16 * 16


def _parts_bytes(r, nc):
    return (r["nodes"] + r["edges"]) * 2 * r["max_n"] * nc * 8


def _at(r, nc, staged, split, max_waves=4):
    """(columns, waves, staged, split, lds), or None where it does not fit."""
    wave = _z_bytes(r["max_n"], r["max_m"], nc) + (_image_bytes(r["image"]) if staged else 0)
    fixed = nc * 8 * max_waves + (_parts_bytes(r, nc) if split else 0)
    if fixed + (2 if split else 1) * wave > BUDGET:
        return None
    items = r["nodes"] + r["edges"] if split else max(1, r["nodes"])
    waves = min((BUDGET - fixed) // wave, max_waves, items)
    if split and waves < 2:
        return None
    return nc, waves, staged, split, fixed + waves * wave


def _counts(requested, max_columns=8):
    top = 1
    while top < requested and top < max_columns:
        top *= 2
    out = []
    while top >= 1:
        out.append(top)
        top //= 2
    return out


def _expected(r):
    want_split = r["max_children"] * 4 > r["nodes"] + r["edges"]
    for staged in ((True, False) if r["aligned"] else (False,)):
        if want_split and r["prefer"]:
            for nc in _counts(r["requested"]):
                s = _at(r, nc, staged, True)
                if s:
                    return s
        for nc in _counts(r["requested"]):
            s = _at(r, nc, staged, False)
            if s:
                return (want_split and _at(r, nc, staged, True)) or s
    return 0, 0, False, False, 0


@pytest.fixture(scope="module")
def lines():
    import __graft_entry__ as entry
    exe = entry.build_tree_residual_cols_shape_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    head = dict(zip(out[0].split()[::2], map(int, out[0].split()[1::2])))
    rows = []
    for line in out[1:]:
        left, right = line.split(" -> ")
        name, left = left.split(" ", 1)
        r = dict(zip(left.split()[::2], map(int, left.split()[1::2])))
        r["name"] = name
        rows.append((r, dict(zip(right.split()[::2], map(int, right.split()[1::2])))))
    return head, rows


def _full(rows, name, aligned=1, prefer=1):
    return next(got for r, got in rows
                if r["name"] == name and r["requested"] == 8 and r["aligned"] == aligned and r["prefer"] == prefer)


def _dims(rows, name):
    r = next(r for r, _ in rows if r["name"] == name)
    return {k: r[k] for k in ("nodes", "edges", "max_n", "max_m", "max_children", "image")}


def _dims_of(parents, children, sd, cd):
    image = max([n * n for n in sd] + [sd[c] * sd[p] + sd[c] * m + sd[p] * m + m * m
                                       for p, c, m in zip(parents, children, cd)])
    return {"nodes": len(sd), "edges": len(cd), "max_n": max(sd), "max_m": max(cd, default=0),
            "max_children": int(max(np.bincount(parents), default=0)) if len(parents) else 0, "image": image}


def test_the_list_of_topologies_is_the_one_the_test_expects(lines):
    import full_batch_problems as fb
    import hard_inputs as hi
    import tree_refine_cases as tc
    head, rows = lines
    assert head == {"budget": BUDGET, "max_columns": 8, "max_waves": 4, "prefer_split": head["prefer_split"]}
    assert head["prefer_split"] in (0, 1)
    assert tuple(dict.fromkeys(r["name"] for r, _ in rows)) == NAMES
    for name in NAMES:                                       # aligned and not, both preferences, short groups
        mine = [r for r, _ in rows if r["name"] == name]
        assert {(r["aligned"], r["prefer"]) for r in mine if r["requested"] == 8} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {r["requested"] for r in mine} == {1, 2, 3, 5, 8}
    # the program's topologies are the ones the GPU tests and the benchmark run
    for name, prob in tc.reference_trees().items():
        assert _dims(rows, name) == _dims_of(prob["parents"], prob["children"], prob["state_dims"], prob["control_dims"])
    for dims in hi.TREES:
        topo = fb.random_topology(np.random.default_rng(hi._seed("tree", *dims)), hi.TREE_NODES, *dims)
        assert _dims(rows, "random<%d,%d>" % dims) == _dims_of(topo.parents, topo.children, topo.sd, topo.cd)
    topo = fb.variable_benchmark_topology(1)
    assert _dims(rows, "star_of_63") == _dims_of(topo.parents, topo.children, topo.sd, topo.cd)
    assert _dims(rows, "star_of_12") == _dims_of([0] * 12, list(range(1, 13)), [6, 3, 4, 5] * 3 + [2], [2, 1, 3] * 4)
    assert _dims(rows, "n91_pair") == _dims_of([0], [1], [91, 2], [1])
    wide = _dims(rows, "parts_beyond_lds")
    assert wide["nodes"] == 300 and wide["max_n"] == 15 and wide["max_children"] * 4 > 599
    assert 599 * 2 * 15 * 8 > BUDGET                        # its parts exceed LDS at one column already


def test_every_line_is_what_the_rules_give(lines):
    _, rows = lines
    for r, got in rows:
        want = _expected(r)
        assert (got["columns"], got["waves"], bool(got["staged"]), bool(got["split"]), got["lds"]) == want, (r, got, want)


def test_the_bounds_hold_everywhere(lines):
    _, rows = lines
    for r, got in rows:
        assert got["lds"] <= BUDGET, (r, got)
        assert got["columns"] in (1, 2, 4, 8), (r, got)
        items = r["nodes"] + r["edges"] if got["split"] else max(1, r["nodes"])
        assert 1 <= got["waves"] <= 4 and got["waves"] <= items, (r, got)
        # a short group is never launched on an instantiation twice as wide as it needs
        assert got["columns"] < 2 * r["requested"], (r, got)
        # what the kernel is told fits what it lays out: red + waves * (vectors [+ image]) [+ parts]
        wave = _z_bytes(r["max_n"], r["max_m"], got["columns"]) + (_image_bytes(r["image"]) if got["staged"] else 0)
        lds = got["columns"] * 32 + got["waves"] * wave + (_parts_bytes(r, got["columns"]) if got["split"] else 0)
        assert got["lds"] == lds, (r, got)
        assert not (got["staged"] and not r["aligned"]), (r, got)
        assert not got["split"] or (r["max_children"] * 4 > r["nodes"] + r["edges"] and got["waves"] >= 2), (r, got)


def test_the_cases_the_design_names(lines):
    head, rows = lines
    for name, lds in (("random<9,3>", 27 * 1024), ("random<15,8>", 56 * 1024)):
        got = _full(rows, name)
        assert (got["columns"], got["waves"], got["staged"], got["split"]) == (8, 4, 1, 0), (name, got)
        assert 0.9 * lds <= got["lds"] <= lds, (name, got)   # about 27 KB and 56 KB
    got = _full(rows, "star_of_12")                          # split with 8 columns: its parts are 19 200 bytes
    assert (got["columns"], got["staged"], got["split"]) == (8, 1, 1) and 25 * 2 * 6 * 8 * 8 == 19200
    # the 63-child star at max_n = 9: the parts are 146 304 bytes at 8 columns and fit at 2 (36 576): the knob decides
    r63 = _dims(rows, "star_of_63")
    assert _parts_bytes(r63, 8) == 146304 and _parts_bytes(r63, 2) == 36576 and r63["max_n"] == 9
    split, turn = _full(rows, "star_of_63", prefer=1), _full(rows, "star_of_63", prefer=0)
    assert head["prefer_split"] == 1                         # the library's default: the faster of the two, as measured
    assert (split["columns"], split["split"], split["staged"]) == (2, 1, 1), split
    assert (turn["columns"], turn["split"], turn["staged"]) == (8, 0, 1), turn
    for prefer in (0, 1):
        for aligned in (0, 1):
            assert not _full(rows, "parts_beyond_lds", aligned, prefer)["split"]            # never split
            assert not _full(rows, "n91_pair", aligned, prefer)["staged"]                    # direct
        assert not _full(rows, "random<9,3>", 0, prefer)["staged"]                           # a misaligned input
    # the n = 91 pair: the columns cut to what one wavefront's vectors allow (8 columns are 53 KB, one wavefront)
    got = _full(rows, "n91_pair", prefer=0)
    assert (got["columns"], got["waves"]) == (8, 1) and _z_bytes(91, 1, 8) + 256 <= BUDGET < 2 * _z_bytes(91, 1, 8)
    got = _full(rows, "n500_pair")
    assert got["columns"] == 1 and _z_bytes(500, 1, 2) + 64 > BUDGET

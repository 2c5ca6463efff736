"""The host table and launch shape of the tree gradient kernel (csrc/tree_vjp_table.hpp), printed by
tests/cpp/test_tree_vjp_table.cpp for a fixed list of topologies.  No GPU.

Every input-arena index has exactly one word, ia and ib lie in [0, output_len), and the form is the one of its block
(the blocks located by the oracle's statement of the layout, not by the plan's).  The gradient evaluated through the
printed table in float64 numpy equals tests/tree_vjp_cases.py in float64 bit for bit: both compute
s * (l[ia] z[ib] + z[ia] l[ib]) with the same three roundings, and the factors 1, 1/2, -1/2 are exact (delta, which
tree_vjp_cases states as -ly y, is -1/2 (p + p) = -p here).  So the table is the mathematics, which
tests/test_tree_vjp_model.py holds against finite differences.  The launch shape is recomputed from the rules the header
states."""
import os
import subprocess

import numpy as np
import pytest

import full_batch_problems as fb
import tree_vjp_cases as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, HALF, MINUS_HALF, COPY = 0, 1, 2, 3
FACTOR = np.array([1.0, 0.5, -0.5, 0.0])
EXPECTED = ["nonuniform_delta_chain", "branch", "variable_branch", "five_node", "single_node", "node_n0", "edge_m0",
            "star_of_12", "chain_30x70"]


@pytest.fixture(scope="module")
def printed():
    import __graft_entry__ as entry
    exe = entry.build_tree_vjp_table_test()
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    lines = run.stdout.splitlines()
    consts = dict(zip(lines[0].split()[0::2], (int(v) for v in lines[0].split()[1::2])))
    trees, cur = {}, None
    for line in lines[1:]:
        f = line.split()
        if f[0] == "tree":
            cur = {"name": f[1], "N": int(f[3]), "E": int(f[5]), "in_len": int(f[7]), "out_len": int(f[9]),
                   "shapes": [], "words": []}
        elif f[0] == "list":
            cur[f[1]] = [int(v) for v in f[2:]]
        elif f[0] == "shape":
            cur["shapes"].append({"batch": int(f[2]), "ask_waves": int(f[4]), "ask_run": int(f[6]), "name": f[8],
                                  "staged": int(f[10]), "waves": int(f[12]), "run": int(f[14]), "runs": int(f[16]),
                                  "lds": int(f[18])})
        elif f[0] == "w":
            cur["words"].append((int(f[1]), int(f[2]), int(f[3])))
        elif f[0] == "end":
            cur["words"] = np.array(cur["words"], dtype=np.int64).reshape(-1, 3)
            trees[cur["name"]] = cur
    return consts, trees


def _topo(t):
    return fb.Topology(t["parents"], t["children"], t["state_dims"], t["control_dims"], name=t["name"])


def _expected_codes(topo):
    """The code of every input-arena index, from the oracle's statement of the layout ([nodes | edges])."""
    codes = []
    for n in topo.sd:
        codes += [HALF] * (n * n) + [COPY] * (2 * n) + [MINUS_HALF] * n
    for e in range(topo.E):
        np_, nc, m = topo.edge_dims(e)
        codes += [ONE] * (nc * np_ + nc * m + np_ * m) + [HALF] * (m * m) + [COPY] * m
    return np.array(codes, dtype=np.int64)


def test_the_fixed_list(printed):
    consts, trees = printed
    assert list(trees) == EXPECTED
    assert consts == {"budget": 65536, "lanes": 64, "max_waves": 8, "compute_units": 256, "min_run": 4096,
                      "max_runs": 65535}
    chain = trees["chain_30x70"]
    assert chain["state_dims"] == [30] * 70 and chain["control_dims"] == [4] * 69 and 16 * chain["out_len"] > 65536
    assert 0 in trees["node_n0"]["state_dims"] and 0 in trees["edge_m0"]["control_dims"]
    assert trees["single_node"]["E"] == 0 and len(trees["star_of_12"]["parents"]) == 12


@pytest.mark.parametrize("name", EXPECTED)
def test_every_index_has_one_word_of_the_right_form(printed, name):
    t = printed[1][name]
    topo = _topo(t)
    assert t["in_len"] == tv.input_len(topo) and t["out_len"] == topo.layout.sol_len
    words = t["words"]
    assert words.shape == (t["in_len"], 3)                                    # one word per index, in the arena's order
    ia, ib, code = words.T
    assert ((0 <= ia) & (ia < t["out_len"]) & (0 <= ib) & (ib < t["out_len"])).all()
    assert np.array_equal(code, _expected_codes(topo))
    same = (code == COPY) | (code == MINUS_HALF)
    assert (ia[same] == ib[same]).all()                                       # a copy and delta read one place


@pytest.mark.parametrize("name", EXPECTED)
def test_the_table_is_the_mathematics(printed, name):
    t = printed[1][name]
    topo = _topo(t)
    rng = np.random.default_rng(len(name) + t["in_len"])
    z, lam = rng.normal(size=(2, t["out_len"])), rng.normal(size=(2, t["out_len"]))
    ia, ib, code = t["words"].T
    pair = FACTOR[code] * (lam[:, ia] * z[:, ib] + z[:, ia] * lam[:, ib])
    through_table = np.where(code == COPY, lam[:, ia], pair)
    ref, _, copy = tv.grad_input(topo, z, lam, dt=np.float64)
    assert np.array_equal(copy, code == COPY)
    assert through_table.dtype == ref.dtype == np.float64
    assert through_table.tobytes() == ref.tobytes(), int((through_table != ref).sum())


def _shape(in_len, out_len, batch, waves, run, c):
    """The rules of tree_vjp_table.hpp, restated."""
    staged = 16 * out_len <= c["budget"]
    if in_len < 1:
        return dict(staged=int(staged), waves=0, run=0, runs=0, lds=0)
    if run < 1:
        runs = 1
        if batch < c["compute_units"]:                        # one workgroup per problem would leave units idle
            runs = min(-(-c["compute_units"] // batch), -(-in_len // c["min_run"]))
        run = -(-in_len // runs)
    run = min(run, in_len)
    if -(-in_len // run) > c["max_runs"]:
        run = -(-in_len // c["max_runs"])
    run = -(-run // 2) * 2                                    # whole 16-byte pieces
    waves = c["max_waves"] if not 1 <= waves <= c["max_waves"] else waves
    pieces = -(-run // 2) + 1
    waves = min(waves, -(-pieces // c["lanes"]))
    return dict(staged=int(staged), waves=waves, run=run, runs=-(-in_len // run), lds=16 * out_len if staged else 0)


@pytest.mark.parametrize("name", EXPECTED)
def test_the_launch_shape_follows_its_rules(printed, name):
    consts, trees = printed
    t = trees[name]
    assert len(t["shapes"]) == 6
    for s in t["shapes"]:
        want = _shape(t["in_len"], t["out_len"], s["batch"], s["ask_waves"], s["ask_run"], consts)
        assert {k: s[k] for k in want} == want, (s, want)
        assert s["name"] == ("tree_vjp<staged>/f64" if want["staged"] else "tree_vjp<direct>/f64")
        assert s["run"] * s["runs"] >= t["in_len"] > s["run"] * (s["runs"] - 1)          # the runs cover the arena once
        assert s["lds"] <= consts["budget"] and 1 <= s["waves"] <= consts["max_waves"] and s["runs"] <= consts["max_runs"]
    default = t["shapes"][0]
    assert default["runs"] == 1 and default["ask_run"] == 0                              # batch 4096: one run per problem
    assert (name == "chain_30x70") == (default["staged"] == 0)

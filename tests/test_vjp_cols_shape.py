"""The launch shape of the multi-column chain gradient kernel (csrc/vjp_cols_shape.hpp), without a GPU: the host
program tests/cpp/test_vjp_cols_shape.cpp prints columns, wavefronts, runs, table and LDS bytes for a fixed list of
shapes, and every line is held to the rules the header states:

  never more than 64 KiB of dynamic LDS; at most 8 columns, and 8 wherever 8 columns of one stage fit; the runs cover
  the T + 1 stages exactly; no more wavefronts than stages of a run; gridDim.y <= 65535; "nothing fits" is reported
  (columns 0) and carries nothing that could be launched; the run is the longest the operand budget holds, or, where
  that is fewer than min_run stages, the longest 64 KiB hold."""
import subprocess

import pytest

BUDGET = 65536


def _operand(n, m, run):
    return (run * (2 * n + m) + 2 * n) * 16


def _table(n, m, sym):
    nq, nr = (n * (n + 1) // 2, m * (m + 1) // 2) if sym else (n * n, m * m)
    return ((nq + n + n * n + 2 * n * m + nr) * 4 + 15) // 16 * 16


@pytest.fixture(scope="module")
def lines():
    import __graft_entry__ as entry
    exe = entry.build_vjp_cols_shape_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    head = dict(zip(out[0].split()[::2], map(int, out[0].split()[1::2])))
    rows = []
    for line in out[1:]:
        left, right = line.split(" -> ")
        rows.append((dict(zip(left.split()[::2], map(int, left.split()[1::2]))),
                     dict(zip(right.split()[::2], map(int, right.split()[1::2])))))
    return head, rows


def test_the_list_of_shapes_is_the_one_the_test_expects(lines):
    head, rows = lines
    assert head["budget"] == BUDGET and head["max_columns"] == 8 and head["max_waves"] == 8 and head["max_chunks"] == 65535
    assert head["operand_budget"] in (16384, 32768, 65536) and 1 <= head["waves"] <= 8
    seen = {(r["n"], r["m"], r["T"], r["sym"]) for r, _ in rows if r["requested"] == 8}
    assert {(1, 1, 0, 0), (3, 2, 3, 0), (12, 4, 5, 0), (12, 4, 5, 1), (32, 8, 2, 0), (33, 17, 2, 0), (128, 1, 1, 0),
            (4, 2, 20, 0), (12, 4, 50, 0), (32, 8, 100, 0)} <= seen
    assert any(r["requested"] == 0 for r, _ in rows) and any(r["budget"] == 16384 for r, _ in rows)
    assert any(r["wish_run"] > 0 for r, _ in rows) and any(r["wish_waves"] > 8 for r, _ in rows)
    assert sum(1 for _, got in rows if got["columns"] == 0) >= 5


def test_columns_per_launch(lines):
    """8, or as many columns of ONE stage as 64 KiB hold (without the table)."""
    _, rows = lines
    for r, _ in rows:
        assert r["per_launch"] == min(8, BUDGET // _operand(r["n"], r["m"], 1)), r
    by = {(r["n"], r["m"]): r["per_launch"] for r, _ in rows}
    assert by[(128, 1)] == 7 and by[(256, 4)] == 3 and by[(600, 8)] == 1 and by[(1400, 8)] == 0
    assert by[(12, 4)] == 8 and by[(32, 8)] == 8 and by[(33, 17)] == 8 and by[(64, 8)] == 8


def test_the_bounds_hold_everywhere(lines):
    head, rows = lines
    for r, got in rows:
        if got["columns"] == 0:
            continue
        n, m, T = r["n"], r["m"], r["T"]
        nc = max(r["requested"], 1)
        assert got["columns"] == nc <= r["per_launch"], (r, got)
        assert got["lds"] <= BUDGET, (r, got)
        assert 1 <= got["waves"] <= 8 and got["waves"] <= got["run"], (r, got)
        assert 1 <= got["chunks"] <= 65535, (r, got)
        # the runs cover the T + 1 stages exactly: the last one is not empty and none lies beyond
        assert (got["chunks"] - 1) * got["run"] < T + 1 <= got["chunks"] * got["run"], (r, got)
        # evened out: no shorter run gives the same number of workgroups
        assert got["run"] == -(-(T + 1) // got["chunks"]), (r, got)
        # what the kernel is told is what it lays out: [table] + columns * pairs of the run
        table = _table(n, m, r["sym"])
        assert got["lds"] == (table if got["table"] else 0) + nc * _operand(n, m, got["run"]), (r, got)
        # the table exactly where it and one stage of the group's columns fit together
        assert bool(got["table"]) == (table + nc * _operand(n, m, 1) <= BUDGET), (r, got)


def _first_run(head, r, nc):
    """The run before it is evened out: the wish, or the longest the operand budget holds, or -- where that is fewer
    than min_run stages -- the longest 64 KiB leave beside the table; at most the latter (None: not even one stage)."""
    n, m, stages = r["n"], r["m"], r["T"] + 1
    table = _table(n, m, r["sym"])
    room = BUDGET - (table if table + nc * _operand(n, m, 1) <= BUDGET else 0)
    fixed, stage = nc * _operand(n, m, 0), nc * (_operand(n, m, 1) - _operand(n, m, 0))
    longest = lambda b: 0 if b < fixed + stage else min((b - fixed) // stage, stages)
    most = longest(room)
    if most < 1:
        return None
    if r["wish_run"] > 0:
        return min(r["wish_run"], most)
    want = longest(r["budget"] or head["operand_budget"])
    return most if want < head["min_run"] else min(want, most)


def test_the_run_is_the_longest_the_budget_holds(lines):
    head, rows = lines
    for r, got in rows:
        if got["columns"] == 0:
            continue
        stages = r["T"] + 1
        first = _first_run(head, r, got["columns"])
        chunks = -(-stages // first)
        assert got["chunks"] == chunks and got["run"] == -(-stages // chunks), (r, got, first)
        assert got["waves"] == min(r["wish_waves"] or head["waves"], 8, got["run"]), (r, got)
    by = {(r["n"], r["m"], r["T"], r["requested"], r["budget"], r["wish_run"]): got for r, got in rows}
    assert head["min_run"] == 4
    assert by[(12, 4, 50, 8, 16384, 0)]["run"] == 13 and by[(12, 4, 50, 8, 65536, 0)]["run"] == 13   # 3 < min_run
    assert by[(12, 4, 50, 8, 0, 0)]["run"] == 8 and by[(32, 8, 100, 8, 0, 0)]["run"] == 5            # 8 stays, 2 does not
    assert by[(12, 4, 50, 8, 0, 1000)]["run"] == 13 and by[(12, 4, 50, 8, 0, 9)]["run"] == 9


def test_nothing_fits_is_reported_and_not_launchable(lines):
    head, rows = lines
    for r, got in rows:
        nc = max(r["requested"], 1)
        first = _first_run(head, r, nc) if nc <= r["per_launch"] else None
        launchable = first is not None and -(-(r["T"] + 1) // first) <= 65535
        if got["columns"] == 0:
            assert got == {"columns": 0, "waves": 0, "chunks": 0, "run": 0, "table": 0, "lds": 0}, (r, got)
        assert (got["columns"] > 0) == launchable, (r, got)
    refused = {(r["n"], r["m"], r["T"], r["requested"]) for r, got in rows if got["columns"] == 0}
    assert {(128, 1, 1, 8), (600, 8, 2, 2), (1400, 8, 2, 1), (600, 8, 65535, 1), (1, 1, 70000, 8)} <= refused
    launched = {(r["n"], r["m"], r["T"], r["requested"]) for r, got in rows if got["columns"] > 0}
    assert {(128, 1, 1, 7), (600, 8, 65534, 1), (1, 1, 65534, 8)} <= launched

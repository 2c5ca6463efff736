"""The launch shape of the multi-column tree gradient kernel (csrc/tree_vjp_cols_shape.hpp), without a GPU: the host
program tests/cpp/test_tree_vjp_cols_shape.cpp prints columns, staged, wavefronts, runs and LDS bytes for a fixed list of
arenas, and every line is held to the rule the header states, read from the constants the program prints:

  a plan is staged where one column fits `budget` (64 KiB), else its launches are the direct form with 8 columns; a
  staged launch carries min(8, columns_budget / (16 out_len)) columns -- columns_budget is 64 KiB or, with the kernel's
  limit raised, up to the 160 KiB a workgroup may declare: the test reads which from the program, it does not depend on
  the candidate that was kept; a cap (SIP_LQR_TREE_VJP_MULTI_COLUMNS) on top; a staged launch of nc columns takes
  nc * 16 * out_len bytes, never more than columns_budget, a direct one none; wavefronts and run are those of the
  one-column kernel (8 wavefronts, one run per problem unless the batch is below 256, runs of whole 16-byte pieces that
  cover the arena exactly, gridDim.y <= 65535);
  an empty input arena gives nothing to launch (waves 0)."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def lines():
    import __graft_entry__ as entry
    exe = entry.build_tree_vjp_cols_shape_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    head = dict(zip(out[0].split()[::2], map(int, out[0].split()[1::2])))
    rows = []
    for line in out[1:]:
        left, right = line.split(" -> ")
        rows.append((dict(zip(left.split()[::2], map(int, left.split()[1::2]))),
                     dict(zip(right.split()[::2], map(int, right.split()[1::2])))))
    return head, rows


def _budget(head, r):
    """What the columns of one launch may take: the rule's, or the measuring aid's one budget."""
    return head["columns_budget"] if r["wish_kib"] < 0 else min(r["wish_kib"] * 1024, head["most"])


def _fit(head, r):
    """Columns that go through LDS together; 0: the direct form."""
    column = head["pair"] * r["out_len"]
    if r["out_len"] < 1:
        return 8
    if r["wish_kib"] < 0 and column > head["budget"]:
        return 0
    return min(8, _budget(head, r) // column)


def test_the_constants_and_the_list_are_what_the_test_expects(lines):
    head, rows = lines
    assert head["budget"] == 64 * 1024 and head["most"] == 160 * 1024 and head["pair"] == 16
    assert head["budget"] <= head["columns_budget"] <= head["most"]
    assert head["max_columns"] == 8 and head["max_waves"] == 8 and head["lanes"] == 64 and head["piece"] == 2
    assert head["compute_units"] == 256 and head["max_runs"] == 65535
    plain = {r["out_len"] for r, _ in rows if r["wish_kib"] < 0 and r["cap"] == 0}
    assert {512, 513, 1280, 1281, 4096, 4097, 636, 1148, 0} <= plain
    assert any(r["cap"] > 0 for r, _ in rows) and any(r["batch"] < 256 and r["in_len"] > 0 for r, _ in rows)
    assert any(r["requested"] == 0 for r, _ in rows) and any(r["wish_kib"] == 0 for r, _ in rows)
    assert any(r["wish_kib"] > 64 for r, _ in rows) and any(r["wish_run"] > 0 for r, _ in rows)


def test_columns_per_launch(lines):
    head, rows = lines
    for r, _ in rows:
        fit = _fit(head, r)
        cols = fit if fit > 0 else 8
        assert r["per_launch"] == (min(cols, r["cap"]) if r["cap"] > 0 else cols), r
    by = {(r["out_len"], r["cap"]): r["per_launch"] for r, _ in rows if r["wish_kib"] < 0}
    room = head["columns_budget"] // 16                      # pairs the columns of a launch may take
    for out_len in (512, 513, 636, 1148, 1280, 1281, 4096):
        assert by[(out_len, 0)] == min(8, room // out_len), out_len
    assert by[(512, 0)] == 8 and by[(4097, 0)] == 8 and by[(4476, 0)] == 8 and by[(0, 0)] == 8
    assert by[(512, 3)] == 3 and by[(512, 1)] == 1 and by[(1148, 2)] == 2 and by[(4476, 3)] == 3
    assert by[(1148, 5)] == min(5, room // 1148)
    # the three candidates of the measurement, whatever the rule: 64 KiB, the limit raised, the direct form
    aid = {r["wish_kib"]: (r["per_launch"], got["staged"]) for r, got in rows if r["wish_kib"] >= 0 and r["cap"] == 0}
    assert aid[147] == (8, 1) and aid[160] == (8, 1) and aid[999] == (8, 1) and aid[0] == (8, 0)


def test_staged_exactly_where_the_columns_fit(lines):
    head, rows = lines
    for r, got in rows:
        if got["waves"] == 0:
            continue
        nc = max(r["requested"], 1)
        assert got["columns"] == nc, (r, got)
        assert bool(got["staged"]) == (nc <= _fit(head, r)), (r, got)
        assert got["lds"] == (nc * 16 * r["out_len"] if got["staged"] else 0), (r, got)
        assert got["lds"] <= _budget(head, r), (r, got)
        assert got["lds"] <= head["most"], (r, got)
    by = {(r["out_len"], r["requested"], r["wish_kib"], r["cap"]): got for r, got in rows if r["batch"] >= 256}
    assert by[(512, 8, -1, 0)]["staged"] == 1 and by[(512, 8, -1, 0)]["lds"] == 65536
    assert by[(513, 7, -1, 0)]["staged"] == 1 and by[(4096, 1, -1, 0)]["lds"] == 65536
    assert by[(4097, 8, -1, 0)]["staged"] == 0 and by[(1148, 3, -1, 0)]["lds"] == 3 * 16 * 1148
    for out_len in (1148, 1280):                             # 8 columns staged exactly where the rule's budget holds them
        assert by[(out_len, 8, -1, 0)]["staged"] == int(8 * 16 * out_len <= head["columns_budget"])
    assert by[(1148, 8, 147, 0)] == dict(by[(1148, 8, 147, 0)], staged=1, lds=8 * 16 * 1148)
    assert by[(1148, 8, 0, 0)]["staged"] == 0 and by[(1148, 8, 0, 0)]["lds"] == 0
    direct = {r["requested"]: got for r, got in rows if r["out_len"] == 4476}
    assert all(got["staged"] == 0 and got["lds"] == 0 for got in direct.values()) and {0, 1, 3, 8} <= set(direct)


def test_wavefronts_and_runs(lines):
    head, rows = lines
    piece, lanes = head["piece"], head["lanes"]
    for r, got in rows:
        if got["waves"] == 0:
            continue
        n = r["in_len"]
        # the runs cover the arena exactly, start on whole pieces, and fit gridDim.y
        assert got["run"] % piece == 0 and 1 <= got["runs"] <= head["max_runs"], (r, got)
        assert (got["runs"] - 1) * got["run"] < n <= got["runs"] * got["run"], (r, got)
        if r["wish_run"] > 0:
            want = min(r["wish_run"], n)
        elif r["batch"] >= head["compute_units"]:
            want = n
        else:
            idle, most = -(-head["compute_units"] // r["batch"]), -(-n // head["min_run"])
            want = -(-n // min(idle, most))
        assert got["run"] == -(-want // piece) * piece, (r, got)
        waves = r["wish_waves"] if 1 <= r["wish_waves"] <= 8 else 8
        fill = -(-(got["run"] // piece + 1) // lanes)
        assert got["waves"] == min(waves, fill), (r, got)
    by = {(r["in_len"], r["batch"], r["wish_run"]): got for r, got in rows if r["wish_kib"] < 0 and r["cap"] == 0
          and r["requested"] == 8 and r["wish_waves"] == 0}
    assert by[(20000, 4096, 0)]["runs"] == 1 and by[(20000, 256, 0)]["runs"] == 1
    assert by[(20000, 255, 0)]["runs"] == 2 and by[(20000, 3, 0)]["runs"] == 5 and by[(151, 3, 0)]["runs"] == 1
    assert by[(151, 3, 0)]["waves"] == 2 and by[(5001, 100, 0)]["runs"] == 2


def test_an_empty_arena_launches_nothing(lines):
    _, rows = lines
    empty = [got for r, got in rows if r["in_len"] == 0]
    assert len(empty) >= 2
    for got in empty:
        assert got["waves"] == 0 and got["runs"] == 0 and got["run"] == 0 and got["lds"] == 0, got
    assert all(got["waves"] > 0 for r, got in rows if r["in_len"] > 0)

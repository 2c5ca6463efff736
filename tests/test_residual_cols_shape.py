"""The launch shape of the chain residual, for one column and for several (csrc/residual_cols_shape.hpp), without a GPU:
the host program
tests/cpp/test_residual_cols_shape.cpp prints columns, wavefronts, staged and LDS bytes for a fixed list of shapes, and
every line is recomputed here from the rules the header states:

  never more than 64 KiB of dynamic LDS; staged needs `mats` 16-byte aligned and the image plus NC vector sets to fit;
  staged with fewer columns before unstaged with more; among those the largest column count that leaves `want_waves`
  wavefronts (or one per stage on a shorter chain), else the largest that fits; no more wavefronts than stages."""
import re
import subprocess

import pytest

BUDGET = 65536


def _z_bytes(n, m, nc):
    return ((nc * (6 * n + 2 * m) + n + 1) // 2 * 2) * 8


def _image_bytes(n, m, f32, sym):
    nq, nr = (n * (n + 1) // 2, m * (m + 1) // 2) if sym else (n * n, m * m)
    stg = nq + n + n * n + 2 * n * m + nr
    return (stg * (4 if f32 else 8) + 16 + 15) // 16 * 16


def _single_column_stages(n, m, f32, sym, aligned):
    """Where one column stages: exactly where the rule the single-column kernel had of its own staged (32 bytes for the
    norms, 7 n + 2 m doubles of vectors and the image within 64 KiB, `mats` aligned)."""
    z = ((7 * n + 2 * m + 1) // 2 * 2) * 8
    return aligned and z + _image_bytes(n, m, f32, sym) <= BUDGET - 32


def _expected(n, m, T, f32, sym, aligned, requested, max_columns, max_waves, want_waves):
    top = 1
    while top < requested and top < max_columns:
        top *= 2
    stages = T + 1
    want = min(want_waves, stages)
    for staged in ((True, False) if aligned else (False,)):
        for need in ([want, 1] if want > 1 else [1]):
            nc = top
            while nc >= 1:
                red = nc * 8 * max_waves
                wave = _z_bytes(n, m, nc) + (_image_bytes(n, m, f32, sym) if staged else 0)
                if red + need * wave <= BUDGET:
                    waves = min((BUDGET - red) // wave, max_waves, stages)
                    return nc, waves, staged, red + waves * wave
                nc //= 2
    return 0, 0, False, 0


@pytest.fixture(scope="module")
def lines():
    import __graft_entry__ as entry
    exe = entry.build_residual_cols_shape_test()
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
    assert head == {"budget": BUDGET, "max_columns": 8, "max_waves": 4, "want_waves": head["want_waves"]}
    assert 1 <= head["want_waves"] <= 4
    seen = {(r["n"], r["m"], r["f32"], r["sym"]) for r, _ in rows if r["aligned"] and r["requested"] == 8}
    for n, m in ((1, 1), (5, 3), (12, 4), (16, 8), (32, 8)):
        assert (n, m, 0, 0) in seen and (n, m, 1, 0) in seen
    assert (8, 4, 0, 1) in seen and {(35, 3, 0, 0), (60, 8, 0, 0), (64, 8, 0, 0)} <= seen
    assert any(not r["aligned"] for r, _ in rows)
    assert any(r["T"] + 1 < 4 and r["n"] > 1 for r, _ in rows)


def test_every_line_is_what_the_rules_give(lines):
    head, rows = lines
    for r, got in rows:
        want = _expected(r["n"], r["m"], r["T"], r["f32"], r["sym"], r["aligned"], r["requested"],
                         head["max_columns"], head["max_waves"], head["want_waves"])
        assert (got["columns"], got["waves"], bool(got["staged"]), got["lds"]) == want, (r, got, want)


def test_the_bounds_hold_everywhere(lines):
    _, rows = lines
    for r, got in rows:
        assert got["lds"] <= BUDGET, (r, got)
        assert 1 <= got["columns"] <= 8 and got["columns"] in (1, 2, 4, 8), (r, got)
        assert 1 <= got["waves"] <= 4 and got["waves"] <= r["T"] + 1, (r, got)
        assert got["columns"] >= min(r["requested"], 1)
        # a short group is never launched on an instantiation twice as wide as it needs
        assert got["columns"] < 2 * max(r["requested"], 1), (r, got)
        # what the kernel is told fits what it lays out: red + waves * (vectors [+ image])
        wave = _z_bytes(r["n"], r["m"], got["columns"]) + \
            (_image_bytes(r["n"], r["m"], r["f32"], r["sym"]) if got["staged"] else 0)
        assert got["lds"] == got["columns"] * 32 + got["waves"] * wave, (r, got)


def test_staged_exactly_where_it_can_be(lines):
    _, rows = lines
    for r, got in rows:
        image = _image_bytes(r["n"], r["m"], r["f32"], r["sym"])
        if not r["aligned"] or image > BUDGET:
            assert not got["staged"], (r, got)
        one_column_fits = 32 + _z_bytes(r["n"], r["m"], 1) + image <= BUDGET
        if _single_column_stages(r["n"], r["m"], r["f32"], r["sym"], bool(r["aligned"])) and one_column_fits:
            assert got["staged"], (r, got)
    # the shapes of the issue: (64, 8) in fp64 has a 76 KB image, (60, 8) one of 67 KB: neither can be staged
    by = {(r["n"], r["m"], r["f32"]): got for r, got in rows if r["aligned"] and r["requested"] == 8 and r["T"] > 2}
    assert not by[(64, 8, 0)]["staged"] and not by[(60, 8, 0)]["staged"] and by[(35, 3, 0)]["staged"]
    assert by[(32, 8, 0)]["staged"] and by[(32, 8, 1)]["staged"]

"""The manifest of the fused fp64 chain kernels (csrc/gen_qw16_kernels.py): the one list the slices of
qw16_kernels.hip, the dispatch of sip_lqr_amd.hip and the build take their shapes from."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location(
    "gen_qw16_kernels", os.path.join(ROOT, "sip_optimal_control_amd", "csrc", "gen_qw16_kernels.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

SLICES = gen.manifest()
ENTRIES = [e for s in SLICES for e in s]
GRID = {(n, m) for n in range(1, 17) for m in range(1, 9)}
SYMMETRIC = {(12, 4), (8, 4), (4, 4)}
# the benchmark grid n in {4, 6, 8, 12} x m in {1, 2, 3, 4}, three small shapes, the hosts of the embedding, n = 16
CORE = {(4, 1), (4, 2), (4, 3), (4, 4), (6, 1), (6, 2), (6, 3), (6, 4), (8, 1), (8, 2), (8, 3), (8, 4),
        (12, 1), (12, 2), (12, 3), (12, 4), (1, 1), (2, 1), (3, 2), (8, 8), (12, 8), (14, 4), (14, 8), (15, 4), (15, 8),
        (16, 1), (16, 2), (16, 3), (16, 4), (16, 8)}


def test_slice_count_is_the_builds():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    assert len(SLICES) == gen.SLICES == entry.QW16_SLICES
    assert sum(1 for _, src, _, _ in entry.hip_units() if src.endswith("qw16_kernels.hip")) == gen.SLICES


def test_every_shape_has_one_default_kernel_staged_up_to_15():
    assert len(CORE) == 30
    for shape in GRID:
        # the default: the first full-layout entry of the shape in its slice (find_kernel takes the first match)
        full = [e for e in ENTRIES if (e.n, e.m) == shape and not e.sym]
        assert len(full) == (2 if shape in {(12, 4), (4, 2)} else 1)
        assert full[0].staged == (shape[0] <= 15) and full[0].mrhs
        assert [e.staged for e in full[1:]] == [False] * (len(full) - 1)  # the alternative: the direct kernel
        assert len({id(s) for s in SLICES for e in s if e in full}) == 1  # alternatives stay in one slice
    assert {(e.n, e.m) for e in ENTRIES} == GRID
    assert {(e.n, e.m) for e in ENTRIES if e.sym} == SYMMETRIC
    assert all(e.staged and e.split and not e.mrhs for e in ENTRIES if e.sym)
    assert (len(ENTRIES), sum(e.mrhs for e in ENTRIES), sum(e.split for e in ENTRIES)) == (133, 130, 91)


def test_core_set():
    assert {(e.n, e.m) for e in ENTRIES if e.core} == CORE
    assert all(e.core == ((e.n, e.m) in CORE) for e in ENTRIES)


def test_split_set():
    rule = {(n, m) for n, m in GRID if n <= 15 and n * (n + m) % 2 == 0}
    assert len(rule) == 88
    assert {(e.n, e.m) for e in ENTRIES if e.split and not e.sym} == rule
    assert {(e.n, e.m) for e in ENTRIES if e.split and e.sym} == SYMMETRIC
    assert all(e.staged for e in ENTRIES if e.split)


def test_no_kernel_in_two_slices():
    keys = [(e.n, e.m, e.staged, e.sym) for e in ENTRIES]
    assert len(keys) == len(set(keys))
    assert all(SLICES)  # no empty translation unit


def test_shape_option():
    (only,) = gen.manifest("12x4")
    assert only == [gen.Entry(12, 4, True, False, True, True, True)]  # fused staged, multi-rhs and split
    (core,) = gen.manifest("core")
    assert sorted(core) == sorted(e for e in ENTRIES if e.core)
    (two,) = gen.manifest("14x8,16x2")
    assert sorted((e.n, e.m, e.staged) for e in two) == [(14, 8, True), (16, 2, False)]
    text = gen.render(gen.manifest("12x4"))
    assert "#define QW16_SLICE_COUNT 1\n" in text and text.count("QW16_ENTRY(") == 1
    assert 'QW16_ENTRY(12, 4, true, false, "staged", true, QW16_MRHS, QW16_SPLIT)' in text

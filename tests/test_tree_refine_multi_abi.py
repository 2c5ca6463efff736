"""sip_lqr_tree_residual_multi_columns, sip_lqr_tree_residual_multi_kernel_name, sip_lqr_tree_residual_multi,
sip_lqr_tree_refine_multi_workspace_bytes and sip_lqr_tree_refine_multi without a GPU: the symbols, the header and the
argument checks.

The calls are made in a child process that sees no HIP device (HIP_VISIBLE_DEVICES=-1), as tests/test_tree_refine_abi.py
makes them: a misuse returns SIP_LQR_ERR_INVALID_ARGUMENT before any HIP call.  A tree plan with a valid topology cannot
exist in that process; a plan with a latched invalid topology can, and everything is refused on it.  The checks that
need a valid plan are made in tests/test_gpu_tree_refine_multi.py."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sip_lqr_tree_residual_multi_columns", "sip_lqr_tree_residual_multi_kernel_name", "sip_lqr_tree_residual_multi",
       "sip_lqr_tree_refine_multi_workspace_bytes", "sip_lqr_tree_refine_multi")
OK, INVALID = 0, -1

CHILD = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
from sip_optimal_control_amd._lib import load_library
lib = load_library()
out = {}
ints = lambda v: (ctypes.c_int * len(v))(*v)
P = ctypes.c_void_p(4096)         # never dereferenced: the checks come before any HIP call
N = None
def calls(h):
    res = lambda **kw: lib.sip_lqr_tree_residual_multi(*[kw.get(k, d) for k, d in (
        ("plan", h), ("input", P), ("rhs", N), ("out", P), ("num_rhs", 3), ("res", P), ("norms", P), ("stream", N))])
    ref = lambda **kw: lib.sip_lqr_tree_refine_multi(*[kw.get(k, d) for k, d in (
        ("plan", h), ("input", P), ("work", P), ("rhs", P), ("out", P), ("num_rhs", 3), ("iterations", 2),
        ("from_zero", 1), ("status", P), ("rws", P), ("norms", P), ("stream", N))])
    return res, ref
def facts(h):
    return {"columns": int(lib.sip_lqr_tree_residual_multi_columns(h)),
            "name": lib.sip_lqr_tree_residual_multi_kernel_name(h).decode(),
            "bytes": [int(lib.sip_lqr_tree_refine_multi_workspace_bytes(h, k)) for k in (-1, 0, 1, 3, 9)]}
res, ref = calls(None)
out["null_plan"] = dict(facts(None), residual=res(), refine=ref(), residual0=res(num_rhs=0), refine0=ref(num_rhs=0))
# a cycle: 0 -> 1 -> 0 (latched; the plan exists without a device)
bad = ctypes.c_void_p()
rc = lib.sip_lqr_tree_plan_create(3, 2, 0, ints([0, 1]), ints([1, 0]), ints([2, 2, 2]), ints([1, 1]), 0, ctypes.byref(bad))
out["latched_create"] = [rc, lib.sip_lqr_tree_topology_status(bad)]
res, ref = calls(bad)
out["latched_facts"] = facts(bad)
out["latched"] = {"residual": res(), "residual with rhs": res(rhs=P), "residual of no column": res(num_rhs=0),
                  "refine": ref(), "refine from the iterates": ref(from_zero=0), "refine of no column": ref(num_rhs=0),
                  "residual num_rhs=-1": res(num_rhs=-1), "refine num_rhs=-1": ref(num_rhs=-1),
                  "residual norms": res(norms=N), "residual out": res(out=N), "refine status": ref(status=N),
                  "refine rws": ref(rws=N), "iterations=0": ref(iterations=0), "from_zero=2": ref(from_zero=2)}
lib.sip_lqr_tree_plan_destroy(bad)
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_hip()
    from sip_optimal_control_amd._lib import load_library
    return load_library()


@pytest.fixture(scope="module")
def child(lib, tmp_path_factory):
    script = tmp_path_factory.mktemp("tree_refine_multi_abi") / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    line = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_the_symbols_are_exported_and_bound(lib):
    from sip_optimal_control_amd import _lib
    raw = ctypes.CDLL(_lib.library_path())
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    sig, P, I = _lib._SIGNATURES, ctypes.c_void_p, ctypes.c_int
    assert sig["sip_lqr_tree_residual_multi_columns"] == (I, [P])
    assert sig["sip_lqr_tree_residual_multi_kernel_name"] == (ctypes.c_char_p, [P])
    assert sig["sip_lqr_tree_residual_multi"] == (I, [P, P, P, P, I, P, P, P])
    assert sig["sip_lqr_tree_refine_multi_workspace_bytes"] == (ctypes.c_size_t, [P, I])
    assert sig["sip_lqr_tree_refine_multi"] == (I, [P, P, P, P, P, I, I, I, P, P, P, P])
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    for name in ("residual_multi", "refine_multi", "residual_multi_kernel_name"):
        assert hasattr(BatchedTreeLQR, name), name


def test_the_header_declares_them_and_is_plain_c(tmp_path):
    text = open(os.path.join(ROOT, "include", "sip_lqr_amd.h")).read()
    for name in NEW:
        assert name + "(" in text, name
    # the documented scratch size
    assert "2 * up(num_rhs * batch * sip_lqr_tree_rhs_len() * 8) + up(num_rhs * batch * 8) +" in text
    assert "up(sip_lqr_tree_solve_multi_scratch_bytes(plan, num_rhs))" in text
    src = tmp_path / "hdr.c"
    src.write_text('#include "sip_lqr_amd.h"\n'
                   "int main(void) {\n"
                   "  int (*c)(const sip_lqr_tree_plan *) = sip_lqr_tree_residual_multi_columns;\n"
                   "  const char *(*k)(const sip_lqr_tree_plan *) = sip_lqr_tree_residual_multi_kernel_name;\n"
                   "  int (*r)(const sip_lqr_tree_plan *, const double *, const double *, const double *, int, double *,\n"
                   "           double *, void *) = sip_lqr_tree_residual_multi;\n"
                   "  size_t (*b)(const sip_lqr_tree_plan *, int) = sip_lqr_tree_refine_multi_workspace_bytes;\n"
                   "  int (*f)(const sip_lqr_tree_plan *, const double *, const double *, const double *, double *, int,\n"
                   "           int, int, const int32_t *, void *, double *, void *) = sip_lqr_tree_refine_multi;\n"
                   "  return c == 0 || k == 0 || r == 0 || b == 0 || f == 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_a_null_plan_is_refused(child):
    assert child["null_plan"] == {"columns": 0, "name": "", "bytes": [0] * 5, "residual": INVALID, "refine": INVALID,
                                  "residual0": INVALID, "refine0": INVALID}


def test_a_latched_invalid_topology_is_refused(child):
    assert child["latched_create"] == [OK, 4]                 # the plan exists; SIP_LQR_INVALID_TOPOLOGY is latched
    assert child["latched_facts"] == {"columns": 0, "name": "", "bytes": [0] * 5}
    for what, rc in child["latched"].items():
        assert rc == INVALID, (what, rc)
    assert len(child["latched"]) == 14


def test_the_workspace_is_zero_without_columns(child):
    """num_rhs 0 and -1 (and any num_rhs on a plan that cannot run): no scratch."""
    assert child["null_plan"]["bytes"][:2] == [0, 0] and child["latched_facts"]["bytes"][:2] == [0, 0]

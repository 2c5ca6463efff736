"""sip_lqr_tree_residual_kernel_name, sip_lqr_tree_residual, sip_lqr_tree_refine_workspace_bytes and sip_lqr_tree_refine
without a GPU: the symbols, the header and the argument checks.

The calls are made in a child process that sees no HIP device (HIP_VISIBLE_DEVICES=-1): a misuse returns
SIP_LQR_ERR_INVALID_ARGUMENT before any HIP call.  A tree plan with a valid topology uploads its tables when it is
created, so it cannot exist in that process (sip_lqr_tree_plan_create returns SIP_LQR_ERR_HIP there, asserted below); a
plan with a latched invalid topology can, and everything is refused on it.  The checks that need a valid plan -- a
missing pointer, iterations, from_zero, and the size of the refine scratch on three plans -- are made where one exists,
in tests/test_gpu_tree_refine.py."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sip_lqr_tree_residual_kernel_name", "sip_lqr_tree_residual", "sip_lqr_tree_refine_workspace_bytes",
       "sip_lqr_tree_refine")
OK, INVALID, ERR_HIP = 0, -1, -3

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
    res = lambda **kw: lib.sip_lqr_tree_residual(*[kw.get(k, d) for k, d in (
        ("plan", h), ("input", P), ("rhs", N), ("output", P), ("res", P), ("norm", P), ("stream", N))])
    ref = lambda **kw: lib.sip_lqr_tree_refine(*[kw.get(k, d) for k, d in (
        ("plan", h), ("input", P), ("work", P), ("rhs", N), ("output", P), ("iterations", 2), ("from_zero", 1),
        ("status", P), ("rws", P), ("norms", P), ("stream", N))])
    return res, ref
res, ref = calls(None)
out["null_plan"] = {"residual": res(), "refine": ref(), "bytes": int(lib.sip_lqr_tree_refine_workspace_bytes(None)),
                    "name": lib.sip_lqr_tree_residual_kernel_name(None).decode()}
# a cycle: 0 -> 1 -> 0 (latched; the plan exists without a device)
bad = ctypes.c_void_p()
rc = lib.sip_lqr_tree_plan_create(3, 2, 0, ints([0, 1]), ints([1, 0]), ints([2, 2, 2]), ints([1, 1]), 0, ctypes.byref(bad))
out["latched_create"] = [rc, lib.sip_lqr_tree_topology_status(bad)]
res, ref = calls(bad)
out["latched"] = {"residual": res(), "residual with rhs": res(rhs=P), "refine": ref(),
                  "refine from the iterate": ref(from_zero=0), "bytes": int(lib.sip_lqr_tree_refine_workspace_bytes(bad))}
out["misuse_on_latched"] = {
    "residual norm": res(norm=N), "residual input": res(input=N), "residual output": res(output=N),
    "refine input": ref(input=N), "refine work": ref(work=N), "refine output": ref(output=N),
    "refine status": ref(status=N), "refine rws": ref(rws=N), "refine norms": ref(norms=N),
    "iterations=0": ref(iterations=0), "iterations=33": ref(iterations=33), "iterations=-1": ref(iterations=-1),
    "from_zero=2": ref(from_zero=2), "from_zero=-1": ref(from_zero=-1)}
lib.sip_lqr_tree_plan_destroy(bad)
count, hip = ctypes.c_int(0), None
for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
    try:
        hip = ctypes.CDLL(name)
        break
    except OSError:
        pass
out["devices_visible"] = None if hip is None else int(hip.hipGetDeviceCount(ctypes.byref(count)) == 0 and count.value > 0)
good = ctypes.c_void_p()
out["valid_create"] = lib.sip_lqr_tree_plan_create(3, 2, 0, ints([0, 0]), ints([1, 2]), ints([2, 2, 2]), ints([1, 1]), 0,
                                                   ctypes.byref(good))
if good.value:
    lib.sip_lqr_tree_plan_destroy(good)
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
    script = tmp_path_factory.mktemp("tree_refine_abi") / "child.py"
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
    sig = _lib._SIGNATURES
    assert sig["sip_lqr_tree_residual_kernel_name"] == (ctypes.c_char_p, [ctypes.c_void_p])
    assert sig["sip_lqr_tree_residual"][0] is ctypes.c_int and len(sig["sip_lqr_tree_residual"][1]) == 7
    assert sig["sip_lqr_tree_refine_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert sig["sip_lqr_tree_refine"][0] is ctypes.c_int and len(sig["sip_lqr_tree_refine"][1]) == 11
    assert sig["sip_lqr_tree_refine"][1][5:7] == [ctypes.c_int, ctypes.c_int]      # iterations, from_zero


def test_the_header_declares_them_and_is_plain_c(tmp_path):
    text = open(os.path.join(ROOT, "include", "sip_lqr_amd.h")).read()
    for name in NEW:
        assert name + "(" in text, name
    assert "2 * up(batch * sip_lqr_tree_rhs_len() * 8) + up(batch * 8)" in text     # the documented scratch size
    src = tmp_path / "hdr.c"
    src.write_text('#include "sip_lqr_amd.h"\n'
                   "int main(void) {\n"
                   "  const char *(*k)(const sip_lqr_tree_plan *) = sip_lqr_tree_residual_kernel_name;\n"
                   "  int (*r)(const sip_lqr_tree_plan *, const double *, const double *, const double *, double *,\n"
                   "           double *, void *) = sip_lqr_tree_residual;\n"
                   "  size_t (*b)(const sip_lqr_tree_plan *) = sip_lqr_tree_refine_workspace_bytes;\n"
                   "  int (*f)(const sip_lqr_tree_plan *, const double *, const double *, const double *, double *, int,\n"
                   "           int, const int32_t *, void *, double *, void *) = sip_lqr_tree_refine;\n"
                   "  return k == 0 || r == 0 || b == 0 || f == 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_a_null_plan_is_refused(child):
    assert child["null_plan"] == {"residual": INVALID, "refine": INVALID, "bytes": 0, "name": ""}


def test_a_latched_invalid_topology_is_refused(child):
    assert child["latched_create"] == [OK, 4]                 # the plan exists; SIP_LQR_INVALID_TOPOLOGY is latched
    for what, rc in child["latched"].items():
        assert rc == (0 if what == "bytes" else INVALID), (what, rc)
    for what, rc in child["misuse_on_latched"].items():
        assert rc == INVALID, (what, rc)
    assert len(child["misuse_on_latched"]) == 14


def test_a_valid_plan_needs_a_device(child):
    """Why the remaining checks live in the GPU file: no valid tree plan without a device."""
    assert child["devices_visible"] == 0, "the child process was to see no HIP device"
    assert child["valid_create"] == ERR_HIP

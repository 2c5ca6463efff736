"""sip_lqr_residual_multi_columns, sip_lqr_residual_multi, sip_lqr_refine_multi_workspace_bytes and sip_lqr_refine_multi
without a GPU: the symbols, the header, the size of the refine scratch and the argument checks.

As in tests/test_refine_abi.py the calls are made in a child process that sees no HIP device (HIP_VISIBLE_DEVICES=-1),
on a plan that therefore has none: a misuse returns SIP_LQR_ERR_INVALID_ARGUMENT before any HIP call, a well-formed
call returns SIP_LQR_ERR_HIP instead of launching on the made-up pointers, and num_rhs = 0 returns SIP_LQR_OK having
launched nothing."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sip_lqr_residual_multi_columns", "sip_lqr_residual_multi", "sip_lqr_refine_multi_workspace_bytes",
       "sip_lqr_refine_multi")
OK, INVALID, ERR_HIP = 0, -1, -3

CHILD = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
from sip_optimal_control_amd._lib import load_library
lib = load_library()
out = {}
P = ctypes.c_void_p(4096)         # never dereferenced: the plans have no device
N = None
def calls(h):
    res = lambda **kw: lib.sip_lqr_residual_multi(*[kw.get(k, d) for k, d in (
        ("plan", h), ("mats", P), ("vecs", P), ("sol", P), ("num_rhs", 9), ("wide", 0), ("res", P), ("norms", P),
        ("stream", N))])
    ref = lambda **kw: lib.sip_lqr_refine_multi(*[kw.get(k, d) for k, d in (
        ("plan", h), ("mats", P), ("vecs", P), ("sol", P), ("num_rhs", 9), ("iterations", 3), ("from_zero", 1),
        ("gains", P), ("ws", P), ("cws", P), ("rws", P), ("status", P), ("norms", P), ("stream", N))])
    return res, ref
h = ctypes.c_void_p()           # fp32 general engine: solve_multi goes column by column, no column workspace
assert lib.sip_lqr_plan_create(1, 6, 5, 12, 4, 0, ctypes.byref(h)) == 0
assert lib.sip_lqr_solve_multi_workspace_bytes(h, 9) == 0
g = ctypes.c_void_p()           # fp64 (12, 4): the 8-column sweep, which needs its column workspace
assert lib.sip_lqr_plan_create(0, 6, 5, 12, 4, 0, ctypes.byref(g)) == 0
assert lib.sip_lqr_solve_multi_workspace_bytes(g, 9) > 0
res, ref = calls(h)
gres, gref = calls(g)
out["residual_misuse"] = {
    "plan": res(plan=N), "mats": res(mats=N), "norms": res(norms=N), "num_rhs=-1": res(num_rhs=-1),
    "vecs": res(vecs=N), "sol": res(sol=N), "vecs, one column": res(vecs=N, num_rhs=1), "wide=2": res(wide=2),
    "wide=-1": res(wide=-1), "wide=2, no columns": res(wide=2, num_rhs=0), "norms, no columns": res(norms=N, num_rhs=0)}
out["refine_misuse"] = {
    "plan": ref(plan=N), "mats": ref(mats=N), "vecs": ref(vecs=N), "sol": ref(sol=N), "gains": ref(gains=N),
    "ws": ref(ws=N), "rws": ref(rws=N), "norms": ref(norms=N), "iterations=0": ref(iterations=0),
    "iterations=33": ref(iterations=33), "iterations=-1": ref(iterations=-1), "from_zero=2": ref(from_zero=2),
    "from_zero=-1": ref(from_zero=-1), "num_rhs=-1": ref(num_rhs=-1),
    "column workspace where bytes are needed": gref(cws=N)}
out["no_columns"] = {
    "residual": res(num_rhs=0), "residual, no vecs, no sol, no vector": res(num_rhs=0, vecs=N, sol=N, res=N),
    "refine": ref(num_rhs=0), "refine, no column workspace": gref(num_rhs=0, cws=N)}
out["columns"] = {"f32 (12,4)": lib.sip_lqr_residual_multi_columns(h), "f64 (12,4)": lib.sip_lqr_residual_multi_columns(g),
                  "NULL": lib.sip_lqr_residual_multi_columns(N)}
# the well-formed calls are made only where the HIP runtime itself reports no device to this process
count, hip = ctypes.c_int(0), None
for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
    try:
        hip = ctypes.CDLL(name)
        break
    except OSError:
        pass
out["devices_visible"] = None if hip is None else int(hip.hipGetDeviceCount(ctypes.byref(count)) == 0 and count.value > 0)
if out["devices_visible"] == 0:
    out["deviceless"] = {
        "residual": res(), "residual wide, no vector, one column": res(wide=1, res=N, num_rhs=1),
        "refine": ref(), "refine, NULL column workspace where none is needed": ref(cws=N),
        "refine, no status, 32 rounds, from the iterates": gref(status=N, iterations=32, from_zero=0)}
lib.sip_lqr_plan_destroy(h)
lib.sip_lqr_plan_destroy(g)
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
    script = tmp_path_factory.mktemp("refine_multi_abi") / "child.py"
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
    assert sig["sip_lqr_residual_multi_columns"] == (ctypes.c_int, [ctypes.c_void_p])
    assert sig["sip_lqr_residual_multi"][0] is ctypes.c_int and len(sig["sip_lqr_residual_multi"][1]) == 9
    assert sig["sip_lqr_refine_multi_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int])
    assert sig["sip_lqr_refine_multi"][0] is ctypes.c_int and len(sig["sip_lqr_refine_multi"][1]) == 14


def test_the_header_declares_them_and_is_plain_c(tmp_path):
    text = open(os.path.join(ROOT, "include", "sip_lqr_amd.h")).read()
    for name in NEW:
        assert name + "(" in text, name
    src = tmp_path / "hdr.c"
    src.write_text('#include "sip_lqr_amd.h"\n'
                   "int main(void) {\n"
                   "  int (*c)(const sip_lqr_plan *) = sip_lqr_residual_multi_columns;\n"
                   "  int (*r)(const sip_lqr_plan *, const void *, const void *, const void *, int, int, double *,\n"
                   "           double *, void *) = sip_lqr_residual_multi;\n"
                   "  size_t (*b)(const sip_lqr_plan *, int) = sip_lqr_refine_multi_workspace_bytes;\n"
                   "  int (*f)(const sip_lqr_plan *, const void *, const double *, double *, int, int, int, void *,\n"
                   "           void *, void *, void *, const int32_t *, double *, void *) = sip_lqr_refine_multi;\n"
                   "  return c == 0 || r == 0 || b == 0 || f == 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def _up(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("num_rhs", [0, 1, 9])
@pytest.mark.parametrize("dtype,n,m,T,batch,opt_ins", [
    (0, 12, 4, 50, 4096, ()),
    (1, 5, 3, 12, 3, ()),
    (1, 5, 3, 12, 3, ("fused_f32", "separate_sweeps")),
    (1, 32, 8, 100, 1024, ("separate_sweeps",)),
])
def test_refine_multi_workspace_bytes_is_what_the_header_documents(lib, dtype, n, m, T, batch, opt_ins, num_rhs):
    h = ctypes.c_void_p()
    assert lib.sip_lqr_plan_create(dtype, batch, T, n, m, 0, ctypes.byref(h)) == OK
    for opt in opt_ins:
        assert getattr(lib, "sip_lqr_plan_set_" + opt)(h, 1) == OK
        assert getattr(lib, "sip_lqr_has_" + opt)(h) == 1
    vecs_len, scalar = int(lib.sip_lqr_vecs_len(h)), int(lib.sip_lqr_scalar_bytes(h))
    assert vecs_len == (T + 1) * 2 * n + T * m and scalar == (4 if dtype else 8)
    # rho / s and d as [num_rhs][batch][vecs_len] in the plan's dtype, then s[c][p]: each region a multiple of 256 bytes
    want = 2 * _up(num_rhs * batch * vecs_len * scalar) + _up(num_rhs * batch * 8)
    assert int(lib.sip_lqr_refine_multi_workspace_bytes(h, num_rhs)) == want
    assert 1 <= lib.sip_lqr_residual_multi_columns(h) <= 8
    lib.sip_lqr_plan_destroy(h)
    assert int(lib.sip_lqr_refine_multi_workspace_bytes(None, num_rhs)) == 0
    assert lib.sip_lqr_residual_multi_columns(None) == 0


def test_every_misuse_is_an_invalid_argument(child):
    for entry in ("residual_misuse", "refine_misuse"):
        for what, rc in child[entry].items():
            assert rc == INVALID, (entry, what, rc)
    assert len(child["residual_misuse"]) == 11 and len(child["refine_misuse"]) == 15


def test_no_columns_is_ok_and_launches_nothing(child):
    for what, rc in child["no_columns"].items():
        assert rc == OK, (what, rc)
    assert len(child["no_columns"]) == 4
    assert child["columns"]["NULL"] == 0 and 1 <= child["columns"]["f32 (12,4)"] <= 8 \
        and 1 <= child["columns"]["f64 (12,4)"] <= 8


def test_a_plan_without_a_device_computes_nothing(child):
    assert child["devices_visible"] == 0, "the child process was to see no HIP device"
    for what, rc in child["deviceless"].items():
        assert rc == ERR_HIP, (what, rc)
    assert len(child["deviceless"]) == 5

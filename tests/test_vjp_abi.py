"""sip_lqr_vjp_mats and sip_lqr_vjp without a GPU: the symbols, the header and the argument checks.

The calls are made in a child process that sees no HIP device (HIP_VISIBLE_DEVICES=-1), on a plan that therefore has
none: a misuse returns SIP_LQR_ERR_INVALID_ARGUMENT before any HIP call, and a well-formed call returns
SIP_LQR_ERR_HIP instead of launching on the made-up pointers -- the same on a host with a GPU and on one without."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sip_lqr_vjp_mats", "sip_lqr_vjp")
OK, INVALID, ERR_HIP = 0, -1, -3

CHILD = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
from sip_optimal_control_amd._lib import load_library
lib = load_library()
out = {}
h = ctypes.c_void_p()
assert lib.sip_lqr_plan_create(1, 6, 5, 12, 4, 0, ctypes.byref(h)) == 0
P = ctypes.c_void_p(4096)         # never dereferenced: the plan has no device
N = None
ker = lambda **kw: lib.sip_lqr_vjp_mats(*[kw.get(k, d) for k, d in (
    ("plan", h), ("sol", P), ("adj", P), ("wide", 0), ("status", P), ("grad", P), ("stream", N))])
vjp = lambda **kw: lib.sip_lqr_vjp(*[kw.get(k, d) for k, d in (
    ("plan", h), ("mats", P), ("sol", P), ("gsol", P), ("gains", P), ("ws", P), ("status", P), ("gvecs", P),
    ("gmats", P), ("stream", N))])
out["kernel_misuse"] = {
    "plan": ker(plan=N), "sol": ker(sol=N), "adj": ker(adj=N), "grad": ker(grad=N), "wide=2": ker(wide=2),
    "wide=-1": ker(wide=-1)}
out["vjp_misuse"] = {
    "plan": vjp(plan=N), "mats": vjp(mats=N), "sol": vjp(sol=N), "gsol": vjp(gsol=N), "gains": vjp(gains=N),
    "ws": vjp(ws=N), "gvecs": vjp(gvecs=N)}
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
        "kernel": ker(), "kernel wide, no status": ker(wide=1, status=N), "vjp": vjp(),
        "vjp, no status, no grad_mats": vjp(status=N, gmats=N)}
lib.sip_lqr_plan_destroy(h)
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
    script = tmp_path_factory.mktemp("vjp_abi") / "child.py"
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
    assert _lib._SIGNATURES["sip_lqr_vjp_mats"][0] is ctypes.c_int and len(_lib._SIGNATURES["sip_lqr_vjp_mats"][1]) == 7
    assert _lib._SIGNATURES["sip_lqr_vjp_mats"][1][3] is ctypes.c_int                     # wide
    assert _lib._SIGNATURES["sip_lqr_vjp"][0] is ctypes.c_int and len(_lib._SIGNATURES["sip_lqr_vjp"][1]) == 10


def test_the_unit_is_part_of_the_build():
    import __graft_entry__ as entry
    assert "chain_vjp.hip" in {os.path.basename(src) for _, src, _, _ in entry.hip_units()}
    sources = {os.path.basename(p) for p in entry.hip_sources()}
    assert {"chain_vjp.hip", "chain_vjp.hpp", "vjp_launch.hpp"} <= sources


def test_the_header_declares_them_and_is_plain_c(tmp_path):
    text = open(os.path.join(ROOT, "include", "sip_lqr_amd.h")).read()
    for name in NEW:
        assert name + "(" in text, name
    prose = " ".join(text.replace("\n *", " ").split())
    for stated in ("The gains K | k are not differentiated", "sip_lqr_factor_solve alone does not leave the state",
                   "No second derivative is offered", "gradient over symmetric perturbations",
                   "derivative with respect to the packed parameter"):
        assert stated in prose, stated
    src = tmp_path / "hdr.c"
    src.write_text('#include "sip_lqr_amd.h"\n'
                   "int main(void) {\n"
                   "  int (*k)(const sip_lqr_plan *, const void *, const void *, int, const int32_t *, void *,\n"
                   "           void *) = sip_lqr_vjp_mats;\n"
                   "  int (*v)(const sip_lqr_plan *, const void *, const void *, const void *, void *, void *,\n"
                   "           const int32_t *, void *, void *, void *) = sip_lqr_vjp;\n"
                   "  return k == 0 || v == 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_every_misuse_is_an_invalid_argument(child):
    for entry in ("kernel_misuse", "vjp_misuse"):
        for what, rc in child[entry].items():
            assert rc == INVALID, (entry, what, rc)
    assert len(child["kernel_misuse"]) == 6 and len(child["vjp_misuse"]) == 7


def test_a_plan_without_a_device_computes_nothing(child):
    assert child["devices_visible"] == 0, "the child process was to see no HIP device"
    for what, rc in child["deviceless"].items():
        assert rc == ERR_HIP, (what, rc)
    assert len(child["deviceless"]) == 4

"""sip_lqr_plan_set_wide_controls / sip_lqr_has_wide_controls / sip_kkt_plan_set_chain_wide_controls on host-only plans
(no compute calls), and what the build leaves of the n = 32 matrix-core kernels for 12 and 16 controls: the opt-in takes
effect exactly on FULL-layout plans of the general engine with 9 <= m <= 16, n <= 32 (the exact rows at n = 32,
m in {12, 16} in either dtype, fp64 embeddings otherwise), changes the name and (upwards only) the workspace and nothing
else; the separate sweeps compose with it as on the m <= 8 rows; the two new units define every kernel of their rows
once and sip_lqr_amd defines none."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
F64, F32 = 0, 1
BATCH, T = 4, 5
TAG = {F64: "f64", F32: "f32"}
GENERAL = "tree_generic(chain layout)/"
SUFFIX = " + chain_factor_mt16 + chain_solve_mt16"


def _row(dtype, M):
    return f"chain_factor_solve_mt16<32,{M},mfma16x16x4>/{TAG[dtype]}"


# (dtype, n, m) -> the kernel name after the opt-in
TAKES = {(F64, 32, 16): _row(F64, 16),
         (F32, 32, 12): _row(F32, 12),
         (F64, 17, 9): _row(F64, 12) + " embedding (17,9)",
         (F64, 12, 12): _row(F64, 12) + " embedding (12,12)",
         (F64, 31, 13): _row(F64, 16) + " embedding (31,13)"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_hip()
    from sip_optimal_control_amd._lib import load_library
    return load_library()


def _plan(lib, dtype, n, m):
    h = ctypes.c_void_p()
    assert lib.sip_lqr_plan_create(dtype, BATCH, T, n, m, 0, ctypes.byref(h)) == OK
    return h


def _facts(lib, h):
    return (lib.sip_lqr_kernel_name(h).decode(), int(lib.sip_lqr_workspace_bytes(h)), int(lib.sip_lqr_mats_len(h)),
            int(lib.sip_lqr_vecs_len(h)), int(lib.sip_lqr_gains_len(h)), int(lib.sip_lqr_has_wide_controls(h)),
            int(lib.sip_lqr_solve_multi_workspace_bytes(h, 8)), int(lib.sip_lqr_has_separate_sweeps(h)))


def test_the_three_symbols_exist(lib):
    from sip_optimal_control_amd import _lib
    raw = ctypes.CDLL(_lib.library_path())
    for name in ("sip_lqr_plan_set_wide_controls", "sip_lqr_has_wide_controls", "sip_kkt_plan_set_chain_wide_controls"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name


@pytest.mark.parametrize("dtype,n,m", sorted(TAKES))
def test_opt_in(lib, dtype, n, m):
    h = _plan(lib, dtype, n, m)
    name0, ws0, mats0, vecs0, gains0, has0, cols0, sep0 = before = _facts(lib, h)
    assert name0 == GENERAL + TAG[dtype] and has0 == 0               # find_kernel does not return these rows
    assert lib.sip_lqr_plan_set_wide_controls(h, 0) == OK and _facts(lib, h) == before          # on = 0
    assert lib.sip_lqr_plan_set_wide_controls(h, 1) == OK
    name1, ws1, mats1, vecs1, gains1, has1, cols1, sep1 = after = _facts(lib, h)
    assert name1 == TAKES[(dtype, n, m)] and has1 == 1
    assert (mats1, vecs1, gains1) == (mats0, vecs0, gains0) == (
        (T + 1) * (n * n + n) + T * (n * n + 2 * n * m + m * m), (T + 1) * 2 * n + T * m, T * (m * n + m))
    assert ws1 >= ws0
    # the spill of the sweep (three tiles of W | g per node, in the plan's scalars) is inside it
    assert ws1 >= BATCH * (T + 1) * (3 * 256 + 32) * (8 if dtype == F64 else 4)
    assert cols1 == 0 and sep1 == 0                                   # without separate sweeps: column by column
    assert lib.sip_lqr_plan_set_wide_controls(h, 1) == INVALID       # a second effective opt-in
    assert lib.sip_lqr_plan_set_wide_controls(h, 0) == OK and _facts(lib, h) == after
    lib.sip_lqr_plan_destroy(h)


def _left_alone(lib, dtype, n, m):
    h = _plan(lib, dtype, n, m)
    before = _facts(lib, h)
    assert lib.sip_lqr_plan_set_wide_controls(h, 1) == OK
    assert _facts(lib, h) == before and lib.sip_lqr_has_wide_controls(h) == 0
    assert lib.sip_lqr_plan_set_wide_controls(h, 1) == OK            # nothing took effect: not "a second opt-in"
    assert _facts(lib, h) == before
    lib.sip_lqr_plan_destroy(h)
    return before


@pytest.mark.parametrize("dtype,n,m", [(F64, 12, 4), (F64, 32, 8), (F64, 33, 9), (F64, 20, 17), (F32, 17, 9)])
def test_other_plans_are_left_alone(lib, dtype, n, m):
    _left_alone(lib, dtype, n, m)


@pytest.mark.parametrize("dtype,n,m", [(F64, 32, 16), (F32, 32, 12), (F64, 17, 9), (F64, 12, 4)])
def test_a_plan_forced_onto_the_general_engine_stays_there(lib, monkeypatch, dtype, n, m):
    monkeypatch.setenv("SIP_LQR_VARIANT", "general")
    assert _left_alone(lib, dtype, n, m)[0] == GENERAL + TAG[dtype]


def test_no_embedding_under_pad_0(lib, monkeypatch):
    monkeypatch.setenv("SIP_LQR_PAD", "0")
    assert _left_alone(lib, F64, 17, 9)[0] == GENERAL + "f64"
    h = _plan(lib, F64, 32, 12)                                        # an exact row embeds nothing
    assert lib.sip_lqr_plan_set_wide_controls(h, 1) == OK and lib.sip_lqr_kernel_name(h).decode() == _row(F64, 12)
    lib.sip_lqr_plan_destroy(h)


def test_null_plan(lib):
    assert lib.sip_lqr_plan_set_wide_controls(None, 1) == INVALID
    assert lib.sip_lqr_plan_set_wide_controls(None, 0) == INVALID
    assert lib.sip_lqr_has_wide_controls(None) == 0
    assert lib.sip_kkt_plan_set_chain_wide_controls(None, 1) == INVALID


@pytest.mark.parametrize("dtype,n,m", [(F64, 32, 12), (F32, 32, 16), (F64, 17, 9), (F64, 16, 16)])
def test_separate_sweeps_compose(lib, dtype, n, m):
    h = _plan(lib, dtype, n, m)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK and lib.sip_lqr_has_separate_sweeps(h) == 0  # general engine
    assert lib.sip_lqr_plan_set_wide_controls(h, 1) == OK and lib.sip_lqr_has_wide_controls(h) == 1
    name0, ws0 = lib.sip_lqr_kernel_name(h).decode(), int(lib.sip_lqr_workspace_bytes(h))
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK and lib.sip_lqr_has_separate_sweeps(h) == 1
    name1 = lib.sip_lqr_kernel_name(h).decode()
    assert name1 == name0 + SUFFIX and int(lib.sip_lqr_workspace_bytes(h)) >= ws0
    esize = 8 if dtype == F64 else 4
    for cols in (8, 40):
        want = BATCH * (T + 1) * min(cols, 16) * (32 + m) * esize if n == 32 else 0   # embedded: the column loop
        assert int(lib.sip_lqr_solve_multi_workspace_bytes(h, cols)) == want, (cols, want)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == INVALID
    lib.sip_lqr_plan_destroy(h)


def test_split_on_the_general_engine_is_respected(lib, monkeypatch):
    monkeypatch.setenv("SIP_LQR_SPLIT", "general")
    h = _plan(lib, F64, 32, 16)
    assert lib.sip_lqr_plan_set_wide_controls(h, 1) == OK and lib.sip_lqr_has_wide_controls(h) == 1
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK and lib.sip_lqr_has_separate_sweeps(h) == 0
    assert lib.sip_lqr_kernel_name(h).decode() == _row(F64, 16)
    lib.sip_lqr_plan_destroy(h)


# ---- Newton-KKT (a Newton-KKT plan uploads its tables when it is created: these two need a device) ------------------
def _kkt_plan(lib, parents, children, sd, cd):
    E = len(cd)
    arr = lambda v: (ctypes.c_int * max(1, len(v)))(*v)
    zeros_n, zeros_e = arr([0] * (E + 1)), arr([0] * E)
    h = ctypes.c_void_p()
    assert lib.sip_kkt_plan_create(3, E, 0, arr(parents), arr(children), arr(sd), arr(cd), zeros_n, zeros_n, zeros_e,
                                   zeros_e, 0, ctypes.byref(h)) == OK
    return h


@pytest.mark.gpu
def test_kkt_chain_plan_forwards_the_opt_in(lib):
    E = 4
    h = _kkt_plan(lib, list(range(E)), list(range(1, E + 1)), [17] * (E + 1), [9] * E)
    assert lib.sip_kkt_input_status(h) == 0
    name0, work0 = lib.sip_kkt_kernel_name(h).decode(), int(lib.sip_kkt_work_bytes(h))
    assert name0.startswith("chain:" + GENERAL + "f64")
    assert lib.sip_kkt_plan_set_chain_wide_controls(h, 0) == OK and lib.sip_kkt_kernel_name(h).decode() == name0
    assert lib.sip_kkt_plan_set_chain_wide_controls(h, 1) == OK
    name1 = lib.sip_kkt_kernel_name(h).decode()
    assert name1.startswith("chain:" + _row(F64, 12) + " embedding (17,9)") and name1 != name0
    assert name1[len("chain:" + _row(F64, 12) + " embedding (17,9)"):] == name0[len("chain:" + GENERAL + "f64"):]
    assert int(lib.sip_kkt_work_bytes(h)) >= work0
    assert lib.sip_kkt_plan_set_chain_wide_controls(h, 1) == INVALID          # a second effective call
    assert lib.sip_kkt_plan_set_chain_separate_sweeps(h, 1) == OK
    assert lib.sip_kkt_kernel_name(h).decode().startswith("chain:" + _row(F64, 12) + " embedding (17,9)" + SUFFIX)
    assert lib.sip_kkt_plan_set_theta(h, 2) == OK
    assert lib.sip_kkt_plan_set_chain_wide_controls(h, 0) == INVALID          # after set_theta
    lib.sip_kkt_plan_destroy(h)


@pytest.mark.gpu
def test_kkt_tree_plan_is_left_alone(lib):
    h = _kkt_plan(lib, [0, 0, 1], [1, 2, 3], [17, 17, 17, 17], [9, 9, 9])
    assert lib.sip_kkt_input_status(h) == 0
    before = (lib.sip_kkt_kernel_name(h).decode(), int(lib.sip_kkt_work_bytes(h)))
    assert before[0].startswith("tree:")
    assert lib.sip_kkt_plan_set_chain_wide_controls(h, 1) == OK
    assert (lib.sip_kkt_kernel_name(h).decode(), int(lib.sip_kkt_work_bytes(h))) == before
    assert lib.sip_kkt_plan_set_chain_wide_controls(h, 1) == OK               # nothing took effect
    lib.sip_kkt_plan_destroy(h)


# ---- the listings of the new units --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listings():
    """{unit: text of its device assembly as built} (the build keeps the listing next to each object)."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import __graft_entry__ as entry
    entry.build_hip()
    units = ("chain_mt16_wide", "chain_mt16_wide_solve", "chain_mt16", "chain_mt16_solve", "sip_lqr_amd")
    pattern = os.path.join(ROOT, "build", "obj", "%s", "*-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not all(glob.glob(pattern % u) for u in units) or not entry.listings_current():
        entry.build_hip(force=True)  # library from elsewhere (no build/obj): rebuild with listings
    out = {}
    for u in units:
        (path,) = glob.glob(pattern % u)
        out[u] = open(path).read()
    return out


def _defined(text):
    """[(kernel, scalar, M)] of the mt16 kernels a listing defines, one per .amdhsa_kernel."""
    found = re.findall(r"\.amdhsa_kernel _ZN6sipamd4mt16\d+(chain_\w+?_mt16)I([fd])Li(\d+)EEE", text)
    return sorted((k, s, int(m)) for k, s, m in found)


def test_each_new_unit_defines_every_kernel_of_its_rows_once(listings):
    rows = [(s, M) for s in "df" for M in (12, 16)]
    assert _defined(listings["chain_mt16_wide"]) == sorted(("chain_factor_solve_mt16", s, M) for s, M in rows)
    assert _defined(listings["chain_mt16_wide_solve"]) == sorted(
        (k, s, M) for k in ("chain_factor_mt16", "chain_solve_mt16") for s, M in rows)


def test_the_other_units_define_none_of_them(listings):
    assert _defined(listings["sip_lqr_amd"]) == []
    for unit in ("chain_mt16", "chain_mt16_solve"):
        assert {M for _, _, M in _defined(listings[unit])} == {4, 8}, unit

"""sip_lqr_plan_set_separate_sweeps on plans of the fused fp32 chain kernel (host-only plans, no compute calls), and what
the build leaves of chain_factor_qf32 / chain_solve_cols_qf32 (csrc/chain_qf32_sweeps.hpp).

The opt-in takes effect on a plan on which sip_lqr_plan_set_fused_f32 took effect BEFORE it: the name gains the suffix of
the row, sip_lqr_solve_multi_workspace_bytes becomes batch * 4 * (T + 1) * min(c, 8) * (2 n + m), the workspace stays what
it was.  In the other call order, or with the split calls on the general engine, nothing changes.  The listing of the new
translation unit holds one factor and one solve kernel per row, passes the DPP hazard checker, uses no scratch on the
grid rows and no fp64 arithmetic."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
F32 = 1
BATCH, T = 6, 5
SUFFIX = " + chain_factor_qf32 + chain_solve_qf32"
GRID = [(n, m) for n in (4, 6, 8, 12) for m in (1, 2, 3, 4)]
ROWS = GRID + [(1, 1), (5, 3), (9, 2), (15, 8)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_hip()
    from sip_optimal_control_amd._lib import load_library
    return load_library()


def _plan(lib, n, m):
    h = ctypes.c_void_p()
    assert lib.sip_lqr_plan_create(F32, BATCH, T, n, m, 0, ctypes.byref(h)) == OK
    return h


def _fused(lib, n, m):
    h = _plan(lib, n, m)
    assert lib.sip_lqr_plan_set_fused_f32(h, 1) == OK and lib.sip_lqr_has_fused_f32(h) == 1
    return h


def _facts(lib, h):
    return (lib.sip_lqr_kernel_name(h).decode(), int(lib.sip_lqr_workspace_bytes(h)), int(lib.sip_lqr_mats_len(h)),
            int(lib.sip_lqr_vecs_len(h)), int(lib.sip_lqr_gains_len(h)), int(lib.sip_lqr_has_separate_sweeps(h)),
            tuple(int(lib.sip_lqr_solve_multi_workspace_bytes(h, c)) for c in (1, 3, 8, 20)))


def _column_bytes(n, m, c):
    return BATCH * 4 * (T + 1) * min(c, 8) * (2 * n + m)


def test_fused_f32_then_separate_on_the_c3_shape(lib):
    n, m = 12, 4
    h = _fused(lib, n, m)
    name0, ws0, mats0, vecs0, gains0, has0, cols0 = before = _facts(lib, h)
    assert name0 == "chain_factor_solve_qf32<12,4,direct>/f32" and has0 == 0 and cols0 == (0, 0, 0, 0)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 0) == OK and _facts(lib, h) == before          # on = 0
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK
    name1, ws1, mats1, vecs1, gains1, has1, cols1 = after = _facts(lib, h)
    assert has1 == 1 and lib.sip_lqr_has_fused_f32(h) == 1
    assert name1 == name0 + SUFFIX and name1.startswith(name0)
    assert ws1 == ws0                                  # the spill, the scratch and the gfac region were there already
    assert (mats1, vecs1, gains1) == (mats0, vecs0, gains0)
    for c in (3, 8, 20):
        assert int(lib.sip_lqr_solve_multi_workspace_bytes(h, c)) == _column_bytes(n, m, c), c
    assert cols1 == tuple(_column_bytes(n, m, c) for c in (1, 3, 8, 20))
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == INVALID                                   # a second opt-in
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 0) == OK and _facts(lib, h) == after
    lib.sip_lqr_plan_destroy(h)


@pytest.mark.parametrize("n,m", ROWS)
def test_every_row_takes_the_opt_in(lib, n, m):
    h = _fused(lib, n, m)
    ws0 = int(lib.sip_lqr_workspace_bytes(h))
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK
    assert lib.sip_lqr_has_separate_sweeps(h) == 1
    assert lib.sip_lqr_kernel_name(h).decode() == f"chain_factor_solve_qf32<{n},{m},direct>/f32" + SUFFIX
    assert int(lib.sip_lqr_workspace_bytes(h)) == ws0
    assert int(lib.sip_lqr_solve_multi_workspace_bytes(h, 11)) == _column_bytes(n, m, 11)
    lib.sip_lqr_plan_destroy(h)


def test_the_reverse_order_changes_nothing(lib):
    """separate first (a plan of the general engine: nothing to opt into), then fused_f32: the fused_f32-only plan."""
    ref = _fused(lib, 12, 4)
    want = _facts(lib, ref)
    h = _plan(lib, 12, 4)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK and lib.sip_lqr_has_separate_sweeps(h) == 0
    assert lib.sip_lqr_plan_set_fused_f32(h, 1) == OK and lib.sip_lqr_has_fused_f32(h) == 1
    assert _facts(lib, h) == want and want[5] == 0 and want[6] == (0, 0, 0, 0)
    lib.sip_lqr_plan_destroy(h), lib.sip_lqr_plan_destroy(ref)


def test_split_on_the_general_engine_is_left_alone(lib, monkeypatch):
    monkeypatch.setenv("SIP_LQR_SPLIT", "general")
    h = _fused(lib, 12, 4)
    before = _facts(lib, h)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK and lib.sip_lqr_has_separate_sweeps(h) == 0
    assert _facts(lib, h) == before and before[0] == "chain_factor_solve_qf32<12,4,direct>/f32"
    assert before[6] == (0, 0, 0, 0)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK               # nothing took effect: not "a second opt-in"
    lib.sip_lqr_plan_destroy(h)


def test_an_fp32_plan_without_the_fp32_opt_in_is_left_alone(lib):
    h = _plan(lib, 12, 4)
    before = _facts(lib, h)
    assert lib.sip_lqr_plan_set_separate_sweeps(h, 1) == OK
    assert _facts(lib, h) == before and before[5] == 0 and before[0] == "tree_generic(chain layout)/f32"
    lib.sip_lqr_plan_destroy(h)


# ---- the listing of the new unit --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing():
    """Path of the device assembly of chain_qf32_sweeps.hip as built (the build keeps it next to the object)."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import __graft_entry__ as entry
    entry.build_hip()
    pattern = os.path.join(ROOT, "build", "obj", "chain_qf32_sweeps", "*-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not glob.glob(pattern) or not entry.listings_current():
        entry.build_hip(force=True)  # library from elsewhere (no build/obj): rebuild with listings
    (path,) = glob.glob(pattern)
    return path


def _kernels(path, kernel):
    """{(n, m): (descriptor text, body text)} of the instantiations of `kernel` in a listing."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S*%sILi(\d+)ELi(\d+)E\S*)(.*?)\.end_amdhsa_kernel" % kernel, text, re.S):
        body = text[text.index(m.group(1) + ":"):]
        assert (int(m.group(2)), int(m.group(3))) not in out, m.group(1)
        out[(int(m.group(2)), int(m.group(3)))] = (m.group(4), body[:body.index("s_endpgm")])
    return out


KERNELS = ("chain_factor_qf32", "chain_solve_cols_qf32")


def test_the_unit_defines_one_factor_and_one_solve_kernel_per_row(listing):
    text = open(listing).read()
    assert len(re.findall(r"\.amdhsa_kernel ", text)) == 2 * len(ROWS)
    assert "chain_factor_solve_qf32" not in text          # the fused kernels stay in their own unit
    for kernel in KERNELS:
        assert sorted(_kernels(listing, kernel)) == sorted(ROWS), kernel
    assert all(re.search(r"ILi%dELi%dELi8E" % (n, m), text) for n, m in ROWS)       # 8 columns per solve sweep


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_listing_is_hazard_free(listing, kernel):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_hazards.py"), listing, kernel],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.count("0 hazard(s)") == len(ROWS), out.stdout[-2000:]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_on_the_grid_rows_and_no_fp64_arithmetic(listing, kernel):
    kernels = _kernels(listing, kernel)
    for (n, m), (descriptor, body) in kernels.items():
        assert "v_fmac_f64" not in body and "v_fma_f64" not in body, (kernel, n, m)
        assert "v_fmac_f32_dpp" in body, (kernel, n, m)
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", descriptor).group(1))
        print(f"{kernel}<{n},{m}>: {vgprs} VGPRs")
        if (n, m) in GRID:
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptor), (kernel, n, m)
            assert "scratch_" not in body, (kernel, n, m)

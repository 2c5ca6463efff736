"""sip_lqr_plan_set_fused_f32 / sip_lqr_has_fused_f32 on host-only plans (no compute calls), and what the build leaves
of the fused fp32 chain kernel chain_factor_solve_qf32 (csrc/chain_qf32.hpp): the opt-in takes effect exactly on fp32
full-layout plans of the general engine whose shape has a row, changes the name and (upwards only) the workspace and
nothing else; the kernels' listing passes the DPP hazard checker, holds the fused `v_fmac_f32_dpp` and, on the grid
rows, uses no scratch; the fp64 blocks gen_dpp_blocks.py writes are those it wrote before it learnt the fp32 family."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
F64, F32 = 0, 1
BATCH, T = 6, 5
GENERAL = "tree_generic(chain layout)/f32"
GRID = [(n, m) for n in (4, 6, 8, 12) for m in (1, 2, 3, 4)]
ROWS = GRID + [(1, 1), (5, 3), (9, 2), (15, 8)]
# sha256 of dpp_blocks_gen.hpp as the generator wrote it before the fp32 family existed (6 061 592 bytes)
FP64_BLOCKS_SHA256 = "007fcd9e37771c02e0e8a1b1f08b8f2eefbd19e6a5f69ae3f0483a7d3b7eafdd"


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
            int(lib.sip_lqr_vecs_len(h)), int(lib.sip_lqr_gains_len(h)), int(lib.sip_lqr_has_fused_f32(h)))


def test_the_symbols_exist(lib):
    from sip_optimal_control_amd import _lib
    raw = ctypes.CDLL(_lib.library_path())
    for name in ("sip_lqr_plan_set_fused_f32", "sip_lqr_has_fused_f32"):
        assert hasattr(raw, name), name


def test_opt_in_on_the_c3_shape(lib):
    h = _plan(lib, F32, 12, 4)
    name0, ws0, mats0, vecs0, gains0, has0 = before = _facts(lib, h)
    assert name0 == GENERAL and has0 == 0
    assert lib.sip_lqr_plan_set_fused_f32(h, 0) == OK and _facts(lib, h) == before          # on = 0
    assert lib.sip_lqr_plan_set_fused_f32(h, 1) == OK
    name1, ws1, mats1, vecs1, gains1, has1 = after = _facts(lib, h)
    assert name1 == "chain_factor_solve_qf32<12,4,direct>/f32" and has1 == 1
    assert (mats1, vecs1, gains1) == (mats0, vecs0, gains0)
    assert ws1 >= ws0
    # the spill [S | g | h] of every node, in floats, is inside it
    assert ws1 >= BATCH * (T + 1) * (12 * 12 + 2 * 12) * 4
    assert int(lib.sip_lqr_solve_multi_workspace_bytes(h, 3)) == 0                           # column by column
    assert lib.sip_lqr_plan_set_fused_f32(h, 1) == INVALID                                   # a second opt-in
    assert lib.sip_lqr_plan_set_fused_f32(h, 0) == OK and _facts(lib, h) == after
    lib.sip_lqr_plan_destroy(h)


def test_null_plan(lib):
    assert lib.sip_lqr_plan_set_fused_f32(None, 1) == INVALID
    assert lib.sip_lqr_plan_set_fused_f32(None, 0) == INVALID
    assert lib.sip_lqr_has_fused_f32(None) == 0


@pytest.mark.parametrize("dtype,n,m", [(F64, 12, 4), (F32, 16, 4), (F32, 7, 3), (F32, 32, 8), (F32, 17, 3)])
def test_other_plans_are_left_alone(lib, dtype, n, m):
    assert (n, m) not in ROWS or dtype == F64
    h = _plan(lib, dtype, n, m)
    before = _facts(lib, h)
    assert lib.sip_lqr_plan_set_fused_f32(h, 1) == OK
    assert _facts(lib, h) == before and lib.sip_lqr_has_fused_f32(h) == 0
    assert lib.sip_lqr_plan_set_fused_f32(h, 1) == OK          # nothing took effect: not "a second opt-in"
    lib.sip_lqr_plan_destroy(h)


def test_a_plan_forced_onto_the_general_engine_stays_there(lib, monkeypatch):
    monkeypatch.setenv("SIP_LQR_VARIANT", "general")
    h = _plan(lib, F32, 12, 4)
    before = _facts(lib, h)
    assert before[0] == GENERAL
    assert lib.sip_lqr_plan_set_fused_f32(h, 1) == OK
    assert _facts(lib, h) == before and lib.sip_lqr_has_fused_f32(h) == 0
    lib.sip_lqr_plan_destroy(h)


@pytest.mark.parametrize("n,m", ROWS)
def test_every_row_is_reachable_and_only_by_the_opt_in(lib, n, m):
    h = _plan(lib, F32, n, m)
    assert lib.sip_lqr_kernel_name(h).decode() == GENERAL      # find_kernel does not return these rows
    assert lib.sip_lqr_plan_set_fused_f32(h, 1) == OK
    assert lib.sip_lqr_kernel_name(h).decode() == f"chain_factor_solve_qf32<{n},{m},direct>/f32"
    assert lib.sip_lqr_has_fused_f32(h) == 1
    lib.sip_lqr_plan_destroy(h)


# ---- the listing of the new unit --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing():
    """Path of the device assembly of chain_qf32.hip as built (the build keeps it next to the object)."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import glob
    import __graft_entry__ as entry
    entry.build_hip()
    pattern = os.path.join(ROOT, "build", "obj", "chain_qf32", "*-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not glob.glob(pattern) or not entry.listings_current():
        entry.build_hip(force=True)  # library from elsewhere (no build/obj): rebuild with listings
    (path,) = glob.glob(pattern)
    return path


def _kernels(path):
    """{(n, m): (descriptor text, body text)} of the chain_factor_solve_qf32 instantiations in a listing."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S*chain_factor_solve_qf32ILi(\d+)ELi(\d+)E\S*)(.*?)\.end_amdhsa_kernel", text, re.S):
        body = text[text.index(m.group(1) + ":"):]
        out[(int(m.group(2)), int(m.group(3)))] = (m.group(4), body[:body.index("s_endpgm")])
    return out


def test_the_unit_defines_every_row_once(listing):
    assert sorted(_kernels(listing)) == sorted(ROWS)


def test_the_listing_is_hazard_free(listing):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_hazards.py"), listing,
                          "chain_factor_solve_qf32"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.count("0 hazard(s)") == len(ROWS), out.stdout[-2000:]


def test_the_cross_lane_arithmetic_is_fused(listing):
    """Every product is `v_fmac_f32_dpp`; the only unfused broadcasts are the pivots of the factorisations (N + M per
    stage and N for the terminal node: one v_mov_b32_dpp each)."""
    for (n, m), (_, body) in _kernels(listing).items():
        fused, moved = body.count("v_fmac_f32_dpp"), body.count("v_mov_b32_dpp")
        assert fused >= 4 * n * n, (n, m, fused)                # more than the four n x n products of a stage
        assert moved <= 2 * (2 * n + m), (n, m, moved)             # (twice: room for a peeled loop trip)
        assert "v_fmac_f64" not in body and "v_fma_f64" not in body, (n, m)


@pytest.mark.parametrize("n,m", GRID)
def test_the_grid_rows_use_no_scratch(listing, n, m):
    descriptor, body = _kernels(listing)[(n, m)]
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", descriptor), (n, m)
    assert "scratch_" not in body


# ---- the generator ----------------------------------------------------------------------------------------------------
def test_the_fp64_blocks_are_what_the_generator_wrote_before(tmp_path):
    gen = os.path.join(ROOT, "sip_optimal_control_amd", "csrc", "gen_dpp_blocks.py")
    f64, f32 = tmp_path / "f64.hpp", tmp_path / "f32.hpp"
    subprocess.check_call([sys.executable, gen, str(f64)])
    subprocess.check_call([sys.executable, gen, str(f32), "f32"])
    assert hashlib.sha256(f64.read_bytes()).hexdigest() == FP64_BLOCKS_SHA256
    text = f32.read_text()
    assert "v_fmac_f32_dpp" in text and "f64" not in text and "double" not in text
    assert "namespace qf32 {" in text
    for block in ("rank1", "spread", "dotv", "spreadv", "rank1x", "spreadx"):
        assert re.search(r"void %s\(float \*" % block, text), block
    assert text.count('asm volatile("s_nop 1\\n\\tv_fmac_f32_dpp') > 0      # the WAIT convention

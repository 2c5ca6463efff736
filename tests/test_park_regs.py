"""The accumulation-register check of the parked chain kernels (tools/check_park_regs.py): what it flags on
hand-written listings, and that the kernels of the library as built pass it, use no scratch and stay inside the 512
registers a wavefront has when it owns its SIMD."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("park", os.path.join(ROOT, "tools", "check_park_regs.py"))
park = importlib.util.module_from_spec(spec)
spec.loader.exec_module(park)

DESC = "\t.amdhsa_private_segment_fixed_size 0\n\t.amdhsa_next_free_vgpr 300\n\t.amdhsa_accum_offset 256\n"


def _block(first, n=13, op="v_accvgpr_write_b32 a[{r}], v1"):
    body = "\n".join("\t" + op.format(r="%d+%d" % (first, k) if k else "%d" % first) for k in range(n))
    return "\t; sip_park_begin\n" + body + "\n\t; sip_park_end"


def _check(body, desc=DESC):
    return park.check_kernel("k", body.split("\n"), desc)


def test_register_names():
    assert park.agprs("\tv_accvgpr_write_b32 a7, v3") == {7}
    assert park.agprs("\tv_accvgpr_read_b32 v3, a[0xb6+2]") == {0xb6 + 2}
    assert park.agprs("\tds_write_b128 v1, a[4:7] offset:16") == {4, 5, 6, 7}
    assert park.agprs("\tv_mov_b32 v2, 0xa0 ; a9 in a comment") == set()
    assert park.agprs("\ts_mov_b32 s0, exec_lo") == set()


def test_accepts_banks_below_the_compilers_registers():
    body = _block(0) + "\n" + _block(13, op="v_accvgpr_read_b32 v1, a[{r}]") + "\n\tv_accvgpr_write_b32 a26, v9\n\tv_accvgpr_read_b32 v9, a26"
    problems, summary = _check(body)
    assert problems == [] and summary["keep"] == 2 and summary["own"] == 1 and summary["own_lowest"] == 26


def test_flags_a_bank_register_outside_the_markers():
    problems, _ = _check(_block(0) + "\n\tv_accvgpr_write_b32 a5, v9")
    assert len(problems) == 1 and "outside the markers" in problems[0]
    problems, _ = _check(_block(0) + "\n\tds_write_b64 v1, a[12:13]")  # a pair that reaches into the bank
    assert len(problems) == 1


def test_flags_partial_banks_scratch_and_totals():
    assert any("whole banks" in p for p in _check(_block(0, n=12))[0])
    assert any("whole banks" in p for p in _check(_block(13))[0])
    assert any("scratch" in p for p in _check(_block(0), DESC.replace("fixed_size 0", "fixed_size 16"))[0])
    assert any("totals" in p for p in _check(_block(0), DESC.replace("vgpr 300", "vgpr 520"))[0])
    assert any("totals" in p for p in _check(_block(0), DESC.replace("vgpr 300", "vgpr 260"))[0])  # 256 + 13 > 260
    assert any("unbalanced" in p for p in _check("\t; sip_park_begin\n\tv_accvgpr_write_b32 a0, v1")[0])


def test_kernels_without_markers_are_not_parked():
    assert _check("\tv_accvgpr_write_b32 a3, v1\n\tv_accvgpr_read_b32 v1, a3") == ([], None)


def test_shipped_parked_kernels_keep_their_banks():
    """The two parked kernels of the library as built -- (12, 4), full and symmetric-packed -- name their banks only
    between the markers, spill nothing to scratch, fit one wavefront's 512 registers, and still pass the DPP-hazard
    and counted-wait checker; KEEP in the listing is the KEEP of chain_qw16.hpp."""
    import subprocess
    import sys
    from test_tools import _shipped_listings
    entry, by_unit = _shipped_listings()
    header = open(os.path.join(ROOT, "sip_optimal_control_amd", "csrc", "chain_qw16.hpp")).read()
    m = re.search(r"static constexpr int KEEP = SYM \? (\d+) : (\d+);", header)
    want = {"sym": int(m.group(1)), "full": int(m.group(2))}
    found = {}
    for unit, path in by_unit.items():
        if not unit.startswith("qw16_kernels_"):
            continue
        text = open(path).read()
        if "sip_park_begin" not in text:
            continue
        for name, body, desc in park.kernels(text):
            problems, summary = park.check_kernel(name, body, desc)
            if summary is None:
                assert problems == []
                continue
            assert problems == [], (name, problems)
            assert "chain_factor_solve_qw16ILi12ELi4ELb1ELb1ELb0E" in name, name  # <12, 4, staged, packed, not split, ...>
            found["sym" if "ILi12ELi4ELb1ELb1ELb0ELb1ELb1E" in name else "full"] = summary["keep"]
            assert summary["next_free_vgpr"] <= 512
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_hazards.py"), path,
                              "chain_factor_solve_qw16"], capture_output=True, text=True)
        assert out.returncode == 0, path + "\n" + out.stdout[-2000:]
    assert found == want, (found, want)

"""The derived sizes and LDS partitions of the Newton-KKT chain kernels, stated once (chain_kkt_derive and the
*_lds descriptions of csrc/kkt_chain_kernels.hpp, kkt_theta_chain_kernels.hpp) and used by the kernels for their
pointers and by the host for the bytes of every launch: tests/cpp/test_kkt_lds.cpp checks them on the host -- the
family instantiations' dimensions by static_assert, the regions' order and alignment, and the bytes of every launch
against values worked by hand from the sums the host code used to spell out."""
import subprocess


def test_kkt_lds_descriptions():
    import __graft_entry__ as entry
    exe = entry.build_kkt_lds_test()
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert "8 rows, 0 failures" in proc.stdout and "[FAILED]" not in proc.stdout

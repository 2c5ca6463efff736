"""The drop-in `sip::optimal_control::LQR` with the split fused sweeps on (set_split_fused / SIP_LQR_DROPIN_SPLIT=1):
tests/cpp/test_dropin_split.cpp runs the reference's tests (tests/cpp/test_dropin.cpp) with the switch on, then checks
that solve() uses the factorization of factor time (a Q changed in between does not reach it; the default, which
refactors, sees it) and that one factor serves several right-hand sides."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_cpp_dropin_split_suite():
    import __graft_entry__ as entry
    entry.build_hip()
    exe = entry.build_dropin_split_test()
    env = dict(os.environ)
    for k in ("SIP_LQR_DROPIN_GENERAL", "SIP_LQR_DROPIN_SPLIT", "SIP_LQR_DROPIN_FUSED"):
        env.pop(k, None)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.count("[  OK  ]") >= 21 and "[FAILED]" not in proc.stdout
    assert ", 0 failures" in proc.stdout and "split: " in proc.stdout

#!/usr/bin/env python3
"""What libsip_lqr_amd.so is linked from (__graft_entry__.hip_units), for the scripts that build a variant of it:
    tools/lib_objects.py [source ...]   the objects of the last full build, without the units of the named sources
                                        (sip_kkt_amd, qw16_kernels ...: the script compiles those itself)
    tools/lib_objects.py --sources      the source files, each once"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

units = entry.hip_units()
if sys.argv[1:] == ["--sources"]:
    print(" ".join(dict.fromkeys(os.path.relpath(src, ROOT) for _, src, _, _ in units)))
else:
    stems = {os.path.basename(src)[:-len(".hip")] for _, src, _, _ in units}
    assert set(sys.argv[1:]) <= stems, "no such source: %s" % sorted(set(sys.argv[1:]) - stems)
    print(" ".join(os.path.relpath(obj, ROOT) for obj, src, _, _ in units
                   if os.path.basename(src)[:-len(".hip")] not in sys.argv[1:]))

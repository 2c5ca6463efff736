#!/bin/bash
# Diagnostic (stamped) build of the HIP library -> sip_optimal_control_amd/lib/diag/libsip_lqr_amd.so
# (of the fused chain kernels, the core set in one translation unit: gen_qw16_kernels.py --shapes core; the
# Newton-KKT chain kernels in one unit too: kkt_chain_kernels.hip without SIP_KKT_CHAIN_N)
set -e
cd "$(dirname "$0")/.."
mkdir -p sip_optimal_control_amd/lib/diag build/ab
python3 sip_optimal_control_amd/csrc/gen_qw16_kernels.py build/ab/diag_manifest.hpp --shapes core
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -mllvm -amdgpu-mfma-vgpr-form=1 -DSIP_LQR_STAMPS \
  -DSIP_QW16_MANIFEST="\"$PWD/build/ab/diag_manifest.hpp\"" -DSIP_QW16_SLICE=0 \
  $(python3 tools/lib_objects.py --sources) -o sip_optimal_control_amd/lib/diag/libsip_lqr_amd.so
echo sip_optimal_control_amd/lib/diag/libsip_lqr_amd.so

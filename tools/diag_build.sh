#!/bin/bash
# Diagnostic (stamped) build of the HIP library -> sip_optimal_control_amd/lib/diag/libsip_lqr_amd.so
# (of the fused chain kernels, the core set in one translation unit: gen_qw16_kernels.py --shapes core)
set -e
cd "$(dirname "$0")/.."
mkdir -p sip_optimal_control_amd/lib/diag build/ab
python3 sip_optimal_control_amd/csrc/gen_qw16_kernels.py build/ab/diag_manifest.hpp --shapes core
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -mllvm -amdgpu-mfma-vgpr-form=1 -DSIP_LQR_STAMPS \
  -DSIP_QW16_MANIFEST="\"$PWD/build/ab/diag_manifest.hpp\"" -DSIP_QW16_SLICE=0 \
  sip_optimal_control_amd/csrc/sip_lqr_amd.hip sip_optimal_control_amd/csrc/sip_lqr_tree.hip sip_optimal_control_amd/csrc/sip_kkt_amd.hip sip_optimal_control_amd/csrc/tree_qw16.hip sip_optimal_control_amd/csrc/chain_mt16.hip sip_optimal_control_amd/csrc/qw16_kernels.hip -o sip_optimal_control_amd/lib/diag/libsip_lqr_amd.so
echo sip_optimal_control_amd/lib/diag/libsip_lqr_amd.so

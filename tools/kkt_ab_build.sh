#!/bin/bash
# A/B library with another build of the Newton-KKT chain kernels: tools/kkt_ab_build.sh <name> [extra -D flags...]
# (-DSIP_KKT_*_WAVES=..., -DSIP_KKT_APPLY_FULL_STAGE, -DSIP_KKT_STAMPS: all of them switches of the kernel headers)
# -> sip_optimal_control_amd/lib/diag/libkkt_<name>.so
# kkt_chain_kernels.hip is compiled as ONE unit with the flags; the other objects, sip_kkt_amd.o among them (it
# holds no chain kernel, so the flags mean nothing to it), come from the last full build (tools/lib_objects.py).
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
mkdir -p build/ab sip_optimal_control_amd/lib/diag
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-mfma-vgpr-form=1 "$@" -c sip_optimal_control_amd/csrc/kkt_chain_kernels.hip -o build/ab/kkt_$NAME.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC build/ab/kkt_$NAME.o $(python3 tools/lib_objects.py kkt_chain_kernels) build/obj/build_stamp.o -o sip_optimal_control_amd/lib/diag/libkkt_$NAME.so
echo sip_optimal_control_amd/lib/diag/libkkt_$NAME.so

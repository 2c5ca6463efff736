#!/bin/bash
# build a tree-only variant lib: tools... name flags
set -e
cd "$(dirname "$0")/.."
mkdir -p build/ab sip_optimal_control_amd/lib/diag
NAME=$1; shift
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-mfma-vgpr-form=1 "$@" -save-temps=obj -c sip_optimal_control_amd/csrc/tree_qw16.hip -o build/ab/tree_$NAME.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC build/ab/tree_$NAME.o $(python3 tools/lib_objects.py tree_qw16) build/obj/build_stamp.o -o sip_optimal_control_amd/lib/diag/libtree_$NAME.so
echo sip_optimal_control_amd/lib/diag/libtree_$NAME.so

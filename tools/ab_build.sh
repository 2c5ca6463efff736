#!/bin/bash
# Quick A/B library: tools/ab_build.sh <name> [extra -D flags...]
# -> sip_optimal_control_amd/lib/diag/lib<name>.so ; compare with tools/ab.sh on the GPU box.
# Only the host code and one slice of the fused chain kernels are compiled, the slice with the C3 kernel (12, 4)
# alone (SHAPES=14x8,15x4 ... or SHAPES=core for others: gen_qw16_kernels.py --shapes); the tree / KKT / n = 32
# objects come from the last full build (build/obj, listed by tools/lib_objects.py), so run `python -c "import __graft_entry__ as g; g.build()"` first.
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
mkdir -p sip_optimal_control_amd/lib/diag build/ab
python3 sip_optimal_control_amd/csrc/gen_qw16_kernels.py build/ab/${NAME}_manifest.hpp --shapes "${SHAPES:-12x4}"
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-mfma-vgpr-form=1 "-DSIP_QW16_MANIFEST=\"$PWD/build/ab/${NAME}_manifest.hpp\"")
/opt/rocm/bin/hipcc "${FLAGS[@]}" "$@" -c sip_optimal_control_amd/csrc/sip_lqr_amd.hip -o build/ab/${NAME}_host.o
/opt/rocm/bin/hipcc "${FLAGS[@]}" "$@" -DSIP_QW16_SLICE=0 -save-temps=obj -c sip_optimal_control_amd/csrc/qw16_kernels.hip -o build/ab/$NAME.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC build/ab/${NAME}_host.o build/ab/$NAME.o \
  $(python3 tools/lib_objects.py sip_lqr_amd qw16_kernels) -o sip_optimal_control_amd/lib/diag/lib$NAME.so
echo sip_optimal_control_amd/lib/diag/lib$NAME.so

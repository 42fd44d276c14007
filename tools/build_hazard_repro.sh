#!/bin/bash
# Builds tools/_build/hazard_repro from tools/hazard_repro.hip and the PRODUCT's own kernel sources as shipped (same flags as
# ocrs_amd/build.py).  hipcc cross-compiles for gfx950 without a GPU; the binary travels to the GPU box with the tree.
set -e
cd "$(dirname "$0")/.."
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-function -Wno-pass-failed"
C=ocrs_amd/csrc
mkdir -p tools/_build
for f in kernels_nn kernels_rec kernels_lines; do
  [ tools/_build/$f.o -nt $C/$f.hip ] || /opt/rocm/bin/hipcc $FLAGS -c $C/$f.hip -o tools/_build/$f.o &
done
/opt/rocm/bin/hipcc $FLAGS -x hip -c $C/common.cpp -o tools/_build/common.o &
/opt/rocm/bin/hipcc $FLAGS -c tools/hazard_repro.hip -o tools/_build/hazard_repro.o &
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -o tools/_build/hazard_repro tools/_build/hazard_repro.o tools/_build/kernels_lines.o \
    tools/_build/kernels_nn.o tools/_build/kernels_rec.o tools/_build/common.o -ldl -lpthread
echo built tools/_build/hazard_repro

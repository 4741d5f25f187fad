#!/bin/bash
# Developer tool: builds a variant of the library with extra compiler flags (kernel experiments).
# -DNLPS_DEV=1: the only build that reads the environment switches (NLPS_LAZY_NODAL, NLPS_ADAPTIVE_RESORT).
# What a developer build can still set (measurement instruments, not alternative products):
#   -DNLPS_PHASE_TIMING=1   per-phase wave-cycle sums of the tile kernels (tools/kbench.py --phases)
#   -DNLPS_ABL_ATOM=1       the window scatters issue no LDS atomic (WRONG results by design)
#   -DNLPS_ABL_GATHER=1     the gathers read a register constant instead of their window (WRONG results by design)
# Tuning numbers (waves per SIMD, workgroup sizes, unroll factors) are plain constants beside the code they tune: edit them.
#   tools/build_variant.sh NAME [-DNLPS_...=v ...]   ->  build/exp/lib_NAME.so   (run with NLPS_GPU_LIB=... tools/kbench.py)
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build/exp
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -shared -std=c++17 -ffp-contract=off -munsafe-fp-atomics \
  -fvisibility=hidden -fvisibility-inlines-hidden -DNLPS_DEV=1 "$@" -o build/exp/lib_$name.so \
  nl-partsol_amd/csrc/nlps_gpu.hip nl-partsol_amd/csrc/nlps_io.cpp
echo build/exp/lib_$name.so

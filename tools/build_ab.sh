#!/bin/bash
# Experiment build for kernel A/B runs (never used by tests, bench or the driver): only the config-3
# shape (W 256, multires 7) of the render / density kernels, extra flags (-DFLAG, -mllvm ...) from the command
# line for the render units; every other unit as build.py compiles it.
#   bash tools/build_ab.sh NAME [-DFLAG ...]   ->  tools/ab/lib_NAME.so   (run with ANERF_LIB_PATH=...)
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/ab
NAME=$1; shift
C=a-nerf_amd/csrc
F="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wno-unused-result"
OTHER=""
for u in gemm iso mesh raster simplify step eval sequence posescore; do  # (every other unit of build.py's SRC)
  o=tools/ab/$u.o
  [ -f $o ] && [ $o -nt $C/anerf_$u.hip ] && [ $o -nt $C/anerf_scan.hpp ] && [ $o -nt $C/anerf_iso_table.inc ] && [ $o -nt include/anerf.h ] ||
    /opt/rocm/bin/hipcc $F -c -o $o $C/anerf_$u.hip
  OTHER="$OTHER $o"
done
# (the fp16 instances' unit with build.py's flag for it, RENDER_F16_FLAGS)
/opt/rocm/bin/hipcc $F -DANERF_AB_FAST "$@" -c -o tools/ab/render_$NAME.o $C/anerf_render.hip &
/opt/rocm/bin/hipcc $F -mllvm -amdgpu-mfma-vgpr-form -DANERF_AB_FAST "$@" -c -o tools/ab/render_f16_$NAME.o $C/anerf_render_f16.hip
wait %1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/ab/lib_$NAME.so tools/ab/render_$NAME.o tools/ab/render_f16_$NAME.o $OTHER
rm -f tools/ab/render_$NAME.o tools/ab/render_f16_$NAME.o

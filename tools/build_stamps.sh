#!/bin/bash
# Diagnostic build with in-kernel s_memtime stamps (tools/stamps.py); never used by tests or bench.  The units and
# their flags as build.py compiles them (the fp16 instances' unit with RENDER_F16_FLAGS), plus -DANERF_STAMPS.
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/ab
C=a-nerf_amd/csrc
F="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wno-unused-result -DANERF_STAMPS"
/opt/rocm/bin/hipcc $F -c -o tools/ab/stamps_render.o $C/anerf_render.hip &
/opt/rocm/bin/hipcc $F -mllvm -amdgpu-mfma-vgpr-form -c -o tools/ab/stamps_render_f16.o $C/anerf_render_f16.hip
wait %1
/opt/rocm/bin/hipcc $F -shared -o tools/ab/libanerf_hip_stamps.so tools/ab/stamps_render.o tools/ab/stamps_render_f16.o \
    $C/anerf_gemm.hip $C/anerf_iso.hip $C/anerf_mesh.hip $C/anerf_raster.hip $C/anerf_simplify.hip
rm -f tools/ab/stamps_render.o tools/ab/stamps_render_f16.o

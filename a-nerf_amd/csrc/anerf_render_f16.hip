// anerf_render_f16.hip — the fp16 instances (ANERF_PREC_FP16X3 / FP16X4) of render_kernel, density_kernel and
// radiance_kernel: the same headers as anerf_render.hip, compiled with MFMA results in VGPRs (build.py
// RENDER_F16_FLAGS, -mllvm -amdgpu-mfma-vgpr-form).
//
// Why a unit of its own: between two fp16 hidden layers the next layer's power-of-two scale is the maximum of all of
// a sample's outputs (h3_scale, anerf_mlp.hpp), 64 v_max3_i32 per lane on the accumulators while the MFMA pipe is
// empty, and relu, bias and the fp16 split read and write them too.  With the accumulators in AGPRs, which VALU
// instructions cannot address, that stretch began with 128 v_accvgpr_read_b32 and the kernel kept 68 B per lane of
// scratch; in VGPR form both are gone.  The other precision modes and the training GEMMs
// (anerf_gemm.hip, dW strips held in AGPRs on purpose) keep the default form: the option acts on a whole unit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "../../include/anerf.h"
#include "anerf_device.hpp"

using namespace anerf;

#include "anerf_types.hpp"
#include "anerf_mlp.hpp"
#include "anerf_stages.hpp"
#include "anerf_kernels.hpp"

ANERF_F16_INSTANCES()

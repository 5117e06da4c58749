"""Static checks of the built library's device code for the fp16 render kernels, render_kernel<256,7,4> (fp16x4) and
<256,7,3> (fp16x3): code-object metadata and instruction text, read with tools/isa_diff.py's parsing.  No GPU.

What is held: between two fp16 hidden layers the VALU reads every accumulator (the next layer's scale is
their maximum) while the MFMA pipe is empty, so the accumulators must be where the VALU can read them:
  * no scratch: private_segment_fixed_size 0 and no scratch_ instruction;
  * at most 512 registers per lane.  `.vgpr_count` of a gfx950 code object is the whole unified allocation, the
    AGPRs (`.agpr_count`) included;
  * no v_accvgpr_read_b32 in the 600 instructions before a hidden layer's MFMA run (the drain).  A hidden layer of
    width 256 is one straight-line stretch of 128 groups of P MFMAs (v_mfma_f32_32x32x16_f16): 512 for fp16x4,
    384 for fp16x3; the layer loop is not unrolled, so each kernel holds one such run.

Measured on the build of this change (MFMA results in VGPRs, anerf_render_f16.hip; the half-wave reductions in the
VALU; the bias rows' wave half formed per layer by one v_mbcnt_lo_u32_b32): scratch 0, 457 / 456 registers and no
v_accvgpr_read_b32 before the run, where the build before it had 68 B of scratch, 512 registers and 128 reads (one per
accumulator register).  Inside the run the relu'd inputs h[4..7] are still parked in AGPRs (64 + 64 copies per
layer), which these checks do not cover.
"""
import importlib
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_diff  # noqa: E402

_lib = importlib.import_module("a-nerf_amd._lib")

MFMA = "v_mfma_f32_32x32x16_f16"
GROUPS = 128  # 2 * RBO * RBI groups of a 256 x 256 layer (mlp_layer_h3)
WINDOW = 600
BRANCH = re.compile(r"^(s_cbranch|s_branch|s_endpgm|s_setpc|s_swappc)")


@pytest.fixture(scope="module")
def units():
    assert os.path.exists(_lib.LIB_PATH), "libanerf_hip.so is not built (python -m a-nerf_amd.build)"
    return isa_diff.load(_lib.LIB_PATH)


def _kernel(units, P):
    found = [(lines, res[name]) for funcs, res in units for name, lines in funcs.items()
             if re.search(rf"render_kernelILi256ELi7ELi{P}EE", name) and name in res]
    assert len(found) == 1, f"render_kernel<256,7,{P}>: {len(found)} definitions in the library"
    return found[0]


def _hidden_runs(lines, P):
    """Index of the first MFMA of every straight-line stretch that holds a whole hidden layer's MFMAs."""
    out, first, n = [], None, 0
    for i, l in enumerate(lines + ["s_endpgm"]):
        if l.startswith(MFMA):
            first, n = (i if first is None else first), n + 1
        elif BRANCH.match(l):
            if n >= GROUPS * P:
                out.append(first)
            first, n = None, 0
    return out


@pytest.mark.parametrize("P", [4, 3])
def test_fp16_render_kernel_registers_and_scratch(units, P):
    lines, res = _kernel(units, P)
    assert int(res[".private_segment_fixed_size"]) == 0
    assert not [l for l in lines if l.startswith("scratch_")]
    assert int(res[".agpr_count"]) <= int(res[".vgpr_count"]) <= 512


@pytest.mark.parametrize("P", [4, 3])
def test_fp16_hidden_layer_drain_reads_no_agpr(units, P):
    lines, _ = _kernel(units, P)
    runs = _hidden_runs(lines, P)
    assert runs, f"no straight-line run of {GROUPS * P} {MFMA}"
    for first in runs:
        reads = [l for l in lines[max(0, first - WINDOW):first] if l.startswith("v_accvgpr_read_b32")]
        print(f"render_kernel<256,7,{P}>: {len(reads)} v_accvgpr_read_b32 in the {WINDOW} instructions before the "
              f"hidden layer's first MFMA (instruction {first})")
        assert not reads, reads

"""CPU: the C-ABI library loads and exports every entry point include/anerf.h declares.

No compute calls are made (no GPU here); argument validation paths that return before any
HIP call are exercised.
"""
import ctypes
import importlib
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HEADER = os.path.join(os.path.dirname(HERE), "include", "anerf.h")
_lib = importlib.import_module("a-nerf_amd._lib")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w]+\s*\**\s*(anerf_\w+)\s*\(", src, flags=re.M)))


def test_header_declares_expected_entry_points():
    fns = header_functions()
    for f in ("anerf_model_create", "anerf_render_rays", "anerf_gen_rays", "anerf_near_far", "anerf_compose",
              "anerf_encode_points", "anerf_workspace_size", "anerf_last_error", "anerf_abi_version",
              "anerf_density_points", "anerf_density_grid", "anerf_gen_rays_box", "anerf_compose_box",
              "anerf_pose_kinematics", "anerf_kp_boxes", "anerf_train_samples", "anerf_train_encode",
              "anerf_train_encode_backward", "anerf_train_composite", "anerf_train_composite_backward",
              "anerf_train_importance", "anerf_pose_kinematics_backward", "anerf_ray_batch", "anerf_gather_rows",
              "anerf_mlp_split_bytes", "anerf_mlp_split_weights", "anerf_mlp_split_weights_batch", "anerf_mlp_gemm", "anerf_mlp_wgrad_workspace",
              "anerf_mlp_wgrad", "anerf_train_view_mix", "anerf_train_view_mix_backward",
              "anerf_train_view_factor", "anerf_train_view_factor_backward", "anerf_train_view_factor_workspace"):
        assert f in fns


def test_library_exports_every_header_symbol():
    lib = _lib.load()
    for f in header_functions():
        assert hasattr(lib, f), f"libanerf_hip.so does not export {f}"
    assert set(header_functions()) == set(_lib.SIGNATURES), "ctypes signatures out of sync with anerf.h"


def test_abi_version():
    src = open(HEADER).read()
    ver = int(re.search(r"#define ANERF_ABI_VERSION (\d+)", src).group(1))
    assert _lib.load().anerf_abi_version() == ver


def test_invalid_model_desc_is_rejected_with_message():
    lib = _lib.load()
    d = _lib.ModelDesc()
    d.n_joints, d.net_depth, d.net_width, d.multires, d.multires_views = 24, 8, 100, 7, 4
    h = ctypes.c_void_p()
    rc = lib.anerf_model_create(ctypes.byref(d), None, None, None, 0, ctypes.byref(h))
    assert rc == -1
    assert b"net_width" in lib.anerf_last_error()
    assert not h.value


def test_null_model_render_is_rejected():
    lib = _lib.load()
    rc = lib.anerf_render_rays(None, None, 11, 1, None, None, 1, None, None, 64, 0, 4096, 0, None, None, None,
                               None, None, None, None, None, None, None, 0, None)
    assert rc == -1
    assert b"model" in lib.anerf_last_error()


def test_library_reads_no_experiment_switches_from_the_environment():
    """The fp16 operand range, the bone-direction part's precision and the two-launch schedule are
    compile-time constants of the shipped library (experiment builds pass -D flags, tools/build_ab.sh):
    none of the switch names is in the binary, so no environment variable can change a render."""
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    for name in (b"ANERF_H3_TARGET", b"ANERF_UX6", b"ANERF_FUSED_PASSES"):
        assert name not in blob, name


def test_compile_time_switches_are_the_declared_ones():
    """Every ANERF_* macro that a preprocessor conditional of the kernel sources tests is declared here:
    the switches of the maintained diagnostic and A/B tools (DESIGN.md lists the tool each serves).
    Experiment scaffolding does not stay in the product sources: build it from a patched copy."""
    allowed = {"ANERF_STAMPS", "ANERF_ASM_MARKS", "ANERF_AB_FAST", "ANERF_H3_TARGET"}
    csrc = os.path.join(REPO, "a-nerf_amd", "csrc")
    found = set()
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name)) as f:
            src = f.read().replace("\\\n", " ")
        for cond in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", src, flags=re.M):
            found |= set(re.findall(r"\bANERF_[A-Z0-9_]+", cond))
    assert found == allowed, sorted(found ^ allowed)


def test_build_discards_a_library_whose_sources_moved(tmp_path, monkeypatch):
    """build.py keeps only a build whose sources did not change while hipcc ran (a header edited between
    the offload passes gives host and device different struct layouts) and renames it into place whole."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("anerf_build", os.path.join(REPO, "a-nerf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    out = str(tmp_path / "libx.so")
    monkeypatch.setattr(b, "OUT", out)
    monkeypatch.setattr(b, "STAMP", out + ".stamp")
    cc = tmp_path / "cc.sh"  # (a stand-in compiler: creates the file after -o)
    cc.write_text('#!/bin/sh\nwhile [ $# -gt 0 ]; do [ "$1" = -o ] && touch "$2"; shift; done\n')
    cc.chmod(0o755)
    monkeypatch.setattr(b, "HIPCC", str(cc))
    monkeypatch.setattr(b, "FLAGS", [])
    monkeypatch.setattr(b, "SRC", [])
    monkeypatch.setattr(b, "OBJS", str(tmp_path / "objs"))
    hashes = iter(["a", "b"])
    monkeypatch.setattr(b, "source_hash", lambda: next(hashes))
    with pytest.raises(RuntimeError, match="sources changed"):
        b.build(force=True, verbose=False)
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    monkeypatch.setattr(b, "source_hash", lambda: "c")
    assert b.build(force=True, verbose=False) == out and os.path.exists(out)
    assert open(out + ".stamp").read().strip() == "c"


def test_view_mix_rejects_bad_shapes():
    """anerf_train_view_mix validates before any HIP call (anerf.h: width % 4 == 0, ld >= NJ, the LDS plan)."""
    lib = _lib.load()
    assert lib.anerf_train_view_mix(1, 1, 24, 130, 1, 24, 16, 16, None) == -1
    assert lib.anerf_train_view_mix(1, 1, 103, 128, 1, 103, 16, 16, None) == -1  # (G + windows over 64 KB of LDS)
    assert lib.anerf_train_view_mix(1, 1, 24, 128, 1, 20, 16, 16, None) == -1
    assert b"anerf_train_view_mix" in lib.anerf_last_error()
    assert lib.anerf_train_view_mix_backward(1, 1, 24, 128, 1, 24, 16, 16, None, 24, 16, None) == -1


def test_view_windows_flag_validation():
    """ANERF_ENC_VIEW_WINDOWS (ABI 16) needs cutoff_viewdir and cutoff_inputs and no staged encoder; anerf_model_create
    rejects the rest before any HIP call."""
    lib = _lib.load()

    def create(**kw):
        d = _lib.ModelDesc()
        d.n_joints, d.net_depth, d.net_width, d.multires, d.multires_views = 24, 8, 256, 7, 4
        d.skip, d.use_cutoff, d.cutoff_inputs, d.cutoff_viewdir, d.density_scale = 4, 1, 1, 1, 1.0
        d.encoder_flags = _lib.ANERF_ENC_VIEW_WINDOWS
        for k, v in kw.items():
            setattr(d, k, v)
        h = ctypes.c_void_p()
        return lib.anerf_model_create(ctypes.byref(d), None, None, None, 0, ctypes.byref(h))
    assert create(cutoff_viewdir=0) == -1 and b"VIEW_WINDOWS" in lib.anerf_last_error()
    # (without use_cutoff the reference's view embedder is a plain Embedder: no windows to factor)
    assert create(use_cutoff=0) == -1 and b"VIEW_WINDOWS" in lib.anerf_last_error()
    assert create(cutoff_inputs=0) == -1 and b"VIEW_WINDOWS" in lib.anerf_last_error()
    assert create(encoder_flags=_lib.ANERF_ENC_VIEW_WINDOWS | _lib.ANERF_ENC_VIEW_ANGLE) == -1
    assert b"staged" in lib.anerf_last_error()
    assert create(multires_bones=2) == -1 and b"staged" in lib.anerf_last_error()
    assert create(encoder_flags=256) == -1 and b"unknown" in lib.anerf_last_error()


def test_package_reads_no_environment_switches(tmp_path):
    """with ANERF_LIB_PATH and ANERF_TRAIN_FWD set, a fresh process importing the package gets the
    in-tree library and the layer-by-layer training forward (the A/B tooling applies ANERF_LIB_PATH itself,
    tools/_ablib.py, through _lib.use_library)."""
    import subprocess
    import sys
    fake = tmp_path / "libfake.so"
    fake.write_bytes(b"not a library")
    code = ("import importlib, json; L = importlib.import_module('a-nerf_amd._lib'); "
            "M = importlib.import_module('a-nerf_amd.mlp'); L.load(); "
            "print(json.dumps([L.LIB_PATH, M.FUSED_FORWARD]))")
    env = dict(os.environ, ANERF_LIB_PATH=str(fake), ANERF_TRAIN_FWD="fused")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    path, fused = json.loads(out.stdout.strip().splitlines()[-1])
    assert os.path.abspath(path) == os.path.abspath(os.path.join(REPO, "a-nerf_amd", "libanerf_hip.so"))
    assert fused is False
    # the tooling hook does switch libraries, and the ABI check applies to what it loads
    code2 = ("import sys; sys.path.insert(0, 'tools'); import _ablib, importlib; "
             "L = importlib.import_module('a-nerf_amd._lib'); print(L.LIB_PATH)")
    out2 = subprocess.run([sys.executable, "-c", code2], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out2.returncode == 0 and out2.stdout.strip().endswith("libfake.so"), out2.stderr[-2000:]


def test_binding_rejects_a_wrong_argument_count():
    """_lib.load()'s entry points check their argument count (ctypes alone lets a surplus argument through)."""
    lib = _lib.load()
    with pytest.raises(TypeError, match="anerf_train_view_mix takes 9 arguments, got 10"):
        lib.anerf_train_view_mix(1, 1, 24, 130, 1, 24, 16, 16, None, None)
    assert lib.anerf_train_view_mix(1, 1, 24, 130, 1, 24, 16, 16, None) == -1

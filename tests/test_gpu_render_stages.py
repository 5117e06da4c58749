"""The render call's per-ray stages as kernels of their own: raw2outputs and the importance sampling after a render
launch that ends at the raws (render_coarse_stage_kernel / render_fine_stage_kernel), and the one case that keeps
them in the kernel (single_net, render_fused_kernel).

Every case isolates the stages from the MLP: the device's own debug arrays (raw_*, z_*, weights0) go through the CPU
oracle's raw2outputs and sample_pdf, and the device's maps, alphas and fine z are compared with what the oracle makes
of them, at the tolerances tests/test_gpu_parity.py uses for the same comparisons:
  * rgb / disp / acc maps 1e-4 absolute, per-sample alpha 2e-3, coarse weights 1e-5;
  * the sorted fine z bit for bit: the oracle's sample_pdf and the device's importance() both reproduce torch on
    identical weights (test_oracle_golden.test_compositing_and_sample_pdf_match_reference,
    test_gpu_parity.test_importance_bit_exact_on_reference_weights), and here the weights are identical.

Shapes: S + I = 64 + 128 (the flagship's), 8 + 4, 7 + 5 (T % 4 != 0: the scalar z hand-off) and I = 0; ray counts 1, 3,
6 and 261: no multiple of the rays per workgroup, the last workgroup ragged.  The rays are the NaN-fill fixture's, so
some miss the cylinder and get the chunk's mean near / far.
"""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

from _golden import Golden  # noqa: E402

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
syn = importlib.import_module("a-nerf_amd.synthetic")
config = importlib.import_module("a-nerf_amd.config")
_lib = importlib.import_module("a-nerf_amd._lib")

TOL = 1e-4
TOL_ALPHA = 2e-3
TOL_WEIGHTS = 1e-5
COUNTS = (1, 3, 6, 261)
SHAPES = [(64, 128), (8, 4), (7, 5), (33, 0)]
PRECISIONS = ["fp16x4", "fp32", "bf16x6"]


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def scene():
    """Rays, transforms and cylinder of the NaN-fill fixture (24 joints): the first 261 rays."""
    import oracle
    g = Golden("h1_nanfill_s32i16_d4w128")
    rb = np.ascontiguousarray(g.ray_batch()[:max(COUNTS)])
    _, _, q, _ = oracle.OracleModel(g.cfg, g.ckpt).near_far(rb, g["cyls"][0:1], chunk=4096)
    assert 0 < int(np.isnan(q).sum()) < len(rb), "the rays must hold hits and misses of the cylinder"
    return dict(rb=rb, skts=g["skts"][0:1], cyls=g["cyls"][0:1])


_MODELS = {}


def _model(W, precision, S, I, **kw):
    """A synthetic 4-layer model of width W (cached): the device caster and the oracle on the same checkpoint."""
    import oracle
    key = (W, precision, S, I, tuple(sorted(kw.items())))
    if key not in _MODELS:
        cfg = config.RenderConfig(n_joints=24, netdepth=4, netwidth=W, N_samples=S, N_importance=I,
                                  precision=precision, **kw).validate()
        ckpt = syn.make_checkpoint(90 + W, n_joints=24, D=4, W=W, fine=I > 0)
        _MODELS[key] = (anerf.RayCaster(cfg, ckpt), oracle.OracleModel(cfg, ckpt), cfg)
    return _MODELS[key]


def _importance_weights(w, single_net):
    """isample_from_lineseg's weights (ray_utils.py:265-277), float32 throughout."""
    w = np.asarray(w, np.float32)
    if not single_net:
        return np.ascontiguousarray(w[..., 1:-1])
    return 0.5 * (np.maximum(w[..., :-2], w[..., 1:-1]) + np.maximum(w[..., 1:-1], w[..., 2:])) + np.float32(0.01)


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaNs differ"
    d = float(np.nanmax(np.abs(got - ref))) if got.size and not np.isnan(ref).all() else 0.0
    print(f"{what}: max |device - oracle| = {d:.3e} (bound {tol:.0e})")
    assert d <= tol, f"{what}: {d:.3e} > {tol:.0e}"


def _render(rc, cfg, scene, rb, cams=None, **kw):
    n = rb.shape[0]
    skts = torch.from_numpy(scene["skts"]).cuda().expand(n, -1, -1, -1)
    cyls = torch.from_numpy(scene["cyls"]).cuda().expand(n, -1)
    kw.setdefault("lindisp", cfg.lindisp)
    out = rc.render_rays(torch.from_numpy(rb).cuda(), cfg.N_samples, skts=skts, cyls=cyls,
                         cams=None if cams is None else torch.from_numpy(cams).cuda(),
                         N_importance=cfg.N_importance, chunk=4096, debug=True, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    dbg = {k: v.cpu().numpy() for k, v in rc.last_debug.items()}
    return out, dbg


def _check(rc, om, cfg, scene, rb, what, cams=None, ret_alpha=True, **kw):
    """One render with debug arrays; the stages' outputs against the oracle on the device's own raws and z."""
    S, I = cfg.N_samples, cfg.N_importance
    out, dbg = _render(rc, cfg, scene, rb, cams=cams, ret_alpha=ret_alpha, **kw)
    assert ("alpha" in out) == ret_alpha and ("alpha0" in out) == (ret_alpha and I > 0)
    dirs = rb[:, 3:6]
    assert np.isfinite(dbg["z_coarse"]).all() and np.isfinite(dbg["raw_coarse"]).all()
    c = om.raw2outputs(dbg["raw_coarse"], dbg["z_coarse"], dirs)
    names = ("rgb0", "disp0", "acc0", "alpha0") if I > 0 else ("rgb_map", "disp_map", "acc_map", "alpha")
    for k, r in zip(names[:3], ("rgb_map", "disp_map", "acc_map")):
        _close(out[k], c[r], TOL, f"{what} {k}")
    if ret_alpha:
        _close(out[names[3]], c["alpha"], TOL_ALPHA, f"{what} {names[3]}")
    if I == 0:
        return out, dbg
    _close(dbg["weights0"], c["weights"], TOL_WEIGHTS, f"{what} weights0")
    z = dbg["z_coarse"]
    mids = (0.5 * (z[:, 1:] + z[:, :-1])).astype(np.float32)
    zis = om.sample_pdf(mids, _importance_weights(dbg["weights0"], cfg.single_net), I)
    np.testing.assert_array_equal(dbg["z_fine"], np.sort(np.concatenate([z, zis], -1), -1), err_msg=f"{what} z_fine")
    f = om.raw2outputs(dbg["raw_fine"], dbg["z_fine"], dirs)
    for k in ("rgb_map", "disp_map", "acc_map"):
        _close(out[k], f[k], TOL, f"{what} {k}")
    if ret_alpha:
        _close(out["alpha"], f["alpha"], TOL_ALPHA, f"{what} alpha")
    return out, dbg


@pytest.mark.parametrize("S,I", SHAPES)
@pytest.mark.parametrize("W", [64, 256])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stage_kernels_match_oracle_on_device_raws(scene, precision, W, S, I):
    rc, om, cfg = _model(W, precision, S, I)
    for n in COUNTS:
        _check(rc, om, cfg, scene, scene["rb"][:n], f"{precision} W{W} {S}+{I} n{n}")


@pytest.mark.parametrize("S,I", [(8, 4), (33, 0)])
def test_ret_alpha_off_leaves_the_maps_unchanged(scene, S, I):
    rc, om, cfg = _model(64, "fp16x4", S, I)
    rb = scene["rb"][:6]
    on, _ = _check(rc, om, cfg, scene, rb, f"alpha on {S}+{I}")
    off, _ = _check(rc, om, cfg, scene, rb, f"alpha off {S}+{I}", ret_alpha=False)
    for k in off:
        np.testing.assert_array_equal(off[k], on[k], err_msg=k)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lindisp(scene, precision):
    rc, om, cfg = _model(64, precision, 8, 4, lindisp=True)
    _, dbg = _check(rc, om, cfg, scene, scene["rb"][:6], f"lindisp {precision}")
    # inverse-depth samples: the spacing grows along the ray
    assert (np.diff(dbg["z_coarse"], 2, axis=-1) > 0).all()


def test_missed_rays_take_the_filled_near_far(scene):
    """A ray that misses the cylinder renders on the chunk's mean near / far (and alone, on the batch's 0 / 1)."""
    import oracle
    g = Golden("h1_nanfill_s32i16_d4w128")
    rb = scene["rb"]
    near, far, q, filled = oracle.OracleModel(g.cfg, g.ckpt).near_far(rb, scene["cyls"], chunk=4096)
    miss = np.flatnonzero(np.isnan(q))
    rc, om, cfg = _model(256, "fp16x4", 7, 5)
    _, dbg = _check(rc, om, cfg, scene, rb, "misses in the batch")
    np.testing.assert_array_equal(dbg["near"], near)
    np.testing.assert_array_equal(dbg["far"], far)
    np.testing.assert_array_equal(dbg["z_coarse"][miss][:, 0], near[miss])
    _, dbg1 = _check(rc, om, cfg, scene, rb[miss[:1]], "a miss alone")
    assert dbg1["near"][0] == rb[miss[0], 6] and dbg1["far"][0] == rb[miss[0], 7]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_near_far_given(scene, precision):
    rc, om, cfg = _model(64, precision, 8, 4)
    rbt = torch.from_numpy(scene["rb"][:37].copy()).cuda()
    anerf.raycaster.near_far(rbt, torch.from_numpy(scene["cyls"]).cuda(), out=(rbt[:, 6], rbt[:, 7]))
    rb = rbt.cpu().numpy()
    full, dbg = _check(rc, om, cfg, scene, rb, f"near_far_given {precision}", near_far_given=True)
    np.testing.assert_array_equal(dbg["near"], rb[:, 6])
    np.testing.assert_array_equal(dbg["far"], rb[:, 7])
    for i in (0, 5, 36):  # any sub-range renders as in the whole list
        one, _ = _check(rc, om, cfg, scene, rb[i:i + 1], f"near_far_given ray {i}", near_far_given=True)
        for k in one:
            np.testing.assert_array_equal(one[k][0], full[k][i], err_msg=f"ray {i} {k}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_net_keeps_the_fused_kernel(precision):
    """single_net: both passes, composite and importance sampling in one launch (the fine raws merged by sorted_idx)."""
    import dataclasses
    import oracle
    g = Golden("s1_single_s96i48_mrv0")
    cfg = dataclasses.replace(g.cfg, precision=precision)
    rc, om = anerf.RayCaster(cfg, g.ckpt), oracle.OracleModel(cfg, g.ckpt)
    sc = dict(skts=g["skts"][0:1], cyls=g["cyls"][0:1])
    rb = g.ray_batch()
    for n in (1, 6, 23):
        _check(rc, om, cfg, sc, np.ascontiguousarray(rb[:n]), f"single_net {precision} n{n}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_framecodes(precision):
    import dataclasses
    import oracle
    g = Golden("fc_64_s32i32_d4w128")
    cfg = dataclasses.replace(g.cfg, precision=precision)
    rc, om = anerf.RayCaster(cfg, g.ckpt), oracle.OracleModel(cfg, g.ckpt)
    sc = dict(skts=g["skts"][0:1], cyls=g["cyls"][0:1])
    rb = g.ray_batch()
    for cams in (g["cams"], g["cams_neg"]):
        for n in (3, 67):
            _check(rc, om, cfg, sc, np.ascontiguousarray(rb[:n]), f"framecodes {precision} n{n}",
                   cams=np.ascontiguousarray(cams[:n], np.float32))


@pytest.mark.parametrize("S,I", [(64, 128), (33, 0)])
def test_workspace_one_byte_short_is_refused_before_any_launch(scene, S, I):
    rc, _, cfg = _model(64, "fp16x4", S, I)
    lib = _lib.load()
    n = 6
    need = int(lib.anerf_workspace_size(rc.model.handle, n, S, I))
    assert need >= n * (S + I) * 16 + (n * (S + I) * 4 if I else 0)  # the raws (and the fine z) are in it
    rb = torch.from_numpy(scene["rb"][:n]).cuda()
    skts = torch.from_numpy(scene["skts"]).cuda().contiguous()
    cyls = torch.from_numpy(scene["cyls"]).cuda().contiguous()
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    outs = [torch.full(s, -7.0, device="cuda") for s in ((n, 3), (n,), (n,), (n, 3), (n,), (n,), (n, S + I), (n, S))]

    def call(nbytes):
        return lib.anerf_render_rays(rc.model.handle, _lib.ptr(rb), rb.shape[1], n, _lib.ptr(skts), _lib.ptr(cyls), 1,
                                     None, None, S, I, 4096, _lib.PRECISIONS["fp16x4"], *[_lib.ptr(o) for o in outs],
                                     None, _lib.ptr(ws), nbytes, _lib.stream_handle())

    assert call(need - 1) == -3  # ANERF_EWORKSPACE
    assert "workspace too small" in lib.anerf_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs) and not bool(ws.any()), "written before the size check"
    assert call(need) == 0
    torch.cuda.synchronize()
    final = outs[:3] + [outs[6][:, :S + I]] + (outs[3:6] + [outs[7]] if I else [])
    assert all(bool((o != -7.0).all()) for o in final)

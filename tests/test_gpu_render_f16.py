"""The fp16 render kernels (fp16x4, fp16x3) at the smallest shapes that reach every path of their hidden and view
layers (mlp_layer_h3): against the C oracle at the parity tests' 1e-4, and bit-identical from one call to the next.

Shapes: 1 ray and 5 rays (workgroups take R = 4 rays: 5 rays leave a ragged item of one ray, 1 ray is one alone);
S = 33 with I = 31 (two 32-sample blocks per ray, the last one partial, coarse and fine pass) and S = 64 with I = 0
(whole blocks, coarse only); 24 and 17 joints; net depth 8 and 6 (skips = (4,): at depth 6 the skip layer, layer 5,
is the last hidden layer).

Tolerance: 1e-4 absolute on every output, as tests/test_gpu_parity.py; on a near-empty ray (0 < acc < 2^-20) disp
is a ratio of a few 2^-24 alpha quanta and is held to 1e-4 plus the reference's own measured float32 spread
(oracle.h12_spread).
"""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
syn = importlib.import_module("a-nerf_amd.synthetic")

TOL = 1e-4
# (joints, net depth, S, I): every value of each axis twice, each pair of axes in both combinations where it matters
# (partial block x skip-last, coarse-only x skip-last, 17 joints x both sample shapes)
CASES = [(24, 8, 33, 31), (17, 6, 33, 31), (24, 6, 64, 0), (17, 8, 64, 0)]


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_scenes = {}


def _scene(nj, D, S, I):
    """Seeded scene, checkpoint, five rays through the body and the oracle's outputs for them (computed once per
    shape, shared by both precisions: the oracle is float32 throughout)."""
    key = (nj, D, S, I)
    if key not in _scenes:
        import oracle
        cfg = anerf.RenderConfig(n_joints=nj, netdepth=D, N_samples=S, N_importance=I).validate()
        ck = syn.make_checkpoint(31 + nj + D, n_joints=nj, D=D, W=256, fine=I > 0, tau=79.6)
        # (the 17-joint skeleton: the SMPL-24 scene without its arms below the collars; every parent of the first
        # 17 joints is among them, so their transforms are those of the whole skeleton)
        sc = syn.make_scene(n_joints=24, H=128, W=128, seed=7 + nj)
        sc = {**sc, "kps": np.ascontiguousarray(sc["kps"][:, :nj]), "skts": np.ascontiguousarray(sc["skts"][:, :nj])}
        idx, cyls, _ = anerf.rays.valid_pixels(sc["c2ws"], 128, 128, sc["focal"], kps=sc["kps"], ext_scale=0.001)
        om = oracle.OracleModel(cfg, ck)
        c2w = np.ascontiguousarray(sc["c2ws"][0][:3, :4])
        # five rays: of 64 evenly spaced candidates the four the oracle finds most opaque, and the emptiest one
        cand = idx[0][:: max(1, len(idx[0]) // 64)][:64]
        acc = om.render_rays(oracle.gen_rays(c2w, 128, 128, sc["focal"], cand), sc["skts"][0], cyls[0:1],
                             chunk=4096)["acc_map"]
        order = np.argsort(-acc, kind="stable")
        sel = cand[np.concatenate([order[:4], order[-1:]])]
        rb = np.ascontiguousarray(oracle.gen_rays(c2w, 128, 128, sc["focal"], sel), np.float32)
        # near / far of the five rays fixed once (their chunk's NaN fill), so that the first ray renders alone as
        # it does among the five
        near, far, _, _ = om.near_far(rb, cyls[0:1], chunk=4096)
        ref = om.render_rays(rb, sc["skts"][0], cyls[0:1], chunk=4096, near=near, far=far)
        rb[:, 6], rb[:, 7] = near, far
        _scenes[key] = dict(ck=ck, sc=sc, cyls=cyls, rb=rb, ref=ref)
    return _scenes[key]


def _render(rc, s, rb, S, I):
    n = rb.shape[0]
    out = rc.render_rays(torch.from_numpy(rb).cuda(), S, skts=torch.from_numpy(s["sc"]["skts"][0:1]).cuda().expand(n, -1, -1, -1),
                         cyls=torch.from_numpy(s["cyls"][0:1]).cuda().expand(n, -1), N_importance=I, chunk=4096,
                         near_far_given=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


@pytest.mark.parametrize("precision", ["fp16x4", "fp16x3"])
@pytest.mark.parametrize("nj,D,S,I", CASES)
def test_fp16_render_matches_oracle_and_repeats(nj, D, S, I, precision):
    import oracle
    s = _scene(nj, D, S, I)
    cfg = anerf.RenderConfig(n_joints=nj, netdepth=D, N_samples=S, N_importance=I, precision=precision).validate()
    rc = anerf.RayCaster(cfg, s["ck"])
    keys = ["rgb_map", "disp_map", "acc_map"] + (["rgb0", "disp0", "acc0"] if I > 0 else [])
    ne_tol = TOL + oracle.h12_spread()["float64"]
    for n in (1, 5):
        out = _render(rc, s, s["rb"][:n], S, I)
        again = _render(rc, s, s["rb"][:n], S, I)
        for k in keys:
            np.testing.assert_array_equal(out[k], again[k], err_msg=f"{n} rays, {k}: two calls differ")
            ref = np.asarray(s["ref"][k][:n], np.float64)
            d = np.abs(out[k].astype(np.float64) - ref).reshape(n, -1).max(-1)
            acc = np.asarray(s["ref"]["acc0" if k.endswith("0") else "acc_map"][:n], np.float64)
            empty = (acc > 0) & (acc < 2.0 ** -20) if k.startswith("disp") else np.zeros(n, bool)
            print(f"{precision} nj {nj} D {D} S {S} I {I} rays {n} {k}: max |gpu - oracle| {d.max():.3e}"
                  f" ({int(empty.sum())} near-empty)")
            assert np.isfinite(out[k]).all()
            assert (d[~empty] <= TOL).all(), f"{n} rays, {k}: {d[~empty].max():.3e}"
            assert (d[empty] <= ne_tol).all(), f"{n} rays, {k} on near-empty rays: {d[empty].max():.3e}"

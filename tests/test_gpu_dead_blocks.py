"""Dead-block skip of the render kernels: a 32-sample block whose densities are all exactly zero stores
(0, 0, 0, sigma) and leaves out the view layer, the view-direction part and the rgb head (mlp_block,
anerf_mlp.hpp).  Its samples have alpha == +0, so their colour terms are +-0 and no output changes.  A call
with a debug struct does not skip (raw_coarse / raw_fine hold the real rgb raws, the MFMA tally is the full
one), which gives both forms in one build: every output of a plain call must equal the debug call's bit for bit.

The rays are bench.py's frame (seed 13, tau 79.6, 512^2, 64 + 128 samples, near / far over the whole box's
chunks): 64 groups of 4 consecutive rays spread over the ray list, so that both dead and live blocks occur
and some of the workgroups' iterations are dead on all four waves.
"""
import importlib

import numpy as np
import pytest
import torch

from _golden import Golden

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
syn = importlib.import_module("a-nerf_amd.synthetic")
_lib = importlib.import_module("a-nerf_amd._lib")

MODES = ["fp16x4", "fp16x3", "bf16x6", "bf16x3", "fp32"]
MAPS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "alpha", "alpha0")
H = 512


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def frame():
    return _make_frame()


def _make_frame():
    """256 rays of bench.py's frame (64 groups of 4 consecutive rays), near / far of the whole box in columns 6, 7."""
    dev = torch.device("cuda:0")
    ck = syn.make_checkpoint(13, n_joints=24, D=8, W=256, fine=True, tau=79.6)
    sc = syn.make_scene(n_joints=24, H=H, W=H, seed=13)
    _, cyls, boxes = anerf.rays.valid_pixels(sc["c2ws"], H, H, sc["focal"], kps=sc["kps"], ext_scale=0.001)
    (x0, y0), (x1, y1) = (int(v) for v in boxes[0][0]), (int(v) for v in boxes[0][1])
    n = (x1 - x0) * (y1 - y0)
    c2w = torch.from_numpy(np.ascontiguousarray(sc["c2ws"][0][:3, :4])).to(dev)
    rb_all = torch.empty(n, 11, device=dev)
    _lib.check(_lib.load().anerf_gen_rays_box(_lib.ptr(c2w), H, H, sc["focal"], sc["focal"], 0.0, 0.0, 0, x0, y0, x1,
                                              y1, 0.0, 1.0, _lib.ptr(rb_all), _lib.stream_handle(dev)), "gen_rays_box")
    cyl = torch.from_numpy(cyls[0:1]).to(dev)
    anerf.raycaster.near_far(rb_all, cyl, chunk=4096, out=(rb_all[:, 6], rb_all[:, 7]))
    starts = np.linspace(0, n // 4 - 1, 64).astype(np.int64) * 4
    rows = (starts[:, None] + np.arange(4)[None, :]).reshape(-1)
    rb = rb_all[torch.from_numpy(rows).to(dev)].contiguous()
    torch.cuda.synchronize()
    return dict(ck=ck, rb=rb, skts=torch.from_numpy(sc["skts"][0:1]).to(dev), cyl=cyl)


def _caster(ck, precision, S, I):
    cfg = anerf.RenderConfig(n_joints=24, N_samples=S, N_importance=I, precision=precision).validate()
    return anerf.RayCaster(cfg, ck)


def _render(rc, f, rb, S, I, skts=None, **kw):
    n = rb.shape[0]
    out = rc.render_rays(rb, S, skts=f["skts"].expand(n, -1, -1, -1) if skts is None else skts,
                         cyls=f["cyl"].expand(n, -1), N_importance=I, chunk=4096, ret_alpha=True,
                         near_far_given=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _render_abi(rc, f, rb, S, I, ray_pose, debug):
    """anerf_render_rays with the caller's own per-ray pose indices into a one-pose table (RayCaster.render_rays
    forms the indices itself and never passes one out of range)."""
    import ctypes
    n, T = rb.shape[0], S + I
    f32 = dict(device=rb.device, dtype=torch.float32)
    out = {"rgb_map": torch.empty(n, 3, **f32), "disp_map": torch.empty(n, **f32), "acc_map": torch.empty(n, **f32),
           "alpha": torch.empty(n, T, **f32), "rgb0": torch.empty(n, 3, **f32), "disp0": torch.empty(n, **f32),
           "acc0": torch.empty(n, **f32), "alpha0": torch.empty(n, S, **f32)}
    dbg = None
    if debug:
        dbg = _lib.Debug()
        for k, shape in (("near", (n,)), ("far", (n,)), ("z_coarse", (n, S)), ("raw_coarse", (n, S, 4)),
                         ("weights0", (n, S)), ("z_fine", (n, T)), ("raw_fine", (n, T, 4))):
            out["debug_" + k] = torch.empty(*shape, **f32)
            setattr(dbg, k, ctypes.cast(out["debug_" + k].data_ptr(), _lib.c_f))
    skt = f["skts"].reshape(1, 24, 4, 4).contiguous()
    cyl = f["cyl"].reshape(1, 5).contiguous()
    ws, need = rc.model.workspace(n, S, I)
    code = _lib.load().anerf_render_rays(
        rc.model.handle, _lib.ptr(rb), rb.shape[1], n, _lib.ptr(skt), _lib.ptr(cyl), 1, _lib.ptr(ray_pose), None, S, I,
        4096, _lib.PRECISIONS[rc.cfg.precision] | _lib.ANERF_FLAG_NEAR_FAR, _lib.ptr(out["rgb_map"]),
        _lib.ptr(out["disp_map"]), _lib.ptr(out["acc_map"]), _lib.ptr(out["rgb0"]), _lib.ptr(out["disp0"]),
        _lib.ptr(out["acc0"]), _lib.ptr(out["alpha"]), _lib.ptr(out["alpha0"]), ctypes.byref(dbg) if dbg else None,
        _lib.ptr(ws), need, _lib.stream_handle(rb.device))
    _lib.check(code, "anerf_render_rays")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(plain, dbg, what, keys=MAPS):
    for k in keys:
        if k in dbg or k in plain:
            np.testing.assert_array_equal(plain[k], dbg[k], err_msg=f"{what} {k}")


@pytest.mark.parametrize("precision", MODES)
def test_skip_on_off_identity(frame, precision):
    """A plain call (skipping) equals a debug call (not skipping) on every map and alpha, and the rays give the
    skip something to do: between 0.2 and 0.6 of the fine pass's 32-sample blocks are all-zero, and at least one
    group of four rays has a live block."""
    rc = _caster(frame["ck"], precision, 64, 128)
    plain = _render(rc, frame, frame["rb"], 64, 128)
    dbg = _render(rc, frame, frame["rb"], 64, 128, debug=True)
    dead = (dbg["alpha"].reshape(256, 6, 32) == 0).all(-1)
    share = float(dead.mean())
    live_groups = int((~dead).reshape(64, -1).any(-1).sum())
    print(f"{precision}: all-zero fine blocks {share:.3f}, groups with a live block {live_groups} / 64")
    assert 0.2 <= share <= 0.6, share
    assert live_groups >= 1
    # the debug call's raws are the full computation's: a dead block's rgb raws are not the skip's zeros
    raw = rc.last_debug["raw_fine"].cpu().numpy().reshape(256, 6, 32, 4)
    assert np.any(raw[dead][..., :3] != 0)
    _assert_same(plain, dbg, precision)


@pytest.mark.parametrize("precision", MODES)
def test_nan_ray_stays_live(frame, precision):
    """An out-of-range pose index gives the ray NaN transforms.  What the full computation makes of them, the
    skipping call must make too, NaN for NaN (measured on the full computation, MI355X):
      * fp32: every sigma of the ray is NaN (compares unequal to zero: live); rgb and disp maps NaN, acc 1;
      * bf16x6, fp16x4 (fp16x3 alike): the ray's sigma comes out finite (0.628 on all 64 coarse samples, -0.133 on
        all 192 fine ones, so every fine alpha is 0), while the view factor G, and with it every rgb raw, is NaN:
        rgb_map = sum of 0 * NaN = NaN, disp_map and acc_map 0.  A block with zero density whose G or view windows
        are not finite therefore stays live;
      * bf16x3: disp_map 0 as in the split modes (its raws were not looked at).
    rgb_map and rgb0 are NaN in every mode; disp / acc / alpha are compared, and required to be NaN only in fp32,
    where they were seen to be."""
    rb = frame["rb"]
    n = rb.shape[0]
    bad = 101
    pose = torch.zeros(n, dtype=torch.int32, device=rb.device)
    pose[bad] = 7  # (one pose in the table)
    rc = _caster(frame["ck"], precision, 64, 128)
    plain = _render_abi(rc, frame, rb, 64, 128, pose, False)
    dbg = _render_abi(rc, frame, rb, 64, 128, pose, True)
    for k in MAPS:
        np.testing.assert_array_equal(plain[k], dbg[k], err_msg=k)  # (equal_nan is assert_array_equal's default)
    for k in ("rgb_map", "rgb0"):
        assert np.isnan(plain[k][bad]).all() and np.isnan(dbg[k][bad]).all(), k
    if precision == "fp32":
        assert np.isnan(plain["disp_map"][bad]) and np.isnan(plain["alpha"][bad]).all()
    ok = np.arange(n) != bad
    for k in MAPS:
        assert not np.isnan(plain[k][ok]).any(), k


@pytest.mark.parametrize("precision", ["fp32", "fp16x4"])
@pytest.mark.parametrize("name", ["v2_softplus_nocutview", "s1_single_s96i48_mrv0"])
def test_softplus_and_single_net(name, precision):
    """softplus density is never zero (the skip is off); single_net models get the skip through the fused kernel's
    shared mlp_block.  Plain call == debug call, bit for bit."""
    g = Golden(name)
    import dataclasses
    cfg = dataclasses.replace(g.cfg, precision=precision)
    rc = anerf.RayCaster(cfg, g.ckpt)
    rb = torch.from_numpy(g.ray_batch()).cuda()
    n = rb.shape[0]
    kw = dict(skts=torch.from_numpy(g["skts"][0:1]).cuda().expand(n, -1, -1, -1),
              cyls=torch.from_numpy(g["cyls"][0:1]).cuda().expand(n, -1), N_importance=cfg.N_importance, chunk=4096,
              ret_alpha=True, lindisp=cfg.lindisp)
    plain = {k: v.cpu().numpy() for k, v in rc.render_rays(rb, cfg.N_samples, **kw).items() if v is not None}
    dbg = {k: v.cpu().numpy() for k, v in rc.render_rays(rb, cfg.N_samples, debug=True, **kw).items() if v is not None}
    _assert_same(plain, dbg, f"{name} {precision}")


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("S,I", [(7, 5), (33, 0)])
def test_ragged_ray_alone_equals_batch(frame, precision, S, I):
    """254 rays (a last workgroup of two) at sample counts that are no multiple of 32: a ray rendered alone gets
    the outputs it gets inside the batch, with blocks skipped or not by waves that own them or redo the last one."""
    ck = frame["ck"] if I > 0 else syn.make_checkpoint(13, n_joints=24, D=8, W=256, fine=False, tau=79.6)
    rc = _caster(ck, precision, S, I)
    rb = frame["rb"][:254]
    full = _render(rc, frame, rb, S, I)
    dbg = _render(rc, frame, rb, S, I, debug=True)
    _assert_same(full, dbg, f"{precision} {S}+{I}")
    for i in (0, 101, 252, 253):
        one = _render(rc, frame, rb[i:i + 1], S, I)
        for k in MAPS:
            if k in full:
                np.testing.assert_array_equal(one[k][0], full[k][i], err_msg=f"{precision} {S}+{I} ray {i} {k}")

"""GPU: per-vertex normals and radiance colours of extracted meshes.

  * the normals kernel (anerf_isosurface_normals through isosurface.isosurface(normals=True)) against the NumPy
    checker of the same contract (isosurface.isosurface_reference, itself held to an analytic surface and to the
    reference viewer's normals in test_mesh_attrs.py);
  * the point-wise radiance kernel (anerf_radiance_points through RayCaster.render_pts_radiance) against the
    reference's stage dumps (tests/golden/*.npz stage_raw) and against the C oracle, under the raw bar of
    test_gpu_parity.py: 1e-4 + 1e-5 |ref|;
  * extract_mesh / render_mesh with the attributes end to end, and the argument checks of both C entries."""
import dataclasses
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import _iso_cases as C  # noqa: E402
from _golden import Golden  # noqa: E402

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
iso = importlib.import_module("a-nerf_amd.isosurface")
_lib = importlib.import_module("a-nerf_amd._lib")

EINVAL = -1
PRECISIONS = ["fp32", "bf16x3", "bf16x6", "fp16x3", "fp16x4"]


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _oracle():
    import oracle
    return oracle


def _raw_bar(a, ref, what):
    """The project's bar for raw network outputs (test_gpu_parity._raw_close): 1e-4 absolute plus 1e-5 of the
    element.  Prints the figure before it asserts."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    d = np.abs(a - ref)
    excess = d - (1e-4 + 1e-5 * np.abs(ref))
    print(f"{what}: max |gpu - reference| {d.max():.3e} (rgb {d[..., :3].max():.3e}, sigma {d[..., 3].max():.3e}), "
          f"max excess over the bar {excess.max():.3e}")
    assert excess.max() <= 0, f"{what}: max |gpu - reference| {d.max():.3e}"


def _caster(g, precision="fp32"):
    return anerf.RayCaster(dataclasses.replace(g.cfg, precision=precision), g.ckpt)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------ 5. the normals kernel against the checker
NORMAL_CASES = {
    "random9_s0": (("random_field", 0), 0.5, False),
    "random_5x9x13": (("random_field", 3, (5, 9, 13), False), 0.5, False),  # (one-sided borders, non-cubic)
    "sphere16": (("sphere_field",), 0.0, False),
    "blobs_67x61x71": (("blobs_field",), 0.5, False),  # (many workgroups, two scan tiles, ragged tail)
    "last_rows": (("last_rows_field",), 0.0, False),
    "relu": (("relu_field",), 0.25, True),
    "nan": (("nan_field",), 0.0, False),
}


def _assert_normals(n, ref, what):
    n = n.cpu().numpy() if isinstance(n, torch.Tensor) else n
    assert n.dtype == np.float32 and n.shape == ref.shape, (what, n.shape, ref.shape)
    assert np.isfinite(n).all(), what
    diff = int((n.view(np.int32) != ref.view(np.int32)).sum())
    d = float(np.abs(n.astype(np.float64) - ref).max()) if n.size else 0.0
    print(f"{what}: {len(n)} normals, components not bit-identical: {diff}, max |gpu - checker| {d:.3e}")
    assert d <= 1e-6, what


@pytest.mark.parametrize("name", list(NORMAL_CASES))
@pytest.mark.parametrize("flip", [False, True])
def test_normals_match_the_checker(name, flip):
    (fn, *args), thr, relu = NORMAL_CASES[name]
    field = getattr(C, fn)(*args)
    rv, rt, rn = iso.isosurface_reference(field, thr, relu=relu, flip=flip, normals=True)
    assert len(rv) > 0
    v, t, n = iso.isosurface(field, thr, relu=relu, flip=flip, normals=True)
    assert n.is_cuda and n.dtype == torch.float32
    np.testing.assert_array_equal(t.cpu().numpy(), rt)
    pv, pt = iso.isosurface(field, thr, relu=relu, flip=flip)  # the plain call: the same mesh
    assert torch.equal(v, pv) and torch.equal(t, pt)
    _assert_normals(n, rn, f"{name} flip={flip}")
    if name == "nan":  # (a NaN sample next to a crossing edge's outside end: a zero normal, test_mesh_attrs.py)
        f = field.copy()
        f[0, 7, 7] = np.nan
        r2 = iso.isosurface_reference(f, thr, flip=flip, normals=True)
        assert (np.abs(r2[2]).max(axis=1) == 0).sum() == 1
        _assert_normals(iso.isosurface(f, thr, flip=flip, normals=True)[2], r2[2], "nan + a touched vertex")


def test_normals_deterministic_and_stream_independent():
    f = torch.from_numpy(C.blobs_field().copy()).cuda()
    v0, t0, n0 = iso.isosurface(f, 0.5, normals=True)
    v1, t1, n1 = iso.isosurface(f, 0.5, normals=True)
    assert torch.equal(n0, n1) and torch.equal(v0, v1) and torch.equal(t0, t1)
    pv, pt = iso.isosurface(f, 0.5)
    assert torch.equal(v0, pv) and torch.equal(t0, pt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        v2, t2, n2 = iso.isosurface(f, 0.5, normals=True)
    s.synchronize()
    assert torch.equal(n0, n2) and torch.equal(v0, v2) and torch.equal(t0, t2)
    e = iso.isosurface(f, 5.0, normals=True)  # (above the maximum: empty, nothing launched for the normals)
    assert [tuple(x.shape) for x in e] == [(0, 3)] * 3 and e[2].is_cuda and e[2].dtype == torch.float32


# ------------------------------------------------------------------ 6. radiance against the reference's stage dumps
STAGE = ["c2_256_s64_d8w256", "c4_512_s64i128_j65", "fc_64_s32i32_d4w128", "v1_mr10_w64_d4", "v2_softplus_nocutview",
         "v3_nocutinputs", "s1_single_s96i48_mrv0", "mr5_mrv2_s32i16_d8w256", "vw1_viewworld_s32i16_d8w128",
         "cb1_cutoffbones_s32i16_d8w128"]
STAGE_CASES = [(n, "fp32") for n in STAGE] + [(n, p) for n in STAGE[:2] for p in PRECISIONS[1:]]


def _stage_points(g, z):
    """pts = rays_o + rays_d * z of the first 4 rays, the multiply and the add separately rounded in float32."""
    o, d = g["rays_o"][:4].astype(np.float32), g["rays_d"][:4].astype(np.float32)
    prod = (d[:, None, :] * z[:, :, None].astype(np.float32)).astype(np.float32)
    return (o[:, None, :] + prod).astype(np.float32), d


def _radiance_rays(rc, g, pts, d, network, cams=None):
    """One call per ray (a ray has one direction and one framecode): [4, S, 4]."""
    out = []
    for r in range(pts.shape[0]):
        raw = rc.render_pts_radiance(_t(pts[r]), _t(d[r]), _t(g["kps"]), _t(g["skts"]), None,
                                     cams=None if cams is None else cams[r], network=network)
        assert tuple(raw.shape) == (pts.shape[1], 4) and raw.is_cuda and raw.dtype == torch.float32
        out.append(raw.cpu().numpy())
    return np.stack(out)


@pytest.mark.parametrize("name,precision", STAGE_CASES)
def test_radiance_matches_the_stage_dumps(name, precision):
    g = Golden(name)
    rc = _caster(g, precision)
    pts, d = _stage_points(g, g["stage_z"])
    cams = g["cams"][:4] if g.has("cams") else None
    raw = _radiance_rays(rc, g, pts, d, "coarse", cams)
    _raw_bar(raw, g["stage_raw"], f"{name} {precision} coarse")
    # per-point directions in one call: the same values as one direction per call
    dd = np.broadcast_to(d[:, None, :], pts.shape)
    if cams is None:
        one = rc.render_pts_radiance(_t(pts), _t(dd), _t(g["kps"]), _t(g["skts"]), None, network="coarse")
        assert tuple(one.shape) == pts.shape[:-1] + (4,)
        _raw_bar(one.cpu().numpy(), g["stage_raw"], f"{name} {precision} coarse, one call")


def test_radiance_fine_network_matches_the_stage_dump():
    g = Golden("c3_512_s64i128_d8w256")
    rc = _caster(g)
    pts, d = _stage_points(g, g["stage_z_all"])
    raw = _radiance_rays(rc, g, pts, d, "fine")
    _raw_bar(raw, g["stage_raw_f"], "c3 fine at stage_z_all")
    default = _radiance_rays(rc, g, pts[:1], d[:1], None)  # (the reference's default network: the fine one)
    np.testing.assert_array_equal(default, raw[:1])


def test_radiance_mean_framecode_matches_the_oracle():
    """cams=None / a negative index: the eval-mode mean code (the fixture's `outneg` renders use it; no stage dump
    exists for them, so the raws come from the oracle with the mean code rows)."""
    g = Golden("fc_64_s32i32_d4w128")
    assert (g["cams_neg"] < 0).all()
    rc = _caster(g)
    om = _oracle().OracleModel(g.cfg, g.ckpt)
    pts, d = _stage_points(g, g["stage_z"])
    codes = np.asarray(g.ckpt["network_fn_state_dict"]["framecodes.codes.weight"], np.float64)
    mean = (codes.sum(0) / codes.shape[0]).astype(np.float32)
    p = pts.reshape(-1, 3)
    dd = np.ascontiguousarray(np.broadcast_to(d[:, None, :], pts.shape)).reshape(-1, 3)
    ref = om.network(om.encode(g["skts"][0], p, dd), fine=False, code=np.tile(mean, (len(p), 1)))
    for cams in (None, -1, g["cams_neg"][:1]):
        raw = rc.render_pts_radiance(_t(p), _t(dd), _t(g["kps"]), _t(g["skts"]), None, cams=cams, network="coarse")
        _raw_bar(raw.cpu().numpy(), ref, f"fc mean code (cams={cams!r})")
    # and an explicit index differs from it
    idx = rc.render_pts_radiance(_t(p), _t(dd), _t(g["kps"]), _t(g["skts"]), None, cams=2, network="coarse")
    ref2 = om.network(om.encode(g["skts"][0], p, dd), fine=False, code=np.tile(codes[2].astype(np.float32), (len(p), 1)))
    _raw_bar(idx.cpu().numpy(), ref2, "fc code 2")
    assert float((idx - raw)[:, :3].abs().max()) > 1e-3
    with pytest.raises(NotImplementedError, match="one framecode"):
        rc.render_pts_radiance(_t(p), _t(dd), _t(g["kps"]), _t(g["skts"]), None, cams=g["cams"][:4])


# ------------------------------------------------------------------ 7. per-point directions against the C oracle
def _points77(g, seed):
    """77 points (two whole blocks and a ragged third): 50 near joints, 27 beyond every cutoff; independent
    random unit directions."""
    rng = np.random.default_rng(seed)
    kps = g["kps"][0]
    near = kps[rng.integers(0, len(kps), 50)] + rng.normal(0, 0.08, (50, 3))
    far = kps[0] + rng.normal(0, 1.0, (27, 3)) + np.array([60.0, -45.0, 80.0])
    order = rng.permutation(77)
    pts = np.concatenate([near, far])[order].astype(np.float32)
    is_far = (np.arange(77) >= 50)[order]
    d = rng.normal(0, 1, (77, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return pts, d, is_far


@pytest.mark.parametrize("name", ["c2_256_s64_d8w256", "c4_512_s64i128_j65"])
@pytest.mark.parametrize("precision", ["fp32", "fp16x4"])
def test_radiance_per_point_directions_match_the_oracle(name, precision):
    g = Golden(name)
    rc = _caster(g, precision)
    om = _oracle().OracleModel(g.cfg, g.ckpt)
    pts, d, is_far = _points77(g, 77)
    args = (_t(g["kps"]), _t(g["skts"]), None)
    ref = om.network(om.encode(g["skts"][0], pts, d), fine=False)
    raw = rc.render_pts_radiance(_t(pts), _t(d), *args, network="coarse")
    assert tuple(raw.shape) == (77, 4)
    _raw_bar(raw.cpu().numpy(), ref, f"{name} {precision} 77 points")
    # beyond every cutoff all view windows are exactly zero: the view layer's direction part is its bias column
    # alone, so the output does not depend on the direction at all
    feat = om.encode(g["skts"][0], pts[is_far], d[is_far])
    nview = 3 * g.cfg.n_joints * (1 + 2 * g.cfg.multires_views)
    assert (feat[:, -nview:] == 0).all()
    far_a = rc.render_pts_radiance(_t(pts[is_far]), _t(d[is_far]), *args, network="coarse")
    far_b = rc.render_pts_radiance(_t(pts[is_far]), _t(-d[is_far][::-1].copy()), *args, network="coarse")
    assert torch.equal(far_a, far_b)
    _raw_bar(far_a.cpu().numpy(), ref[is_far], f"{name} {precision} beyond the cutoffs")
    assert float((rc.render_pts_radiance(_t(pts), _t(-d), *args, network="coarse") - raw)[:, :3].abs().max()) > 1e-3
    # one direction for all points (read with stride 0) == the same direction repeated
    one = rc.render_pts_radiance(_t(pts), _t(d[3]), *args, network="coarse")
    rep = rc.render_pts_radiance(_t(pts), _t(np.tile(d[3], (77, 1))), *args, network="coarse")
    assert torch.equal(one, rep)
    _raw_bar(one.cpu().numpy(), om.network(om.encode(g["skts"][0], pts, np.tile(d[3], (77, 1))), fine=False),
             f"{name} {precision} one direction")
    # the sigma column is render_pts_density's
    dens = rc.render_pts_density(_t(pts), *args, network="coarse").cpu().numpy()
    _raw_bar(np.concatenate([raw.cpu().numpy()[:, :3], dens], -1), raw.cpu().numpy(), f"{name} {precision} sigma vs density")
    # shapes: leading dimensions kept, an empty query
    assert tuple(rc.render_pts_radiance(_t(pts[:66].reshape(2, 3, 11, 3)), _t(d[0]), *args).shape) == (2, 3, 11, 4)
    assert tuple(rc.render_pts_radiance(_t(pts[:0]), _t(d[:0]), *args).shape) == (0, 4)


# ------------------------------------------------------------------ 8. end to end
THR = 0.3  # (dm_fine_d8w256, as test_gpu_isosurface.py)


def _pose(g):
    return _t(g["kps"]), _t(g["skts"]), _t(g["bones"]) if g.has("bones") else None


def _colour_reference(g, om, vw, outward):
    """sigmoid of the oracle's raw rgb (the default network: fine) at the world vertices, looked at against the
    outward normal, or towards kps[0, 0] where the normal is zero."""
    zero = (outward == 0).all(axis=1, keepdims=True)
    d = np.where(zero, g["kps"][0, 0].astype(np.float32) - vw, -outward).astype(np.float32)
    raw = om.network(om.encode(g["skts"][0], vw, d), fine=True)
    return 1.0 / (1.0 + np.exp(-raw[:, :3].astype(np.float64)))


def test_extract_mesh_with_normals_and_colours():
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = _caster(g)
    om = _oracle().OracleModel(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    kw = dict(radius=radius, res=res, threshold=THR)
    pv, pt = rc.extract_mesh(kps, skts, bones, coords="world", **kw)
    v, t, a = rc.extract_mesh(kps, skts, bones, coords="world", normals=True, colors=True, **kw)
    assert torch.equal(v, pv) and torch.equal(t, pt) and len(t) > 0
    assert sorted(a) == ["colors", "normals"]
    for x in a.values():
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == tuple(v.shape)
    own = rc.render_mesh_density(kps, skts, bones, radius=radius, res=res)
    _, _, rn = iso.isosurface_reference(own.cpu().numpy(), THR, relu=True, normals=True)
    _assert_normals(a["normals"], np.ascontiguousarray(rn[:, [1, 0, 2]]), "extract_mesh world normals")
    assert C.signed_volume(v.cpu().numpy(), t.cpu().numpy()) > 0
    # normals and winding have the same sense (outward).  This density is a random network's: rough at the grid's
    # scale, so a face may disagree with the gradient at its corners -- the sense is what is checked here (the
    # majority of the faces; face by face on smooth fields in test_mesh_attrs.py)
    p = v.cpu().numpy().astype(np.float64)[t.cpu().numpy().astype(np.int64)]
    face = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    nsum = a["normals"].cpu().numpy().astype(np.float64)[t.cpu().numpy().astype(np.int64)].sum(1)
    agree = float(((face * nsum).sum(1) > 0).mean())
    print(f"faces whose winding agrees with their corners' normals: {agree:.3f}")
    assert agree > 0.5
    col = a["colors"].cpu().numpy()
    assert col.min() >= 0 and col.max() <= 1
    ref = _colour_reference(g, om, v.cpu().numpy(), a["normals"].cpu().numpy())
    d = float(np.abs(col - ref).max())
    print(f"colours vs sigmoid(oracle raw): max {d:.3e} over {len(col)} vertices, range [{col.min():.3f}, {col.max():.3f}]")
    assert d <= 1e-4
    # the frames: "index" and "unit" share the normals, "world" permutes them; colours are queried in the world
    vi, ti, ai = rc.extract_mesh(kps, skts, bones, coords="index", normals=True, colors=True, **kw)
    vu, tu, au = rc.extract_mesh(kps, skts, bones, normals=True, **kw)
    assert sorted(au) == ["normals"] and torch.equal(au["normals"], ai["normals"])
    assert torch.equal(ai["normals"][:, [1, 0, 2]], a["normals"]) and torch.equal(ai["colors"], a["colors"])
    _assert_normals(ai["normals"], rn, "extract_mesh index normals")
    # flip: winding and normals reversed together, the viewing direction (from outside) and so the colours not
    vf, tf, af = rc.extract_mesh(kps, skts, bones, coords="world", flip=True, normals=True, colors=True, **kw)
    assert torch.equal(vf, v) and torch.equal(tf, t[:, [0, 2, 1]])
    assert torch.equal(af["normals"], -a["normals"]) and torch.equal(af["colors"], a["colors"])
    # one direction for all vertices
    view = (0.3, -0.5, 0.8)
    vc, tc, ac = rc.extract_mesh(kps, skts, bones, coords="world", colors=True, view=view, **kw)
    assert sorted(ac) == ["colors"] and torch.equal(vc, v)
    raw = om.network(om.encode(g["skts"][0], v.cpu().numpy(), np.tile(np.float32(view), (len(v), 1))), fine=True)
    assert float(np.abs(ac["colors"].cpu().numpy() - 1 / (1 + np.exp(-raw[:, :3].astype(np.float64)))).max()) <= 1e-4
    # above the grid's maximum: an empty mesh with empty attributes
    ve, te, ae = rc.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=float(own.max()) + 1.0,
                                 normals=True, colors=True)
    assert tuple(ve.shape) == (0, 3) and tuple(te.shape) == (0, 3)
    assert tuple(ae["normals"].shape) == (0, 3) and tuple(ae["colors"].shape) == (0, 3)
    assert ae["colors"].is_cuda and ae["colors"].dtype == torch.float32


def test_render_mesh_writes_colours_into_the_plys(tmp_path):
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = _caster(g)
    kps, skts, bones = _pose(g)
    data = {"kp": kps, "skts": skts, "bones": bones}
    out = anerf.render_mesh(str(tmp_path), {"ray_caster": rc, "preproc_kwargs": {}}, data, radius=radius, res=res,
                            threshold=THR, colors=True)
    assert len(out) == 1 and len(out[0]) == 3
    v, t, a = out[0]
    ev, et, ea = rc.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=THR, colors=True)
    assert torch.equal(v, ev) and torch.equal(t, et) and torch.equal(a["colors"], ea["colors"]) and sorted(a) == ["colors"]
    pv, pt, pa = iso.read_ply(str(tmp_path / "meshes" / "000.ply"), attributes=True)
    np.testing.assert_array_equal(pv, v.cpu().numpy())
    np.testing.assert_array_equal(pt, t.cpu().numpy())
    assert sorted(pa) == ["colors"] and pa["colors"].dtype == np.uint8
    np.testing.assert_array_equal(pa["colors"], np.rint(np.float32(255) * a["colors"].cpu().numpy()).astype(np.uint8))
    assert len(np.unique(pa["colors"], axis=0)) > 8
    # the plain call still writes the plain file
    plain = anerf.render_mesh(str(tmp_path / "p"), {"ray_caster": rc, "preproc_kwargs": {}}, data, radius=radius, res=res,
                              threshold=THR)
    assert len(plain[0]) == 2 and torch.equal(plain[0][0], v)
    assert iso.read_ply(str(tmp_path / "p" / "meshes" / "000.ply"), attributes=True)[2] == {}
    both = anerf.render_mesh(str(tmp_path / "b"), {"ray_caster": rc, "preproc_kwargs": {}}, data, radius=radius, res=res,
                             threshold=THR, normals=True, colors=True)
    ba = iso.read_ply(str(tmp_path / "b" / "meshes" / "000.ply"), attributes=True)[2]
    np.testing.assert_array_equal(ba["normals"], both[0][2]["normals"].cpu().numpy())
    np.testing.assert_array_equal(ba["colors"], pa["colors"])


def test_staged_caster_gives_normals_and_refuses_colours():
    g = Golden("sgd1_relpos_mrb2_density")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    sc = rc._staged.eval_caster()
    kps, skts, bones = _pose(g)
    own = sc.render_mesh_density(kps, skts, bones, radius=radius, res=res)
    rv, rt, rn = iso.isosurface_reference(own.cpu().numpy(), 2.0, relu=True, normals=True)
    assert len(rt) > 0
    for caster in (sc, rc):
        v, t, a = caster.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=2.0, coords="index",
                                      normals=True)
        np.testing.assert_array_equal(t.cpu().numpy(), rt)
        np.testing.assert_array_equal(v.cpu().numpy(), rv)
        assert sorted(a) == ["normals"]
        _assert_normals(a["normals"], rn, "staged normals")
        with pytest.raises(NotImplementedError, match="staged"):
            caster.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=2.0, colors=True)
    with pytest.raises(NotImplementedError, match="staged"):
        rc.render_pts_radiance(_t(g["pts"][:5]), _t(np.float32([0, 0, 1])), kps, skts, bones)


# ------------------------------------------------------------------ 9. argument validation
def test_radiance_entry_rejects_bad_arguments():
    g = Golden("c2_256_s64_d8w256")
    rc = _caster(g)
    lib = _lib.load()
    err = lambda: lib.anerf_last_error()  # noqa: E731
    dev = "cuda"
    pts = torch.zeros(5, 3, device=dev)
    dirs = torch.ones(5, 3, device=dev)
    sk = _t(g["skts"]).to(dev).contiguous()
    GUARD = 12345.0
    out = torch.full((5, 4), GUARD, device=dev)
    h, P = rc.model.handle, _lib.ptr
    call = lambda m, p, n, d, nd, s, cam, net, prec, o: lib.anerf_radiance_points(  # noqa: E731
        m, p, n, d, nd, s, cam, net, prec, o, _lib.stream_handle())
    good = (h, P(pts), 5, P(dirs), 5, P(sk), -1.0, 0, 0, P(out))
    for i in (0, 1, 3, 5, 9):  # NULL model, pts, dirs, skts, raw_out
        a = list(good)
        a[i] = None
        assert call(*a) == EINVAL and b"anerf_radiance_points" in err() and b"NULL" in err(), i
    bad = {"n_points < 0": (2, -1, b"n_points"), "n_dirs = 2 with n = 5": (4, 2, b"n_dirs"), "net = 7": (7, 7, b"network"),
           "net = -2": (7, -2, b"network"), "net = 1 without a fine network": (7, 1, b"network"),
           "precision 5": (8, 5, b"precision"), "precision -1": (8, -1, b"precision")}
    for what, (i, val, msg) in bad.items():
        a = list(good)
        a[i] = val
        assert call(*a) == EINVAL and b"anerf_radiance_points" in err() and msg in err(), what
    gs = Golden("sgd1_relpos_mrb2_density")
    staged = anerf.RayCaster(gs.cfg, gs.ckpt)
    a = list(good)
    a[0] = staged.model.handle
    assert call(*a) == EINVAL and b"staged encoder" in err()
    gf = Golden("fc_64_s32i32_d4w128")
    rf = _caster(gf)
    a = list(good)
    a[0], a[6] = rf.model.handle, 5.0  # (5 framecodes: index 5 is past the table)
    assert call(*a) == EINVAL and b"framecode" in err()
    torch.cuda.synchronize()
    assert bool((out == GUARD).all())  # nothing was launched
    # n_points == 0: ANERF_OK without a launch; and the good call runs
    a = list(good)
    a[2], a[4] = 0, 0
    assert call(*a) == 0
    torch.cuda.synchronize()
    assert bool((out == GUARD).all())
    assert call(*good) == 0
    torch.cuda.synchronize()
    assert bool((out != GUARD).all()) and bool(torch.isfinite(out).all())


def test_normals_entry_capacity_and_bad_arguments():
    lib = _lib.load()
    err = lambda: lib.anerf_last_error()  # noqa: E731
    field = C.sphere_field()
    rv, rt, rn = iso.isosurface_reference(field, 0.0, normals=True)
    V = len(rv)
    vol = torch.from_numpy(field.copy()).cuda()
    n0, n1, n2 = vol.shape
    need = lib.anerf_isosurface_workspace(n0, n1, n2)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    totals = torch.empty(2, device="cuda", dtype=torch.int64)
    st = _lib.stream_handle()
    P = _lib.ptr
    assert lib.anerf_isosurface_count(P(vol), n0, n1, n2, 0.0, 0, P(ws), need, P(totals), st) == 0
    assert int(totals[0]) == V
    GUARD = 777.0
    buf = torch.full((V, 3), GUARD, device="cuda")
    cap = V - 5
    for bad in ((None, P(ws), P(buf)), (P(vol), None, P(buf)), (P(vol), P(ws), None)):
        assert lib.anerf_isosurface_normals(bad[0], n0, n1, n2, 0.0, 0, bad[1], need, bad[2], cap, st) == EINVAL
        assert b"anerf_isosurface_normals" in err() and b"NULL" in err()
    assert lib.anerf_isosurface_normals(P(vol), n0, n1, n2, 0.0, 4, P(ws), need, P(buf), cap, st) == EINVAL
    assert lib.anerf_isosurface_normals(P(vol), n0, n1, n2, 0.0, 0, P(ws), need, P(buf), -1, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())  # nothing was launched
    # a capacity smaller than V: the rows beyond it are dropped, nothing past it is written
    assert lib.anerf_isosurface_normals(P(vol), n0, n1, n2, 0.0, 0, P(ws), need, P(buf), cap, st) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[cap:] == GUARD).all()
    _assert_normals(got[:cap], rn[:cap], "capacity V - 5")
    # before the emit pass or after it: the same normals (the pass writes nothing to the workspace)
    verts = torch.empty((V, 3), device="cuda")
    tris = torch.empty((len(rt), 3), device="cuda", dtype=torch.int32)
    assert lib.anerf_isosurface_emit(P(vol), n0, n1, n2, 0.0, 0, P(ws), need, P(verts), V, P(tris), len(rt), st) == 0
    full = torch.empty((V, 3), device="cuda")
    assert lib.anerf_isosurface_normals(P(vol), n0, n1, n2, 0.0, 0, P(ws), need, P(full), V, st) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tris.cpu().numpy(), rt)
    assert torch.equal(full[:cap], buf[:cap])
    _assert_normals(full, rn, "after emit")

"""GPU: the rasteriser and the face-accumulated vertex normals (csrc/anerf_raster.hip through meshops.rasterize_mesh /
vertex_normals / mesh_turntable) against the NumPy checkers of the same contract (themselves held to exact-once
coverage, to float64 and to the sphere in test_mesh_raster.py), and normals="faces" end to end through extract_mesh.
Coverage, the depth test and the normals' sums are integers; every float is a correctly rounded fp32 operation on both
sides, in the same order: all comparisons are exact, floats through their int32 views."""
import importlib

import numpy as np
import pytest
import torch

import _mesh_cases as M
import _raster_cases as R
import _smooth_cases as S
from _golden import Golden

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
meshops = importlib.import_module("a-nerf_amd.meshops")
_lib = importlib.import_module("a-nerf_amd._lib")


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _assert_raster(got, ref, what):
    """Zero differing words between a device MeshRaster and the checker's, field by field."""
    assert isinstance(got, meshops.MeshRaster)
    for name, g, r in zip(got._fields, got, ref):
        if r is None:
            assert g is None, (what, name)
            continue
        assert g.is_cuda and g.dtype == (torch.int32 if name == "face_ids" else torch.float32), (what, name)
        g = g.cpu().numpy()
        assert g.shape == r.shape, (what, name)
        diff = int((_bits(g) != _bits(r)).sum())
        print(f"{what}: {name}: {diff} differing words of {r.size}")
        assert diff == 0, (what, name)


def _run(sc, **kw):
    v, t, A, w, h, attrs = sc
    return meshops.rasterize_mesh(_dev(v), _dev(t), A, w, h, _dev(attrs), R.BACKGROUND, **kw)


# ------------------------------------------------------------------ the rasteriser
@pytest.mark.parametrize("name", R.BASIC)
def test_raster_matches(name):
    _assert_raster(_run(R.scene(name)), R.reference(name), name)


@pytest.mark.parametrize("name", R.SPLIT)
def test_both_sides_of_the_size_split(name):
    """Bounding boxes of RASTER_SMALL_PIXELS - 1, + 0 and + 1 pixel centres (the last one goes to the workgroups'
    list), a triangle over all of 1024 x 1024 and a cube's twelve at 512 x 512: the large path exists -- a thread per
    triangle would walk up to a million pixels -- and gives the same bits."""
    _assert_raster(_run(R.scene(name)), R.reference(name), name)


@pytest.mark.parametrize("name", ["sphere", "blobs"])
@pytest.mark.parametrize("frame", R.VIEWS)
def test_real_meshes_under_the_turntable_matrices(name, frame):
    ref = R.mesh_reference(name, frame)
    assert 0.1 < (ref.face_ids >= 0).mean() < 0.9
    _assert_raster(_run(R.mesh_scene(name, frame)), ref, f"{name} frame {frame}")


def test_triangle_order_does_not_matter():
    v, t, A, w, h, attrs = R.mesh_scene("sphere", 7)
    ref = R.mesh_reference("sphere", 7)
    # no two triangles tie for a pixel: the checker's winner is nearer than every other fragment there
    for k in np.unique(ref.face_ids[ref.face_ids >= 0])[::9]:
        others = meshops.rasterize_mesh_reference(v, np.delete(t, k, axis=0), A, w, h)
        mine = ref.face_ids == k
        assert (others.depth[mine] > ref.depth[mine]).all()
    perm = np.random.default_rng(5).permutation(len(t))
    got = meshops.rasterize_mesh(_dev(v), _dev(t[perm]), A, w, h, _dev(attrs), R.BACKGROUND)
    ids = got.face_ids.cpu().numpy()
    np.testing.assert_array_equal(np.where(ids >= 0, perm[ids], -1), ref.face_ids)
    for name in ("depth", "bary", "image"):
        np.testing.assert_array_equal(_bits(getattr(got, name).cpu().numpy()), _bits(getattr(ref, name)), err_msg=name)


def test_repeatable_on_any_stream_inputs_untouched():
    sc = R.scene("soup_257x255")
    dv = _dev(sc[0])
    keep = dv.clone()

    def run():
        return meshops.rasterize_mesh(dv, _dev(sc[1]), sc[2], sc[3], sc[4], _dev(sc[5]), R.BACKGROUND)
    a, b = run(), run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = run()
        n = meshops.vertex_normals(_dev(M.mesh("sphere")[0]), _dev(M.mesh("sphere")[1]))
    s.synchronize()
    for x, y, z in zip(a, b, c):
        x, y, z = (u.view(torch.int32) for u in (x, y, z))
        assert torch.equal(x, y) and torch.equal(x, z)
    _assert_raster(c, R.reference("soup_257x255"), "side stream")
    np.testing.assert_array_equal(_bits(n.cpu().numpy()), _bits(R.normals_reference("sphere")[2]))
    assert torch.equal(dv.view(torch.int32), keep.view(torch.int32))


def test_host_inputs_int64_and_background_forms():
    v, t, A, w, h, attrs = R.scene("soup_37x21")
    ref = R.reference("soup_37x21")
    _assert_raster(meshops.rasterize_mesh(np.array(v), t.astype(np.int64), torch.from_numpy(np.array(A)), w, h,
                                          np.array(attrs), R.BACKGROUND), ref, "host inputs")
    bg = (0.1, 0.2, 0.3)
    got = meshops.rasterize_mesh(_dev(v), _dev(t), A, w, h, _dev(attrs), bg)
    _assert_raster(got, meshops.rasterize_mesh_reference(v, t, A, w, h, attrs, bg), "three backgrounds")
    assert (got.image[got.face_ids < 0] == torch.tensor(bg, device="cuda")).all()


def test_argument_errors_come_before_a_launch(monkeypatch):
    def no_library():
        raise AssertionError("the argument checks must come before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    v, t, A, w, h, attrs = R.scene("soup_37x21")
    dv, dt, da = _dev(v), _dev(t), _dev(attrs)
    with pytest.raises(ValueError, match="outside"):
        meshops.rasterize_mesh(dv, dt + 1000, A, w, h)
    with pytest.raises(ValueError, match="outside"):
        meshops.vertex_normals(dv, dt - 1000)
    with pytest.raises(ValueError, match="outside"):
        meshops.mesh_turntable(dv, dt + 1000, frames=1)
    for bad in (0, 16385):
        with pytest.raises(ValueError, match="width"):
            meshops.rasterize_mesh(dv, dt, A, bad, h)
        with pytest.raises(ValueError, match="height"):
            meshops.rasterize_mesh(dv, dt, A, w, bad)
    with pytest.raises(ValueError, match="attrs"):
        meshops.rasterize_mesh(dv, dt, A, w, h, da[:-1])


# ------------------------------------------------------------------ vertex normals
WHEEL = ("wheel5000",)  # 5,000 faces on one vertex: sums of 2^42, beyond what fp32 holds exactly


@pytest.mark.parametrize("case", S.CLOSED + ("hemisphere",) + S.SMALL + WHEEL)
def test_vertex_normals_are_bit_identical(case):
    v, t, ref = R.normals_reference(case)
    got = meshops.vertex_normals(_dev(v), _dev(t))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    diff = int((got.cpu().numpy().view(np.int32) != ref.view(np.int32)).sum())
    print(f"{case}: {diff} differing words of {ref.size}")
    assert diff == 0


@pytest.mark.parametrize("nv", M.TILE_EDGES)
def test_vertex_normals_at_the_tile_edges(nv):
    tri = M.strip_triangles(nv)
    v = np.random.default_rng(nv).normal(0, 1, (nv, 3)).astype(np.float32)
    got = meshops.vertex_normals(_dev(v), _dev(tri)).cpu().numpy()
    ref = meshops.vertex_normals_reference(v, tri)
    assert int((got.view(np.int32) != ref.view(np.int32)).sum()) == 0


def test_vertex_normals_with_a_nan_position():
    v, t, clean = R.normals_reference("sphere")
    w = v.copy()
    w[100, 1] = np.nan
    got = meshops.vertex_normals(_dev(w), _dev(t)).cpu().numpy()
    ref = meshops.vertex_normals_reference(w, t)
    assert np.isfinite(ref).all() and (ref != clean).any()
    np.testing.assert_array_equal(got.view(np.int32), ref.view(np.int32))


# ------------------------------------------------------------------ turntable
def test_turntable():
    v, t = M.mesh("sphere")
    kw = dict(frames=5, step_deg=30.0, width=48, height=48)
    got = meshops.mesh_turntable(_dev(v), _dev(t), background=(1.0, 0.5, 0.25), **kw)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (5, 48, 48, 3)
    ref = meshops.mesh_turntable_reference(v, t, background=(1.0, 0.5, 0.25), **kw)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    Ts = meshops.turntable_transforms(v, **kw)
    for k in range(5):
        empty = meshops.rasterize_mesh_reference(v, t, Ts[k], 48, 48).face_ids < 0
        assert 0 < empty.sum() < empty.size
        assert (got[k].cpu().numpy()[empty] == [255, 128, 64]).all()
    assert anerf.mesh_turntable is meshops.mesh_turntable
    # given colours: float in [0, 1] and uint8, used as they are
    c = np.random.default_rng(2).random((len(v), 3)).astype(np.float32)
    np.testing.assert_array_equal(meshops.mesh_turntable(_dev(v), _dev(t), _dev(c), **kw).cpu().numpy(),
                                  meshops.mesh_turntable_reference(v, t, c, **kw))
    u8 = np.rint(255 * c).astype(np.uint8)
    np.testing.assert_array_equal(meshops.mesh_turntable(_dev(v), _dev(t), _dev(u8), **kw).cpu().numpy(),
                                  meshops.mesh_turntable_reference(v, t, u8, **kw))


# ------------------------------------------------------------------ integration
THR = 0.3  # (test_gpu_isosurface.py: no grid value of dm_fine_d8w256 is near it)


def test_extract_mesh_with_face_normals():
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = (torch.from_numpy(g[k]) for k in ("kps", "skts", "bones"))
    kw = dict(radius=radius, res=res, threshold=THR, keep_largest=1, smooth=2)
    for coords in ("index", "unit", "world"):
        pv, pt, pa = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, **kw)
        v, t, a = rc.extract_mesh(kps, skts, bones, coords=coords, normals="faces", **kw)
        assert len(t) > 0 and torch.equal(v.view(torch.int32), pv.view(torch.int32)) and torch.equal(t, pt)
        want = meshops.vertex_normals(v, t)
        assert torch.equal(a["normals"].view(torch.int32), want.view(torch.int32)), coords
        np.testing.assert_array_equal(want.cpu().numpy().view(np.int32),
                                      meshops.vertex_normals_reference(v, t).view(np.int32))
        # the two kinds of normal are on the same side of the surface (the gradient's are of the unsmoothed crossing of
        # a noisy density: only the side is compared -- the other winding would put nearly every vertex below 0)
        cos = (a["normals"] * pa["normals"]).sum(-1)
        print(f"{coords}: {float((cos > 0).float().mean()):.3f} of the vertices have both normals on one side")
        assert float((cos > 0).float().mean()) > 0.75, coords
        # normals=True is what it was: the gradient normals of the call without smoothing
        plain = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, radius=radius, res=res, threshold=THR,
                                keep_largest=1)
        assert torch.equal(pa["normals"], plain[2]["normals"])
    # with view="normal" the face normals give the colour query's directions
    v, t, a = rc.extract_mesh(kps, skts, bones, coords="world", normals="faces", colors=True, **kw)
    kp0 = kps.to(v.device, torch.float32).reshape(-1, 3)[0]
    inward = 0.0 - a["normals"]
    dirs = torch.where((inward == 0).all(-1, keepdim=True), kp0 - v, inward).contiguous()
    raw = rc.render_pts_radiance(v.contiguous(), dirs, kps, skts, bones)
    assert torch.equal(a["colors"], torch.sigmoid(raw[:, :3].to(torch.float32)))
    with pytest.raises(ValueError, match="faces"):
        rc.extract_mesh(kps, skts, bones, normals="vertex", **kw)


# ------------------------------------------------------------------ the C entries' guards
def test_entry_guards():
    lib = _lib.load()
    v, t, A, w, h, attrs = R.scene("soup_37x21")
    dv, dt, da = _dev(v), _dev(t), _dev(attrs)
    nv, nt = len(v), len(t)
    need = lib.anerf_mesh_raster_workspace(nv, nt, w, h)
    assert need >= 8 * w * h + 4 * nt
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    out = dict(face_ids=torch.empty((h, w), device="cuda", dtype=torch.int32),
               depth=torch.empty((h, w), device="cuda"), bary=torch.empty((h, w, 3), device="cuda"),
               image=torch.empty((h, w, 3), device="cuda"))
    Ah = np.ascontiguousarray(A)
    bg = np.full(3, 0.5, np.float32)
    import ctypes

    def call(width=w, height=h, ws_bytes=need, **null):
        o = {k: (None if k in null else _lib.ptr(x)) for k, x in out.items()}
        return lib.anerf_mesh_raster(_lib.ptr(dv), nv, _lib.ptr(dt), nt, Ah.ctypes.data_as(ctypes.c_void_p), width,
                                     height, _lib.ptr(da), 3, bg.ctypes.data_as(ctypes.c_void_p), o["face_ids"],
                                     o["depth"], o["bary"], o["image"], _lib.ptr(ws), ws_bytes,
                                     _lib.stream_handle(dv.device))
    for name in out:
        assert call(**{name: True}) == -1 and name.encode() in lib.anerf_last_error(), name
    assert call(width=0) == -1 and b"width" in lib.anerf_last_error()
    assert call(width=16385) == -1 and b"width" in lib.anerf_last_error()
    assert call(height=0) == -1 and b"height" in lib.anerf_last_error()
    assert call(ws_bytes=need - 4) == -1 and b"anerf_mesh_raster_workspace" in lib.anerf_last_error()
    assert lib.anerf_mesh_raster_workspace(nv, nt, 0, h) == 0 and b"width" in lib.anerf_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out["face_ids"].cpu().numpy(), R.reference("soup_37x21").face_ids)
    # the normals' entry
    nneed = lib.anerf_mesh_vertex_normals_workspace(nv, nt)
    nws = torch.empty(nneed, device="cuda", dtype=torch.uint8)
    nrm = torch.empty((nv, 3), device="cuda")
    args = (_lib.ptr(dv), nv, _lib.ptr(dt), nt)
    stream = _lib.stream_handle(dv.device)
    assert lib.anerf_mesh_vertex_normals(*args, None, _lib.ptr(nws), nneed, stream) == -1
    assert b"normals" in lib.anerf_last_error()
    assert lib.anerf_mesh_vertex_normals(*args, _lib.ptr(nrm), _lib.ptr(nws), nneed - 8, stream) == -1
    assert b"anerf_mesh_vertex_normals_workspace" in lib.anerf_last_error()
    assert lib.anerf_mesh_vertex_normals(*args, _lib.ptr(nrm), _lib.ptr(nws), nneed, stream) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(nrm.cpu().numpy().view(np.int32),
                                  meshops.vertex_normals_reference(v, t).view(np.int32))

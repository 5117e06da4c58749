"""CPU: the perspective rasteriser's NumPy checker (meshops.rasterize_mesh_camera_reference) against geometry -- the
float64 ray-plane hits of the rays get_rays casts -- and against the contract's properties (no cracks along the near
cut, seams drawn once, perspective-correct weights); camera_view against those rays; the C entry's argument checks,
which need no GPU.  test_gpu_mesh_raster_persp.py then holds the kernels to this checker bit for bit."""
import ctypes
import importlib

import numpy as np
import pytest

import _raster_persp_cases as P

anerf = importlib.import_module("a-nerf_amd")
meshops = importlib.import_module("a-nerf_amd.meshops")
_lib = importlib.import_module("a-nerf_amd._lib")

# Case A's largest errors of the checker against the float64 ray-plane hits, measured on the committed checker:
# 3.55e-7 for image (positions on a range of 4) and 1.17e-7 for depth (1 to 4) -- a few fp32 roundings of values up to
# 4 (2^-23 * 4 = 4.8e-7).  The bounds are eight times those; interpolating linearly on the screen instead would be off
# by 0.3 of the range (1.2) at the middle of the span, so any bound below 1e-2 of the range tells the two apart.
CASE_A_IMAGE_ERROR, CASE_A_DEPTH_ERROR = 3.55e-7, 1.17e-7
CASE_A_IMAGE_BOUND, CASE_A_DEPTH_BOUND = 8 * CASE_A_IMAGE_ERROR, 8 * CASE_A_DEPTH_ERROR


def test_case_a_is_perspective_correct_and_on_the_rays():
    sc, ref = P.scene("case_a"), P.reference("case_a")
    covered = ref.face_ids >= 0
    # 32 x 32 pixel centres: of the two columns and the two rows of centres ON the outline the tie rule keeps one each
    assert covered.sum() == 1024 and covered.any(0).sum() == 32 and covered.any(1).sum() == 32
    assert covered[9:40, 17:48].all()
    hits, t = P.case_a_hits()
    image_err = np.abs(ref.image.astype(np.float64) - hits)[covered].max()
    depth_err = np.abs(ref.depth.astype(np.float64) - t)[covered].max()
    print(f"case A: image error {image_err:.3e} (bound {CASE_A_IMAGE_BOUND:.3e}), depth error {depth_err:.3e} "
          f"(bound {CASE_A_DEPTH_BOUND:.3e})")
    assert CASE_A_IMAGE_BOUND < 1e-2 * 4 and CASE_A_DEPTH_BOUND < 1e-2 * 3
    assert image_err <= CASE_A_IMAGE_BOUND and depth_err <= CASE_A_DEPTH_BOUND
    # bary are the weights of the hit point over the ORIGINAL vertices
    v = sc["vertices"].astype(np.float64)[sc["triangles"][ref.face_ids[covered]]]
    back = (ref.bary[covered].astype(np.float64)[:, :, None] * v).sum(1)
    assert np.abs(back - hits[covered]).max() <= CASE_A_IMAGE_BOUND
    assert (ref.depth[~covered] == np.inf).all() and (ref.image[~covered] == P.BACKGROUND).all()


def test_case_b_near_cut_has_no_cracks():
    sc, ref = P.scene("case_b"), P.reference("case_b")
    n_in = np.bincount(P.in_counts(sc), minlength=4)
    assert n_in[1] > 0 and n_in[2] > 0 and n_in[0] > 0 and n_in[3] > 0
    x, z, t = P.case_b_hits()

    def inside(margin, lo, hi):
        return ((t >= lo) & (t <= hi) & (x >= P.PLANE_X[0] + margin) & (x <= P.PLANE_X[1] - margin) &
                (z >= P.PLANE_Z[0] + margin) & (z <= P.PLANE_Z[1] - margin))
    near, far = sc["near"], sc["far"]
    strict, loose = inside(0.02, 1.02 * near, 0.98 * far), inside(-0.02, 0.98 * near, 1.02 * far)
    covered = ref.face_ids >= 0
    band = (loose & ~strict).sum() / covered.sum()
    print(f"case B: {strict.sum()} strict pixels, {(strict & ~covered).sum()} empty, {(covered & ~loose).sum()} stray, "
          f"band {band:.3f}, triangles by vertices IN {n_in.tolist()}")
    assert strict.sum() > 3000
    assert not (strict & ~covered).any(), "a crack: an empty pixel inside the plane"
    assert not (covered & ~loose).any(), "a stray pixel outside the plane"
    assert band <= 0.10
    # the cut line and the far line both cross the image
    assert (t[~covered] < near).any() and (t[~covered] > far).any()
    assert ref.depth[covered].min() >= np.float32(near) * (1 - 1e-6) and ref.depth[covered].max() <= np.float32(far)


@pytest.mark.parametrize("order", P.SEAM_ORDERS)
def test_shared_edge_across_the_near_plane(order):
    """Whatever vertex order and winding the second triangle has, the two meet along the cut edge: every pixel of
    their union belongs to exactly one of them, and no row or column of the union has a gap."""
    name = "seam_pair:%d%d%d" % order
    sc, both = P.scene(name), P.reference(name)
    alone = [meshops.rasterize_mesh_camera_reference(**{**sc, "triangles": sc["triangles"][k:k + 1]}).face_ids >= 0
             for k in range(2)]
    assert alone[0].sum() > 100 and alone[1].sum() > 100
    assert not (alone[0] & alone[1]).any(), "a pixel drawn by both"
    covered = both.face_ids >= 0
    np.testing.assert_array_equal(covered, alone[0] | alone[1])
    np.testing.assert_array_equal(both.face_ids[alone[1]], 1)
    for lines in (covered, covered.T):  # (the union is convex: a crack along the shared edge would split a line)
        for line in lines:
            k = np.nonzero(line)[0]
            assert len(k) == 0 or line[k[0]:k[-1] + 1].all()
    # the first listing's result does not depend on how the second triangle is listed
    first = P.reference("seam_pair:%d%d%d" % P.SEAM_ORDERS[0])
    np.testing.assert_array_equal(both.face_ids, first.face_ids)
    np.testing.assert_array_equal(both.depth[alone[0]], first.depth[alone[0]])


def test_seam_between_the_sub_triangles_is_drawn_once():
    sc, ref = P.scene("seam_diagonal"), P.reference("seam_diagonal")
    assert P.in_counts(sc).tolist() == [2]
    k = np.arange(5, 20)
    assert (ref.face_ids[k, k] == 0).all(), "pixel centres on the seam q0 - q2 are empty"
    # ... and carry the values of the plane there, as their neighbours do: the triangle's plane through the rays
    d, o = P.ray_dirs(sc)
    v = sc["vertices"].astype(np.float64)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    t = (n @ (v[0] - o)) / (d @ n)
    covered = ref.face_ids >= 0
    assert np.abs(ref.depth[covered] - t[covered]).max() < 2e-6
    hit = ref.bary[covered].astype(np.float64) @ v
    assert np.abs(hit - (o + t[..., None] * d)[covered]).max() < 4e-6
    # a convex polygon: no line of it has a gap
    for lines in (covered, covered.T):
        for line in lines:
            j = np.nonzero(line)[0]
            assert len(j) == 0 or line[j[0]:j[-1] + 1].all()


@pytest.mark.parametrize("name", ["case_a", "seam_diagonal", "cube_small"])
def test_rows_sum_to_one(name):
    ref = P.reference(name)
    covered = ref.face_ids >= 0
    assert covered.any()
    s = ref.bary[covered].astype(np.float64).sum(-1)
    assert np.abs(s - 1).max() <= 4 * 2.0 ** -23
    assert (ref.bary[~covered] == 0).all()


@pytest.mark.parametrize("kind", P.NOTHING)
def test_triangles_that_draw_nothing(kind):
    ref = P.reference("nothing:" + kind)
    assert (ref.face_ids == -1).all() and (ref.depth == np.inf).all() and (ref.bary == 0).all()
    assert (ref.image == P.BACKGROUND).all()


def test_equal_depths_go_to_the_smaller_id():
    ref = P.reference("ties")
    assert sorted(np.unique(ref.face_ids)) == [-1, 0, 1]


def test_cube_takes_both_paths():
    """The two sizes of the cube are on either side of RASTER_SMALL_PIXELS (test_gpu_mesh_raster_persp.py draws both),
    and the near plane cuts triangles of it."""
    assert (P.box_pixels("cube_large") > meshops.RASTER_SMALL_PIXELS).all()
    assert (P.box_pixels("cube_small") <= meshops.RASTER_SMALL_PIXELS).all()
    n_in = P.in_counts(P.scene("cube_large"))
    assert ((n_in == 1) | (n_in == 2)).any()
    big, small = P.reference("cube_large"), P.reference("cube_small")
    assert (big.face_ids >= 0).mean() > 0.5 and (small.face_ids >= 0).mean() > 0.5
    assert set(np.unique(small.face_ids)) <= set(np.unique(big.face_ids))


def test_soup_has_every_kind():
    sc, ref = P.scene("soup"), P.reference("soup")
    n_in = np.bincount(P.in_counts(sc), minlength=4)
    assert (n_in > 0).all()
    covered = ref.face_ids >= 0
    assert 0.2 < covered.mean() < 0.8
    assert ref.depth[covered].max() <= np.float32(sc["far"]) and np.isfinite(ref.image).all()
    for k in (5, 9, 11, 12):
        assert not (ref.face_ids == k).any()  # repeated (the smaller id wins) and degenerate triangles


# ------------------------------------------------------------------ camera_view
def test_camera_view_is_the_camera_of_the_rays():
    R = P.rot_y(0.7) @ P.rot_x(-0.4)
    c2w = P.camera(R, (0.3, -1.2, 2.5))
    H, W, focal, center = 30, 40, (37.0, 41.5), (18.25, 16.5)
    V, K = meshops.camera_view(c2w, H, W, focal, center)
    assert V.dtype == np.float32 and V.shape == (3, 4) and K.dtype == np.float32 and K.shape == (4,)
    np.testing.assert_array_equal(K, np.array([37.0, 41.5, 18.75, 17.0], np.float32))
    sc = dict(H=H, W=W, focal=focal, center=center, c2w=c2w)
    d, o = P.ray_dirs(sc)
    for t in (0.5, 3.0):
        cam = (o + t * d) @ V[:, :3].astype(np.float64).T + V[:, 3].astype(np.float64)
        j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        np.testing.assert_allclose(K[0] * cam[..., 0] / cam[..., 2] + K[2], i + 0.5, atol=1e-4)
        np.testing.assert_allclose(K[1] * cam[..., 1] / cam[..., 2] + K[3], j + 0.5, atol=1e-4)
        np.testing.assert_allclose(cam[..., 2], t, rtol=1e-6)
    # without a centre: W / 2, H / 2; one focal for both; a [3, 4] c2w and a tensor are taken too
    import torch
    V2, K2 = meshops.camera_view(torch.from_numpy(c2w[:3]), H, W, 37.0)
    np.testing.assert_array_equal(V2, V)
    np.testing.assert_array_equal(K2, np.array([37.0, 37.0, 20.5, 15.5], np.float32))
    with pytest.raises(ValueError, match="c2w"):
        meshops.camera_view(np.eye(3), H, W, 37.0)
    with pytest.raises(ValueError, match="focal"):
        meshops.camera_view(c2w, H, W, (1.0, 2.0, 3.0))
    assert anerf.camera_view is meshops.camera_view
    assert anerf.rasterize_mesh_camera is meshops.rasterize_mesh_camera


def test_near_and_far_defaults():
    sc = dict(P.scene("cube_small"))
    v = sc["vertices"].astype(np.float64)
    D = np.linalg.norm(sc["c2w"][:3, 3] - 0.5 * (v.min(0) + v.max(0)))
    rho = 0.5 * np.linalg.norm(v.max(0) - v.min(0))
    near, far = max(D - rho, 1e-3 * rho), D + rho
    given = meshops.rasterize_mesh_camera_reference(**{**sc, "near": near, "far": far})
    derived = meshops.rasterize_mesh_camera_reference(**{**sc, "near": None, "far": None})
    for g, d in zip(given, derived):
        np.testing.assert_array_equal(g, d)
    assert (derived.face_ids >= 0).any()
    half = meshops.rasterize_mesh_camera_reference(**{**sc, "near": None})  # far as given, near derived
    assert half.depth[half.face_ids >= 0].max() <= np.float32(sc["far"])
    # the camera inside the box: near falls back to 1e-3 rho
    inside = {**sc, "c2w": P.camera(), "near": None, "far": None}
    assert meshops._camera_range(meshops._bounding_box(sc["vertices"]), inside["c2w"], None, None, "t")[0] == \
        np.float32(1e-3 * rho)
    for bad in (dict(near=0.0), dict(near=-1.0), dict(near=np.nan), dict(far=np.inf), dict(near=2.0, far=1.0)):
        with pytest.raises(ValueError, match="near|far"):
            meshops.rasterize_mesh_camera_reference(**{**sc, **bad})
    with pytest.raises(ValueError, match="fx"):
        meshops.rasterize_mesh_camera_reference(**{**sc, "focal": 0.0})


def test_render_mesh_views_reference():
    kw = P.views()
    out = P.views_reference()
    F_, H, W = len(kw["c2ws"]), kw["H"], kw["W"]
    assert isinstance(out, meshops.MeshViews)
    assert out.rgb.shape == (F_, H, W, 3) and out.rgb.dtype == np.uint8
    assert out.depth.shape == (F_, H, W) and out.depth.dtype == np.float32
    assert out.mask.shape == (F_, H, W) and out.mask.dtype == bool
    for k in range(F_):
        one = meshops.rasterize_mesh_camera_reference(kw["vertices"], kw["triangles"], kw["c2ws"][k], H, W,
                                                      kw["focal"][k], kw["centers"][k], attrs=kw["colors"],
                                                      background=kw["background"])
        assert 0 < out.mask[k].sum() < H * W
        np.testing.assert_array_equal(out.mask[k], one.face_ids >= 0)
        np.testing.assert_array_equal(out.depth[k], one.depth)
        np.testing.assert_array_equal(out.rgb[k], meshops._to_uint8_reference(one.image))
        assert (out.rgb[k][~out.mask[k]] == [255, 128, 64]).all() and np.isinf(out.depth[k][~out.mask[k]]).all()
    # the forms of focal: one value, [F], [F, 2]
    base = {**kw, "centers": None, "colors": None}
    a = meshops.render_mesh_views_reference(**{**base, "focal": 21.0})
    b = meshops.render_mesh_views_reference(**{**base, "focal": np.full(F_, 21.0)})
    c = meshops.render_mesh_views_reference(**{**base, "focal": np.full((F_, 2), 21.0)})
    for x, y, z in zip(a, b, c):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
    u8 = np.rint(255 * kw["colors"]).astype(np.uint8)  # uint8 colours, as a PLY's
    assert meshops.render_mesh_views_reference(**{**kw, "colors": u8}).rgb.shape == (F_, H, W, 3)
    with pytest.raises(ValueError, match="focal"):
        meshops.render_mesh_views_reference(**{**kw, "focal": np.ones(F_ + 1)})
    with pytest.raises(ValueError, match="centers"):
        meshops.render_mesh_views_reference(**{**kw, "centers": np.ones((F_, 3))})
    with pytest.raises(ValueError, match="c2ws"):
        meshops.render_mesh_views_reference(**{**kw, "c2ws": kw["c2ws"][0]})


# ------------------------------------------------------------------ the C entry's argument checks (no GPU needed)
def test_c_abi_validation():
    lib = _lib.load()
    assert lib.anerf_abi_version() == 26
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    V = np.eye(3, 4, dtype=np.float32)
    K = np.array([30.0, 30.0, 8.5, 8.5], np.float32)
    bg = np.zeros(3, np.float32)

    def err():
        return lib.anerf_last_error()

    def call(vertices=p, nv=3, triangles=p, nt=1, view=V, intr=K, near=0.5, far=10.0, width=4, height=4, attrs=p,
             nch=3, background=bg, face_ids=p, depth=p, bary=p, image=p, ws=p, ws_bytes=1 << 20):
        def host(x):
            return None if x is None else x.ctypes.data_as(ctypes.c_void_p)
        return lib.anerf_mesh_raster_persp(vertices, nv, triangles, nt, host(view), host(intr), near, far, width,
                                           height, attrs, nch, host(background), face_ids, depth, bary, image, ws,
                                           ws_bytes, None)
    # (no call below reaches a launch: each is refused, ANERF_EINVAL = -1, with the argument's name in the message)
    for kw, word in ((dict(near=0.0), b"near"), (dict(near=-1.0), b"near"), (dict(near=float("nan")), b"near"),
                     (dict(near=float("inf")), b"near"), (dict(far=float("inf")), b"far"),
                     (dict(far=float("nan")), b"far"), (dict(near=2.0, far=1.0), b"far"),
                     (dict(intr=np.array([np.nan, 30, 8, 8], np.float32)), b"fx"),
                     (dict(intr=np.array([30, np.inf, 8, 8], np.float32)), b"fy"),
                     (dict(intr=np.array([30, 30, np.nan, 8], np.float32)), b"cx"),
                     (dict(intr=np.array([30, 30, 8, -np.inf], np.float32)), b"cy"),
                     (dict(intr=np.array([0, 30, 8, 8], np.float32)), b"fx"),
                     (dict(intr=np.array([30, 0, 8, 8], np.float32)), b"fy"),
                     (dict(view=None), b"view"), (dict(intr=None), b"intrinsics"),
                     (dict(width=0), b"width"), (dict(width=16385), b"width"), (dict(height=0), b"height"),
                     (dict(height=16385), b"height"), (dict(nv=-1), b"n_vertices"), (dict(nt=1 << 31), b"n_tri"),
                     (dict(nch=-1), b"n_channels"), (dict(nch=9), b"n_channels"), (dict(vertices=None), b"vertices"),
                     (dict(triangles=None), b"triangles"), (dict(face_ids=None), b"face_ids"),
                     (dict(depth=None), b"depth"), (dict(bary=None), b"bary"), (dict(attrs=None), b"attrs"),
                     (dict(background=None), b"background"), (dict(image=None), b"image"),
                     (dict(ws=None), b"workspace"), (dict(ws=ctypes.c_void_p(p.value + 4)), b"aligned"),
                     (dict(ws_bytes=8 * 16 + 8 + 4 - 1), b"anerf_mesh_raster_persp_workspace")):
        assert call(**kw) == -1, kw
        assert word in err() and b"anerf_mesh_raster_persp" in err(), (kw, err())
    # far == near is a valid range
    assert call(near=1.0, far=1.0, width=0) == -1 and b"width" in err()
    need = lib.anerf_mesh_raster_persp_workspace(3, 1, 4, 4)
    assert need == 8 * 16 + 8 + 4 == lib.anerf_mesh_raster_workspace(3, 1, 4, 4)
    for bad in ((-1, 1, 4, 4), (3, 1 << 31, 4, 4), (3, 1, 0, 4), (3, 1, 4, 16385)):
        assert lib.anerf_mesh_raster_persp_workspace(*bad) == 0
        assert b"anerf_mesh_raster_persp_workspace" in err()


def test_argument_errors_come_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the argument checks must come before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    sc = P.scene("cube_small")
    for bad, word in ((dict(triangles=sc["triangles"] + 100), "outside"), (dict(W=0), "width"), (dict(H=16385), "height"),
                      (dict(attrs=sc["attrs"][:-1]), "attrs"), (dict(near=-1.0), "near"), (dict(far=0.5), "far"),
                      (dict(focal=0.0), "fx"), (dict(c2w=np.eye(2)), "c2w")):
        with pytest.raises(ValueError, match=word):
            meshops.rasterize_mesh_camera(**{**sc, **bad})
    kw = P.views()
    with pytest.raises(ValueError, match="focal"):
        meshops.render_mesh_views(**{**kw, "focal": np.ones(7)})
    with pytest.raises(ValueError, match="outside"):
        meshops.render_mesh_views(**{**kw, "triangles": kw["triangles"] + 100})

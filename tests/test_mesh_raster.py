"""CPU: the NumPy checkers of the rasteriser and of the face-accumulated vertex normals (meshops'
rasterize_mesh_reference, vertex_normals_reference, turntable_transforms), held to properties that do not come from them: exact-once coverage of
meshes whose vertices lie on pixel centres, the depth rule, a float64 accumulation, the sphere's radial directions.
The kernels are held to these checkers, bit for bit, in test_gpu_mesh_raster.py."""
import importlib
import os
import re

import numpy as np
import pytest

import _mesh_cases as M
import _raster_cases as R
import _smooth_cases as S
from _iso_cases import SPHERE_C

meshops = importlib.import_module("a-nerf_amd.meshops")
_lib = importlib.import_module("a-nerf_amd._lib")


def _coverage_count(v, t, size=33):
    """How many triangles cover each pixel: every triangle rasterised on its own."""
    n = np.zeros((size, size), np.int64)
    for k in range(len(t)):
        n += meshops.rasterize_mesh_reference(v, t[k:k + 1], R.IDENTITY, size, size).face_ids >= 0
    return n


@pytest.mark.parametrize("mesh", ["fan", "grid"])
@pytest.mark.parametrize("reverse", [False, True])
def test_shared_edges_are_drawn_exactly_once(mesh, reverse):
    """Every vertex is on a pixel centre, so pixel centres lie on edges and vertices throughout: each of the 1,024
    pixels the tie rule gives the square is covered once, the 65 it leaves out (two sides of the rim) never."""
    v, t = R.fan_mesh() if mesh == "fan" else R.grid_mesh()
    if reverse:
        t = R.reverse(t)
    n = _coverage_count(v, t)
    assert n.max() == 1
    assert int((n == 1).sum()) == 1024 and int((n == 0).sum()) == 65
    assert (n[1:-1, 1:-1] == 1).all()
    # the whole list at once draws the same pixels
    whole = meshops.rasterize_mesh_reference(v, t, R.IDENTITY, 33, 33)
    np.testing.assert_array_equal(whole.face_ids >= 0, n == 1)


def test_winding_does_not_change_coverage():
    for name in ("soup_37x21", "soup_257x255", "off_image"):
        v, t, A, w, h, _ = R.scene(name)
        for k in range(0, len(t), 7):
            a = meshops.rasterize_mesh_reference(v, t[k:k + 1], A, w, h)
            b = meshops.rasterize_mesh_reference(v, R.reverse(t[k:k + 1]), A, w, h)
            np.testing.assert_array_equal(a.face_ids, b.face_ids)
            np.testing.assert_allclose(a.depth, b.depth, atol=1e-6)  # (the vertices swap roles: an ulp)


def test_depth_keys():
    # coplanar duplicates: the smaller id of the two
    out = R.reference("duplicates")
    ids = set(np.unique(out.face_ids).tolist())
    assert {-1, 1} <= ids and not ids & {2, 3}  # 0 hides its copy 3, 1 its copy 2
    # two parallel quads: the nearer one wherever it is, whatever the order of the list
    a, b = R.reference("quads"), R.reference("quads_swapped")
    np.testing.assert_array_equal(a.depth.view(np.int32), b.depth.view(np.int32))
    order = np.array([2, 0, 3, 1])  # quads_swapped's triangle k is quads' triangle order[k]
    np.testing.assert_array_equal(np.where(b.face_ids >= 0, order[b.face_ids], -1), a.face_ids)
    near = a.depth < 0.45
    np.testing.assert_allclose(a.depth[near], 0.3, atol=1e-6)
    assert near.sum() > 300 and (a.face_ids[near] >= 2).all()
    overlap = near & (np.arange(33)[None, :] < 19) & (np.arange(27)[:, None] < 17)
    assert overlap.sum() > 50  # pixels both quads cover
    np.testing.assert_allclose(a.depth[(a.face_ids >= 0) & ~near], 0.6, atol=1e-6)


def test_empty_pixels_barycentrics_and_attributes():
    out = R.reference("soup_37x21")
    v, t, A, w, h, attrs = R.scene("soup_37x21")
    hit = out.face_ids >= 0
    assert 0 < hit.sum() < hit.size
    assert (out.depth[~hit] == np.inf).all() and (out.bary[~hit] == 0).all()
    assert (out.image[~hit] == np.float32(R.BACKGROUND)).all()
    assert ((out.depth[hit] >= 0) & (out.depth[hit] <= 1)).all()
    np.testing.assert_allclose(out.bary[hit].sum(-1), 1, atol=1e-6)
    assert (out.bary[hit] > -1e-6).all()
    # against float64: the pixel's centre from the barycentrics, the attributes interpolated
    s = (np.concatenate([v, np.ones((len(v), 1))], 1).astype(np.float64) @ A.astype(np.float64).T)[t[out.face_ids[hit]]]
    centre = np.einsum("nk,nkc->nc", out.bary[hit].astype(np.float64), s)
    jj, ii = np.nonzero(hit)
    np.testing.assert_allclose(centre[:, 0], ii + 0.5, atol=0.02)  # (the snap moves a vertex by up to 1 / 512 pixel)
    np.testing.assert_allclose(centre[:, 1], jj + 0.5, atol=0.02)
    np.testing.assert_allclose(centre[:, 2], out.depth[hit], atol=1e-3)
    want = np.einsum("nk,nkc->nc", out.bary[hit].astype(np.float64), attrs[t[out.face_ids[hit]]].astype(np.float64))
    np.testing.assert_allclose(out.image[hit], want, atol=1e-6)


def test_scenes_draw_what_they_are_for():
    assert (R.reference("no_triangles").face_ids == -1).all()
    assert set(np.unique(R.reference("degenerate").face_ids).tolist()) == {-1, 4}
    assert set(np.unique(R.reference("bad_vertices").face_ids).tolist()) == {-1, 5, 6}
    off = R.reference("off_image").face_ids
    assert set(np.unique(off).tolist()) == {-1, 0, 2, 4, 6, 8, 10}  # the six across a border; none of those outside
    d = R.reference("depth_range")
    hit = d.face_ids >= 0
    assert {0, 1} <= set(np.unique(d.face_ids).tolist()) and d.depth[hit].min() < 0.1 and d.depth[hit].max() > 0.85
    assert (R.reference("sliver_tall").face_ids >= 0).sum() == 1000  # the apex is above a column of centres
    assert R.reference("no_attrs").image is None
    assert R.reference("eight_channels").image.shape == (21, 37, 8)
    assert (R.reference("full_1024").face_ids == 0).all()
    assert len(np.unique(R.reference("cube_512").face_ids)) == 7  # three faces of the cube, two triangles each


def test_argument_errors():
    v, t, A, w, h, attrs = R.scene("soup_37x21")
    for fn in (meshops.rasterize_mesh_reference,):
        with pytest.raises(ValueError, match="outside"):
            fn(v, t + 100, A, w, h)
        for bad in (0, 16385, -3):
            with pytest.raises(ValueError, match="width"):
                fn(v, t, A, bad, h)
            with pytest.raises(ValueError, match="height"):
                fn(v, t, A, w, bad)
        with pytest.raises(ValueError, match="attrs"):
            fn(v, t, A, w, h, attrs[:-1])
        with pytest.raises(ValueError, match="channels"):
            fn(v, t, A, w, h, np.zeros((len(v), 9), np.float32))
        with pytest.raises(ValueError, match="transform"):
            fn(v, t, np.eye(4), w, h)


def test_threshold_constant_matches_the_header():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "anerf.h")) as f:
        val = int(re.search(r"#define ANERF_RASTER_SMALL_PIXELS (\d+)", f.read()).group(1))
    assert meshops.RASTER_SMALL_PIXELS == _lib.ANERF_RASTER_SMALL_PIXELS == val


# ------------------------------------------------------------------ vertex normals
def _float64_sums(v, t):
    p = np.asarray(v, np.float64)
    n = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    n /= np.maximum(np.linalg.norm(n, axis=1), 1e-8)[:, None]
    acc = np.zeros_like(p)
    for k in range(3):
        np.add.at(acc, t[:, k], n)
    return acc


@pytest.mark.parametrize("case", S.CLOSED)
def test_vertex_normals_against_float64(case):
    v, t, n = R.normals_reference(case)
    assert n.dtype == np.float32 and n.shape == v.shape
    acc = _float64_sums(v, t)
    ln = np.linalg.norm(acc, axis=1)
    ok = ln > 0.1
    assert ok.sum() > 0.9 * len(v)
    cos = np.einsum("ij,ij->i", n[ok].astype(np.float64), acc[ok] / ln[ok, None])
    cos /= np.linalg.norm(n[ok].astype(np.float64), axis=1)
    angle = np.arccos(np.clip(cos, -1, 1))
    # (arccos near 1 resolves 1.5e-8: measure the angle by the cross product instead)
    angle = np.arcsin(np.clip(np.linalg.norm(np.cross(n[ok].astype(np.float64), acc[ok] / ln[ok, None]), axis=1), 0, 1))
    print(f"{case}: largest angle {angle.max():.3g} rad over {ok.sum()} vertices")
    assert (cos > 0).all() and angle.max() <= 1e-4
    np.testing.assert_allclose(np.linalg.norm(n[ok], axis=1), 1, atol=1e-6)


def test_sphere_normals_are_radial_and_point_outward():
    v, t, n = R.normals_reference("sphere")
    radial = v.astype(np.float64) - SPHERE_C
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    cos = np.einsum("ij,ij->i", n.astype(np.float64), radial)
    assert (cos > 0).all() and np.arccos(np.clip(cos, -1, 1)).max() < 0.1


def test_vertex_normals_small_cases():
    for case in S.SMALL:
        v, t, n = R.normals_reference(case)
        assert n.shape == v.shape and np.isfinite(n).all()
    v, t, n = R.normals_reference("one_triangle")
    unused = np.setdiff1d(np.arange(len(v)), t.reshape(-1))
    assert (n[unused] == 0).all() and (np.abs(np.linalg.norm(n[t[0]], axis=1) - 1) < 1e-6).all()
    v, t, n = R.normals_reference("duplicated")  # twice the same face: the same direction
    one = meshops.vertex_normals_reference(v, t[:1])
    np.testing.assert_allclose(n, one, atol=1e-7)
    # a NaN position: its faces contribute nothing, the others' normals stand
    v, t, n = R.normals_reference("sphere")
    w = v.copy()
    w[100] = np.nan
    m = meshops.vertex_normals_reference(w, t)
    assert np.isfinite(m).all()
    far = ~np.isin(np.arange(len(v)), t[(t == 100).any(1)].reshape(-1))
    np.testing.assert_array_equal(m[far].view(np.int32), n[far].view(np.int32))
    with pytest.raises(ValueError, match="outside"):
        meshops.vertex_normals_reference(v, t + len(v))


# ------------------------------------------------------------------ turntable framing
def test_turntable_transforms():
    v, t = M.mesh("sphere")
    T = meshops.turntable_transforms(v, 91, 4.0, 64, 48)
    assert T.shape == (91, 3, 4) and T.dtype == np.float32
    np.testing.assert_allclose(T[90], T[0], atol=1e-4)  # 360 degrees
    s = np.concatenate([v, np.ones((len(v), 1))], 1).astype(np.float64) @ T[13].astype(np.float64).T
    lo, hi = s.min(0), s.max(0)
    # the mesh's height (its extent along up) fills 1 / 1.2 of the image's WIDTH in pixels, centred; depths in (0, 1)
    np.testing.assert_allclose(hi[1] - lo[1], 64 / 1.2, rtol=1e-5)
    np.testing.assert_allclose(0.5 * (hi[1] + lo[1]), 24, atol=1e-3)
    assert 0.1 <= lo[2] and hi[2] <= 0.9
    # up is up: a larger z is a smaller pixel y; frame 0 looks along +y with x to the right
    np.testing.assert_allclose(T[0][:, :3] / np.linalg.norm(T[0][:, :3], axis=1)[:, None],
                               [[1, 0, 0], [0, 0, -1], [0, 1, 0]], atol=1e-6)
    # another up axis, a mesh without extent, no vertices
    U = meshops.turntable_transforms(v, 2, 90.0, 32, 32, up=(0, 1, 0))
    assert np.isfinite(U).all() and abs(U[0][1, 1]) > 1 and abs(U[0][1, 2]) < 1e-6
    assert np.isfinite(meshops.turntable_transforms(np.zeros((3, 3)), 1)).all()
    assert np.isfinite(meshops.turntable_transforms(np.zeros((0, 3)), 1)).all()
    with pytest.raises(ValueError, match="up"):
        meshops.turntable_transforms(v, 1, up=(0, 0, 0))


def test_turntable_reference_frames():
    v, t = M.mesh("sphere")
    f = meshops.mesh_turntable_reference(v, t, frames=2, step_deg=90.0, width=24, height=24, background=(1.0, 0.5, 0.0))
    assert f.shape == (2, 24, 24, 3) and f.dtype == np.uint8
    ids = meshops.rasterize_mesh_reference(v, t, meshops.turntable_transforms(v, 2, 90.0, 24, 24)[1], 24, 24).face_ids
    assert (f[1][ids < 0] == [255, 128, 0]).all() and 0 < (ids >= 0).sum() < ids.size
    # coloured by normal: the pixel in the middle of frame 0 faces the camera at -y: 0.5 n + 0.5 = (0.5, 0, 0.5)
    assert np.abs(f[0][12, 12].astype(int) - [128, 0, 128]).max() <= 12

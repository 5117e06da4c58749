"""CPU: the vertex-normal contract of isosurface.py on its NumPy checker (isosurface_reference(normals=True)), and the
PLY writer / reader with per-vertex normals and colours.

The device kernel is compared with the checker in test_gpu_mesh_attrs.py; here the checker itself is held to things
that do not depend on it: an analytic surface (the sphere's radial direction) and the reference viewer's own
face-accumulated normals (tests/golden/mesh_normals_ref.npz, written by tests/golden/make_mesh_normals_golden.py
from render_mesh.py:35-53 compute_normal)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import _iso_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
anerf = importlib.import_module("a-nerf_amd")
iso = importlib.import_module("a-nerf_amd.isosurface")
_lib = importlib.import_module("a-nerf_amd._lib")

VIEWER_FIELDS = {"sphere_field": 0.0, "torus_field": 0.0, "two_spheres_field": 0.0, "blobs_field": 0.5}


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def test_package_exports():
    assert anerf.read_ply is iso.read_ply and anerf.mesh_from_grid is iso.mesh_from_grid
    assert hasattr(anerf.RayCaster, "render_pts_radiance")
    for name in ("anerf_isosurface_normals", "anerf_radiance_points"):
        assert name in _lib.SIGNATURES


# ------------------------------------------------------------------ 1. an analytic surface
def test_checker_normals_on_the_sphere_are_radial():
    v, t, n = iso.isosurface_reference(C.sphere_field(), 0.0, normals=True)
    rv, rt = C.reference("sphere_field")
    np.testing.assert_array_equal(v, rv)  # (the flag changes neither the vertices nor the triangles)
    np.testing.assert_array_equal(t, rt)
    assert n.dtype == np.float32 and n.shape == v.shape
    np.testing.assert_allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=2e-7)
    c = _cos(n, v.astype(np.float64) - C.SPHERE_C)  # dense (inside) to empty: outward
    print(f"sphere: min cos(normal, radial) {c.min():.6f} over {len(v)} vertices")
    assert c.min() >= 0.9999


# ------------------------------------------------------------------ 2. the reference viewer's normals
@pytest.mark.parametrize("name", list(VIEWER_FIELDS))
def test_checker_normals_against_the_viewer(name):
    z = np.load(os.path.join(HERE, "golden", "mesh_normals_ref.npz"), allow_pickle=False)
    thr = VIEWER_FIELDS[name]
    assert float(z[name + "_threshold"]) == thr
    v, t, n = iso.isosurface_reference(getattr(C, name)(), thr, normals=True)
    ref = z[name]
    assert ref.shape == n.shape
    c = _cos(n, ref)
    print(f"{name}: min cos(gradient normal, face-accumulated normal) {c.min():.4f} over {len(v)} vertices")
    assert c.min() >= 0.95


# ------------------------------------------------------------------ 3. flags
def test_flip_negates_the_normals():
    f = C.relu_field()
    v0, t0, n0 = iso.isosurface_reference(f, 0.25, relu=True, normals=True)
    v1, t1, n1 = iso.isosurface_reference(f, 0.25, relu=True, flip=True, normals=True)
    np.testing.assert_array_equal(v0, v1)
    np.testing.assert_array_equal(t1, t0[:, [0, 2, 1]])
    np.testing.assert_array_equal(n1, -n0)
    assert np.abs(n0).max() > 0.5
    # the clamp is part of the values the gradient reads
    _, _, nc = iso.isosurface_reference(np.maximum(f, 0), 0.25, normals=True)
    np.testing.assert_array_equal(nc, n0)
    _, _, nr = iso.isosurface_reference(f, 0.25, normals=True)
    assert np.abs(nr - n0).max() > 0.05


def test_world_normals_are_permuted_and_agree_with_the_winding():
    """mesh_from_grid's frames on the checker's arrays: "world" swaps axes 0 and 1 (a reflection), the winding is
    reversed for it and the normal is a vector that just follows the swap -- both then point outward."""
    v, t, n = iso.isosurface_reference(C.sphere_field(), 0.0, normals=True)
    vf, tf, nf = iso.isosurface_reference(C.sphere_field(), 0.0, flip=True, normals=True)  # the winding flag of "world"
    vw, tw, nw = vf[:, [1, 0, 2]], tf, (0.0 - nf[:, [1, 0, 2]])
    np.testing.assert_array_equal(nw, n[:, [1, 0, 2]])
    assert C.signed_volume(vw, tw) > 0 and C.signed_volume(v, t) > 0
    # winding and normals agree, face by face, in both frames
    for vv, tt, nn in ((v, t, n), (vw, tw, nw)):
        p = vv.astype(np.float64)[tt.astype(np.int64)]
        face = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        keep = np.linalg.norm(face, axis=1) > 1e-9
        assert (_cos(face[keep], nn.astype(np.float64)[tt.astype(np.int64)].sum(1)[keep]) > 0.9).all()


def test_zero_gradient_gives_zero_normals():
    # the vertex on edge (1,1,1)-(2,1,1) of this field: the central differences around both ends cancel
    f = np.zeros((4, 3, 3), np.float32)
    f[0], f[1], f[2], f[3] = 1.0, 0.0, 1.0, 0.0
    v, t, n = iso.isosurface_reference(f, 0.5, normals=True)
    assert len(v) > 0
    inner = (v[:, 0] > 1) & (v[:, 0] < 2)
    assert inner.any() and (n[inner] == 0).all() and not np.signbit(n[inner]).any()
    assert (np.abs(n[~inner]).max(axis=1) == 1).all()  # (one-sided differences at the first and last row: +-e_0)


def test_nan_samples_follow_the_contract():
    """A NaN stays a NaN in the gradient: a vertex whose G has a NaN component gets (0, 0, 0), every other vertex the
    normal of the NaN-free field -- bit for bit where no NaN enters its stencil."""
    f, clean = C.nan_field().copy(), C.sphere_field()
    # one more NaN two steps outside the surface on the grid line through (., 7, 7): (1, 7, 7) is the outside end of
    # a crossing edge, and its central difference along axis 0 reads (0, 7, 7)
    assert clean[2, 7, 7] > 0 > clean[1, 7, 7]
    f[0, 7, 7] = np.nan
    v, t, n = iso.isosurface_reference(f, 0.0, normals=True)
    vc, tc, ncl = iso.isosurface_reference(clean, 0.0, normals=True)
    np.testing.assert_array_equal(v, vc)  # (no NaN next to an inside sample: the same mesh)
    np.testing.assert_array_equal(t, tc)
    assert np.isfinite(n).all()
    changed = (n != ncl).any(axis=1)
    print(f"nan field: {int(changed.sum())} of {len(v)} normals touched by a NaN sample")
    assert (n[changed] == 0).all()
    on_edge = (v[:, 1] == 7) & (v[:, 2] == 7) & (v[:, 0] > 1) & (v[:, 0] < 2)
    assert on_edge.sum() == 1 and changed[on_edge].all()
    # every touched vertex has a NaN within its stencil (the two edge ends and their six neighbours each)
    nan_at = np.argwhere(np.isnan(f))
    for p in v[changed]:
        assert (np.abs(nan_at - p).max(axis=1) <= 2).any(), p
    with np.errstate(invalid="ignore"):
        vr, tr, nr = iso.isosurface_reference(f, 1.0, relu=True, normals=True)  # (the clamp keeps a NaN a NaN)
    assert len(vr) > 0 and np.isfinite(nr).all()


def test_normals_of_an_empty_mesh():
    for shape in ((1, 5, 5), (5, 5, 5)):
        out = iso.isosurface_reference(np.zeros(shape, np.float32), 0.5, normals=True)
        assert [a.shape for a in out] == [(0, 3)] * 3 and out[2].dtype == np.float32


# ------------------------------------------------------------------ 4. PLY
def _old_ply_bytes(v, t):
    """The file of the plain layout, assembled by hand: header, float x y z rows, (uchar 3, int32 x 3) faces."""
    v = np.ascontiguousarray(v, "<f4").reshape(-1, 3)
    t = np.ascontiguousarray(t, "<i4").reshape(-1, 3)
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    faces = b"".join(b"\x03" + row.tobytes() for row in t)
    return head + v.tobytes() + faces


def test_plain_ply_is_byte_identical_to_the_old_layout(tmp_path):
    v, t = C.reference("sphere_field")
    path = str(tmp_path / "plain.ply")
    iso.write_ply(path, v, t)
    assert open(path, "rb").read() == _old_ply_bytes(v, t)
    iso.write_ply(path, v, t, normals=None, colors=None)
    assert open(path, "rb").read() == _old_ply_bytes(v, t)
    iso.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert open(path, "rb").read() == _old_ply_bytes(np.zeros((0, 3)), np.zeros((0, 3)))


def test_ply_extras_round_trip(tmp_path):
    v, t, n = iso.isosurface_reference(C.sphere_field(), 0.0, normals=True)
    rng = np.random.default_rng(5)
    c = rng.random((len(v), 3)).astype(np.float32)
    c[0] = (-0.2, 1.3, 0.5)       # clipped
    c[1] = (0.0, 1.0, 0.5 / 255)  # rint: half to even
    want = np.clip(np.rint(np.float32(255) * c), 0, 255).astype(np.uint8)
    assert want[0].tolist() == [0, 255, 128] and want[1].tolist() == [0, 255, 0]
    path = str(tmp_path / "full.ply")
    iso.write_ply(path, v, t, normals=n, colors=c)
    blob = open(path, "rb").read()
    head = blob[:blob.index(b"end_header\n")].decode("ascii").split("\n")
    assert head[2:] == [f"element vertex {len(v)}", "property float x", "property float y", "property float z",
                        "property float nx", "property float ny", "property float nz", "property uchar red",
                        "property uchar green", "property uchar blue", f"element face {len(t)}",
                        "property list uchar int vertex_indices", ""]
    assert len(blob) == blob.index(b"end_header\n") + 11 + 27 * len(v) + 13 * len(t)
    v2, t2, a2 = iso.read_ply(path, attributes=True)
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(t2, t)
    assert sorted(a2) == ["colors", "normals"] and a2["normals"].dtype == np.float32 and a2["colors"].dtype == np.uint8
    np.testing.assert_array_equal(a2["normals"], n)
    np.testing.assert_array_equal(a2["colors"], want)
    # plain read_ply of the same file: the same mesh
    v3, t3 = iso.read_ply(path)
    np.testing.assert_array_equal(v3, v)
    np.testing.assert_array_equal(t3, t)
    # tensors, uint8 colours as they are, one extra only
    iso.write_ply(path, torch.from_numpy(v.copy()), torch.from_numpy(t.copy()), colors=torch.from_numpy(want.copy()))
    v4, t4, a4 = iso.read_ply(path, attributes=True)
    assert sorted(a4) == ["colors"]
    np.testing.assert_array_equal(a4["colors"], want)
    np.testing.assert_array_equal(v4, v)
    iso.write_ply(path, v, t, normals=torch.from_numpy(n.copy()))
    v5, t5, a5 = iso.read_ply(path, attributes=True)
    assert sorted(a5) == ["normals"]
    np.testing.assert_array_equal(a5["normals"], n)
    np.testing.assert_array_equal(t5, t)
    assert iso.read_ply(path, attributes=True)[2].keys() == a5.keys()
    with pytest.raises(ValueError, match="normals"):
        iso.write_ply(path, v, t, normals=n[:-1])
    # a plain file has no attributes
    iso.write_ply(path, v, t)
    assert iso.read_ply(path, attributes=True)[2] == {}


# ------------------------------------------------------------------ the normals entry's argument checks (no HIP call)
def test_normals_entry_rejects_bad_arguments():
    lib = _lib.load()
    err = lambda: lib.anerf_last_error()  # noqa: E731
    need = lib.anerf_isosurface_workspace(9, 9, 9)
    grid = (ctypes.c_float * 729)()
    ws = (ctypes.c_uint64 * (need // 8 + 1))()
    out = (ctypes.c_float * 3)()
    g, w = ctypes.addressof(grid), ctypes.addressof(ws)
    nrm = lambda *a: lib.anerf_isosurface_normals(*a, None)  # noqa: E731
    EINVAL, EWORKSPACE = -1, -3
    assert nrm(None, 9, 9, 9, 0.5, 0, w, need, out, 1) == EINVAL and b"NULL" in err()
    assert nrm(g, 9, 9, 9, 0.5, 0, None, need, out, 1) == EINVAL and b"NULL" in err()
    assert nrm(g, 9, 9, 9, 0.5, 0, w, need, None, 1) == EINVAL and b"NULL" in err()
    assert nrm(g, 9, 9, 9, 0.5, 0, w, need, out, -1) == EINVAL and b"capacity" in err()
    assert nrm(g, 9, 9, 9, 0.5, 0, w, need, out, 1 << 31) == EINVAL and b"capacity" in err()
    assert nrm(g, 9, 0, 9, 0.5, 0, w, need, out, 1) == EINVAL and b">= 1" in err()
    assert nrm(g, 2048, 1024, 1024, 0.5, 0, w, need, out, 1) == EINVAL and b"31 bits" in err()
    assert nrm(g, 9, 9, 9, 0.5, 4, w, need, out, 1) == EINVAL and b"unknown flag" in err()
    assert nrm(g, 9, 9, 9, 0.5, 0, w + 4, need, out, 1) == EINVAL and b"aligned" in err()
    assert nrm(g, 9, 9, 9, 0.5, 0, w, 16, out, 1) == EWORKSPACE and b"anerf_isosurface_normals" in err()
    assert nrm(g, 9, 9, 9, 0.5, 0, w, need, None, 0) == 0  # (capacity 0: nothing to write, no launch)


def test_colors_need_a_network():
    with pytest.raises(ValueError, match="RayCaster.extract_mesh"):
        iso.mesh_from_grid(np.zeros((2, 2, 2), np.float32), None, 1.0, 1, 0.5, colors=True)
    with pytest.raises(ValueError, match="view"):
        iso.mesh_from_grid(np.zeros((2, 2, 2), np.float32), None, 1.0, 1, 0.5, colors=True, view=(1.0, 0.0),
                           radiance=lambda p, d, c: None)

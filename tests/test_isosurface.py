"""CPU: the marching-cubes case table, the NumPy reference of the iso-surface contract (isosurface.py), the PLY
writer and the argument checks of the C entries (which return before any HIP call).

The device kernels are compared with this reference in test_gpu_isosurface.py; here the reference itself is held to
properties that do not depend on it: closedness and orientation (every directed edge has its reverse), vertex
counts from NumPy slicing, interpolation residuals, analytic volumes and Euler characteristics."""
import ctypes
import importlib
import importlib.util
import os

import numpy as np
import pytest

import _iso_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
anerf = importlib.import_module("a-nerf_amd")
iso = importlib.import_module("a-nerf_amd.isosurface")
_lib = importlib.import_module("a-nerf_amd._lib")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_iso_table", os.path.join(REPO, "tools", "gen_iso_table.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------ the table
def test_table_regenerates_to_the_committed_file():
    with open(iso.TABLE_PATH) as f:
        assert f.read() == _generator().render()


def test_table_shape_and_counts():
    tab = iso.load_table()
    assert tab["ntri"].shape == (256,) and tab["tri"].shape == (256, 15)
    assert int(tab["ntri"].max()) == 5 and int(tab["ntri"].sum()) == 820
    assert tab["ntri"][0] == 0 and tab["ntri"][255] == 0
    assert (tab["tri"][0] == -1).all() and (tab["tri"][255] == -1).all()
    for c in range(256):
        n = int(tab["ntri"][c])
        row = tab["tri"][c]
        assert ((row[:3 * n] >= 0) & (row[:3 * n] < 12)).all() and (row[3 * n:] == -1).all()
        # an edge is used exactly when its two corners differ
        used = set(row[:3 * n].tolist())
        for e, (corner, axis) in enumerate(zip(tab["edge_corner"], tab["edge_axis"])):
            crossing = ((c >> corner) & 1) != ((c >> (corner + (1 << axis))) & 1)
            assert (e in used) == crossing, (c, e)
    # edge ids go by (lower corner, axis)
    pairs = list(zip(tab["edge_corner"].tolist(), tab["edge_axis"].tolist()))
    assert pairs == sorted(pairs) and len(set(pairs)) == 12
    assert all(not (corner >> axis) & 1 for corner, axis in pairs)


def test_package_exports():
    assert anerf.isosurface is iso.isosurface and anerf.isosurface_reference is iso.isosurface_reference
    assert anerf.write_ply is iso.write_ply and anerf.render_mesh is iso.render_mesh
    assert hasattr(anerf.RayCaster, "extract_mesh")
    assert hasattr(importlib.import_module("a-nerf_amd.train").StagedCaster, "extract_mesh")


# ------------------------------------------------------------------ 40 random 9^3 fields
@pytest.mark.parametrize("seed", range(40))
def test_random_field_mesh_is_closed_oriented_and_on_the_level_set(seed):
    f = C.random_field(seed)
    v, t = iso.isosurface_reference(f, 0.5)
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    assert len(t) > 0 and t.min() >= 0 and t.max() < len(v)
    assert not C.directed_edge_imbalance(t)  # closed, consistently oriented
    assert len(v) == C.crossing_edges(f, 0.5)
    assert len(np.unique(t)) == len(v)  # every vertex is used
    assert (v >= 0).all() and (v <= np.array(f.shape) - 1).all()
    val, n_int = C.interpolated_values(f, v)
    assert (n_int >= 2).all()
    assert float(np.abs(val - 0.5).max()) <= 1e-6
    assert float(C.areas(v, t).min()) > 0
    # the order is part of the contract: vertices by (owner's linear index, axis)
    owner = np.floor(v).astype(np.int64)
    axis = np.argmax(v - owner, axis=1)
    key = ((owner[:, 0] * f.shape[1] + owner[:, 1]) * f.shape[2] + owner[:, 2]) * 3 + axis
    assert (np.diff(key) > 0).all()


# ------------------------------------------------------------------ analytic shapes, inside = high, threshold 0
def test_sphere():
    v, t = C.reference("sphere_field")
    assert (len(v), len(t)) == (576, 1148)
    assert C.euler(v, t) == 2 and not C.directed_edge_imbalance(t)
    vol = C.signed_volume(v, t)
    exact = 4.0 / 3.0 * np.pi * C.SPHERE_R ** 3
    assert 0.96 * exact <= vol <= 1.00 * exact, vol / exact  # (linear interpolation cuts the convex side)
    r = np.linalg.norm(v.astype(np.float64) - C.SPHERE_C, axis=1)
    assert float(np.abs(r - C.SPHERE_R).max()) <= 0.05
    vf, tf = C.reference("sphere_field", flip=True)
    np.testing.assert_array_equal(vf, v)
    np.testing.assert_array_equal(tf, t[:, [0, 2, 1]])
    assert C.signed_volume(vf, tf) == -vol


def test_torus_and_two_spheres_topology():
    v, t = C.reference("torus_field")
    assert C.euler(v, t) == 0 and not C.directed_edge_imbalance(t) and C.signed_volume(v, t) > 0
    v, t = C.reference("two_spheres_field")
    assert C.euler(v, t) == 4 and not C.directed_edge_imbalance(t) and C.signed_volume(v, t) > 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_surface_cut_by_the_grid_boundary_is_open_only_there(seed):
    f = C.random_field(seed, (9, 9, 9), False)
    v, t = iso.isosurface_reference(f, 0.5)
    assert len(v) == C.crossing_edges(f, 0.5)
    bad = C.directed_edge_imbalance(t)
    assert bad  # (the field crosses the threshold on the outer faces)
    top = np.array(f.shape) - 1
    for a, b in bad:
        on_face = ((v[a] == 0) & (v[b] == 0)) | ((v[a] == top) & (v[b] == top))
        assert on_face.any(), (v[a], v[b])


# ------------------------------------------------------------------ edge cases
def test_empty_results():
    f = C.random_field(0)
    for thr in (-1.0, 2.0):  # all inside, all outside
        v, t = iso.isosurface_reference(f, thr)
        assert v.shape == (0, 3) and v.dtype == np.float32 and t.shape == (0, 3) and t.dtype == np.int32


@pytest.mark.parametrize("shape", [(1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1)])
def test_dimension_of_one_gives_an_empty_mesh(shape):
    """No cells, so no triangles, and no vertices either (a vertex belongs to the cells around its edge)."""
    v, t = iso.isosurface_reference(np.random.default_rng(1).random(shape), 0.5)
    assert v.shape == (0, 3) and v.dtype == np.float32 and t.shape == (0, 3) and t.dtype == np.int32


def test_single_inside_sample_is_an_octahedron():
    f = np.zeros((3, 3, 3), np.float32)
    f[1, 1, 1] = 1.0
    v, t = iso.isosurface_reference(f, 0.25)
    assert (len(v), len(t)) == (6, 8) and C.euler(v, t) == 2 and not C.directed_edge_imbalance(t)
    assert C.signed_volume(v, t) == pytest.approx(4.0 / 3.0 * 0.75 ** 3)
    np.testing.assert_array_equal(v, np.array([[0.25, 1, 1], [1, 0.25, 1], [1, 1, 0.25], [1.75, 1, 1], [1, 1.75, 1],
                                               [1, 1, 1.75]], np.float32))  # (owner's linear index, axis)


def test_nan_samples_are_outside():
    v, t = C.reference("nan_field")
    v0, t0 = C.reference("sphere_field")
    assert np.isfinite(v).all()
    np.testing.assert_array_equal(v, v0)
    np.testing.assert_array_equal(t, t0)
    # with relu too: np.maximum keeps the NaN
    v1, t1 = C.reference("nan_field", threshold=1.0, relu=True)
    v2, t2 = C.reference("sphere_field", threshold=1.0, relu=True)
    assert np.isfinite(v1).all() and len(t1) > 0
    np.testing.assert_array_equal(v1, v2)
    np.testing.assert_array_equal(t1, t2)


def test_relu_moves_vertices():
    f = C.relu_field()
    v, t = C.reference("relu_field", threshold=0.25, relu=True)
    vc, tc = iso.isosurface_reference(np.maximum(f, 0), 0.25)
    np.testing.assert_array_equal(v, vc)
    np.testing.assert_array_equal(t, tc)
    vn, tn = C.reference("relu_field", threshold=0.25)
    np.testing.assert_array_equal(t, tn)  # (the classification at a positive threshold is the same)
    assert float(np.abs(v - vn).max()) > 0.05


def test_write_ply_round_trips(tmp_path):
    v, t = C.reference("sphere_field")
    path = str(tmp_path / "s.ply")
    iso.write_ply(path, v, t)
    with open(path, "rb") as f:
        blob = f.read()
    head = blob[:blob.index(b"end_header\n")].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    assert head[2:] == [f"element vertex {len(v)}", "property float x", "property float y", "property float z",
                        f"element face {len(t)}", "property list uchar int vertex_indices", ""]
    assert len(blob) == blob.index(b"end_header\n") + 11 + 12 * len(v) + 13 * len(t)
    v2, t2 = iso.read_ply(path)
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(t2, t)
    import torch
    iso.write_ply(path, torch.from_numpy(v.copy()), torch.from_numpy(t.copy()))  # (tensors too)
    assert open(path, "rb").read() == blob
    iso.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v3, t3 = iso.read_ply(path)
    assert v3.shape == (0, 3) and t3.shape == (0, 3)


# ------------------------------------------------------------------ the C entries' argument checks (no HIP call)
def test_c_entries_reject_bad_arguments():
    lib = _lib.load()
    err = lambda: lib.anerf_last_error()  # noqa: E731
    need = lib.anerf_isosurface_workspace(9, 9, 9)
    assert need >= 4 * 729
    assert lib.anerf_isosurface_workspace(5, 1, 7) > 0  # (a dimension of 1 is valid)
    assert lib.anerf_isosurface_workspace(0, 9, 9) == 0 and b"anerf_isosurface_workspace" in err()
    assert lib.anerf_isosurface_workspace(2048, 1024, 1024) == 0
    grid = (ctypes.c_float * 729)()
    ws = (ctypes.c_uint64 * (need // 8 + 1))()
    tot = (ctypes.c_int64 * 2)()
    out_v, out_t = (ctypes.c_float * 3)(), (ctypes.c_int32 * 3)()
    g, w = ctypes.addressof(grid), ctypes.addressof(ws)
    count = lambda *a: lib.anerf_isosurface_count(*a, None)  # noqa: E731
    emit = lambda *a: lib.anerf_isosurface_emit(*a, None)  # noqa: E731
    EINVAL, EWORKSPACE = -1, -3
    assert count(None, 9, 9, 9, 0.5, 0, w, need, tot) == EINVAL and b"NULL" in err()
    assert count(g, 9, 9, 9, 0.5, 0, None, need, tot) == EINVAL and b"NULL" in err()
    assert count(g, 9, 9, 9, 0.5, 0, w, need, None) == EINVAL and b"NULL" in err()
    assert count(g, 9, 0, 9, 0.5, 0, w, need, tot) == EINVAL and b">= 1" in err()
    assert count(g, 9, 9, -3, 0.5, 0, w, need, tot) == EINVAL and b">= 1" in err()
    assert count(g, 2048, 1024, 1024, 0.5, 0, w, need, tot) == EINVAL and b"31 bits" in err()
    assert count(g, 65536, 65536, 2, 0.5, 0, w, need, tot) == EINVAL and b"31 bits" in err()
    assert count(g, 9, 9, 9, 0.5, 4, w, need, tot) == EINVAL and b"unknown flag" in err()
    assert count(g, 9, 9, 9, 0.5, 0, w + 4, need, tot) == EINVAL and b"aligned" in err()
    assert count(g, 9, 9, 9, 0.5, 0, w, need - 1, tot) == EWORKSPACE and b"anerf_isosurface_count" in err()
    assert emit(None, 9, 9, 9, 0.5, 0, w, need, out_v, 1, out_t, 1) == EINVAL and b"NULL" in err()
    assert emit(g, 9, 9, 9, 0.5, 0, w, need, None, 1, out_t, 1) == EINVAL and b"NULL" in err()
    assert emit(g, 9, 9, 9, 0.5, 0, w, need, out_v, 1, None, 1) == EINVAL and b"NULL" in err()
    assert emit(g, 9, 9, 9, 0.5, 0, w, need, out_v, -1, out_t, 1) == EINVAL and b"capacities" in err()
    assert emit(g, 9, 9, 9, 0.5, 0, w, need, out_v, 1, out_t, 1 << 31) == EINVAL and b"capacities" in err()
    assert emit(g, 0, 9, 9, 0.5, 0, w, need, out_v, 1, out_t, 1) == EINVAL and b">= 1" in err()
    assert emit(g, 9, 9, 9, 0.5, 8, w, need, out_v, 1, out_t, 1) == EINVAL and b"unknown flag" in err()
    assert emit(g, 9, 9, 9, 0.5, 0, w, 16, out_v, 1, out_t, 1) == EWORKSPACE and b"anerf_isosurface_emit" in err()


def test_isosurface_rejects_bad_shapes_without_a_fallback():
    with pytest.raises(ValueError, match="3-D"):
        iso.isosurface(np.zeros((4, 4), np.float32), 0.5)
    with pytest.raises(ValueError, match="3-D"):
        iso.isosurface_reference(np.zeros((4, 4), np.float32), 0.5)
    with pytest.raises(ValueError, match="coords"):
        iso.mesh_from_grid(np.zeros((2, 2, 2), np.float32), None, 1.0, 1, 0.5, coords="metres")

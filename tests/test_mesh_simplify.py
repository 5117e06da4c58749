"""CPU: the contract of vertex clustering (meshops.simplify_mesh_reference, the checker of the device kernels) against
an independent brute force, the facts that follow from it on the named meshes, its properties, and the argument errors
of simplify_mesh and of the C entries, which come before anything is launched."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _mesh_cases as M
import _simplify_cases as C

anerf = importlib.import_module("a-nerf_amd")
meshops = importlib.import_module("a-nerf_amd.meshops")
_lib = importlib.import_module("a-nerf_amd._lib")


def _assert_same(got, want, what):
    """All four outputs equal, the positions through their int32 views."""
    for name, g, w in zip(C.FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if name == "vertices":
            g, w = g.view(np.int32), w.view(np.int32)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def test_exported():
    assert anerf.simplify_mesh is meshops.simplify_mesh
    assert anerf.simplify_mesh_reference is meshops.simplify_mesh_reference
    assert anerf.SimplifiedMesh is meshops.SimplifiedMesh
    assert anerf.SIMPLIFY_MAX_CELLS == meshops.SIMPLIFY_MAX_CELLS == 2 ** 26 == _lib.ANERF_SIMPLIFY_MAX_CELLS


@pytest.mark.parametrize("cell", C.CELLS)
@pytest.mark.parametrize("case", ("sphere", "blobs", "random33"))
def test_checker_matches_the_brute_force(case, cell):
    v, t = C.mesh(case)
    ref = C.reference(case, cell)
    assert isinstance(ref, meshops.SimplifiedMesh) and ref.attrs is None
    assert ref.vertices.dtype == np.float32 and all(x.dtype == np.int32 for x in ref[1:4])
    _assert_same(ref[:4], C.brute_force(v, t, cell), f"{case} at {cell}")


def test_checker_matches_the_brute_force_with_a_given_origin():
    v, t = C.mesh("blobs")
    for origin in ((0, 0, 0), (-1.25, -0.5, -3)):
        _assert_same(C.reference("blobs", 2.0, origin)[:4], C.brute_force(v, t, 2.0, origin), f"blobs from {origin}")


@pytest.mark.parametrize("case", sorted(C.S.WHEEL_SETS))
def test_checker_on_disjoint_wheels(case):
    """Nothing merges: the checker returns the list as it is, and agrees with the brute force on the smaller case."""
    v, t = C.wheels(case)
    assert (len(v), len(t)) == {"many_wheels": (37400, 36300), "mixed_wheels": (5076, 5073)}[case]
    ref = meshops.simplify_mesh_reference(v, t, 1.0, origin=(0, 0, 0))
    np.testing.assert_array_equal(ref.triangles, t)
    np.testing.assert_array_equal(ref.vertex_map, np.arange(len(v)))
    np.testing.assert_array_equal(ref.representatives, np.arange(len(v)))
    if case == "mixed_wheels":
        _assert_same(ref[:4], C.brute_force(v, t, 1.0, (0, 0, 0)), case)


def test_outputs_are_consistent():
    """What the contract says of the outputs, read off the checker's: the representative is its cell's smallest
    member, the new vertices keep the order of their representatives, the survivors that of the input."""
    v, t = C.mesh("random33")
    ref = C.reference("random33", 2.0)
    reps, vmap = ref.representatives.astype(np.int64), ref.vertex_map.astype(np.int64)
    assert (np.diff(reps) > 0).all() and (vmap >= 0).all()
    np.testing.assert_array_equal(vmap[reps], np.arange(len(reps)))
    assert (reps[vmap] <= np.arange(len(v))).all()
    mapped = vmap[t]
    where = {tuple(r): i for i, r in reversed(list(enumerate(mapped.tolist())))}  # (the first index of every row)
    index = np.array([where[tuple(r)] for r in ref.triangles.tolist()])
    assert (np.diff(index) > 0).all()


@pytest.mark.parametrize("cell", C.CELLS)
def test_closed_meshes_stay_closed(cell):
    for case, chi in (("sphere", 2), ("torus", 0), ("two_spheres", 4)):
        ref = C.reference(case, cell)
        assert (C.edge_counts(ref.triangles) == 2).all(), case
        assert C.euler(ref.triangles) == chi, case


def test_the_recorded_counts():
    ref = C.reference("sphere", 0.5)
    assert (len(ref.vertices), len(ref.triangles)) == (510, 1016)
    assert [C.dropped("blobs", c)[1] for c in C.CELLS] == [0, 0, 1, 4]
    assert [C.dropped("random33", c)[1] for c in C.CELLS] == [356, 2017, 2106, 1936]
    for case in C.NAMED:
        for cell in C.CELLS:
            assert C.dropped(case, cell)[0] > 0, (case, cell)
    # clustering can pinch thin parts: edges with more than two triangles on the random field's surface
    assert (C.edge_counts(C.reference("random33", 2.0).triangles) > 2).any()


@pytest.mark.parametrize("case", C.NAMED)
def test_displacement_is_at_most_a_cell(case):
    """Along every axis |p'[vertex_map[v]] - p[v]| <= cell + slack.  In exact arithmetic both points lie in the closed
    cell [o + cell c, o + cell (c + 1)].  The roundings between them: p - o, the division, c + m, the product with cell
    and the sum with o, each within 2^-24 of a quantity that |o| + |p| + cell bounds (with q = (p - o) / cell the
    first two move cell q by at most 2 2^-24 |p - o|, the others p' by at most 3 2^-24 (|o| + |p| + cell)), and the
    fixed point: every member's offset is rounded to 2^-20 of a cell (2^-21 cell at most), m once more to fp32.
    slack = 8 2^-24 (|o| + |p| + cell) + 2^-20 cell covers them."""
    v, _ = C.mesh(case)
    for cell in C.CELLS:
        ref = C.reference(case, cell)
        moved = np.abs(ref.vertices.astype(np.float64)[ref.vertex_map] - v.astype(np.float64))
        o = v.min(0).astype(np.float64)
        slack = 8 * 2.0 ** -24 * (np.abs(o).max() + np.abs(v).max() + cell) + 2.0 ** -20 * cell
        print(f"{case} at {cell}: moved at most {moved.max() / cell:.4f} cell, slack {slack:.3g}")
        assert moved.max() <= cell + slack


@pytest.mark.parametrize("kind", ("permuted", "reversed"))
@pytest.mark.parametrize("case", ("blobs", "random33"))
def test_relabelling_keeps_the_geometry(case, kind):
    """Renaming the vertices changes ids and order, not the set of new positions nor the set of the triangles'
    vertex-position triples (the triangles keep their order, so the same one of every set of copies survives)."""
    a, b = C.reference(case, 2.0), C.reference(f"{case}/{kind}", 2.0)
    assert not np.array_equal(a.representatives, b.representatives)

    def rows(x):
        x = x.reshape(len(x), -1).view(np.int32)
        return x[np.lexsort(x.T[::-1])]
    np.testing.assert_array_equal(rows(a.vertices), rows(b.vertices))
    np.testing.assert_array_equal(rows(a.vertices[a.triangles]), rows(b.vertices[b.triangles]))


def test_extreme_cells():
    v, t = C.mesh("sphere")
    big = meshops.simplify_mesh_reference(v, t, 1000.0)
    assert big.vertices.shape == (1, 3) and big.triangles.shape == (0, 3)
    assert (big.vertex_map == 0).all() and big.representatives.tolist() == [0]
    cell = 2.0 ** -5
    alone = meshops.simplify_mesh_reference(v, t, cell)
    np.testing.assert_array_equal(alone.vertex_map, np.arange(len(v)))
    np.testing.assert_array_equal(alone.representatives, np.arange(len(v)))
    np.testing.assert_array_equal(alone.triangles, t)
    assert np.abs(alone.vertices - v).max() <= 2.0 ** -20 * cell + 8 * 2.0 ** -24 * (2 * np.abs(v).max() + cell)


def test_empty_lists_and_attrs():
    v, t = C.mesh("blobs")
    none = meshops.simplify_mesh_reference(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert [x.shape for x in none[:4]] == [(0, 3), (0, 3), (0,), (0,)]
    only_v = meshops.simplify_mesh_reference(v, np.zeros((0, 3), np.int32), 2.0)
    assert only_v.triangles.shape == (0, 3)
    ref = C.reference("blobs", 2.0)
    _assert_same(only_v[:4], (ref.vertices, only_v.triangles, ref.vertex_map, ref.representatives), "no triangles")
    f, u = M.attributes(len(v))
    got = meshops.simplify_mesh_reference(v, t, 2.0, attrs={"f": f, "u": u})
    np.testing.assert_array_equal(got.attrs["f"], f[got.representatives])
    np.testing.assert_array_equal(got.attrs["u"], u[got.representatives])
    as_list = meshops.simplify_mesh_reference(v, t, 2.0, attrs=[u])
    assert isinstance(as_list.attrs, list) and np.array_equal(as_list.attrs[0], u[got.representatives])


def test_argument_errors_come_before_any_launch(monkeypatch):
    def no_library():
        raise AssertionError("the argument checks must come before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    v = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]])
    tri = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    for fn in (meshops.simplify_mesh, meshops.simplify_mesh_reference):
        bad = v.clone()
        for x in (float("nan"), float("inf"), float("-inf")):
            bad[2, 1] = x
            with pytest.raises(ValueError, match="finite"):
                fn(bad, tri, 1.0)
        for cell in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60):
            with pytest.raises(ValueError, match="cell"):
                fn(v, tri, cell)
        with pytest.raises(ValueError, match="below the origin"):
            fn(v, tri, 1.0, origin=(0, 0.5, 0))
        with pytest.raises(ValueError, match="origin"):
            fn(v, tri, 1.0, origin=(0, float("nan"), 0))
        with pytest.raises(ValueError, match="origin"):
            fn(v, tri, 1.0, origin=(0, 0))
        with pytest.raises(ValueError, match=str(2 ** 26)):
            fn(v, tri, 0.01)  # 501^3 cells
        with pytest.raises(ValueError, match="SIMPLIFY_MAX_CELLS"):
            fn(v, tri, 1e-30)
        for ids in ([[0, 1, 4]], [[0, -1, 2]]):
            with pytest.raises(ValueError, match="outside"):
                fn(v, torch.tensor(ids, dtype=torch.int32), 1.0)
            with pytest.raises(ValueError, match="outside"):
                fn(v, np.array(ids, np.int64), 1.0)
        with pytest.raises(ValueError, match="outside"):
            fn(torch.zeros(0, 3), tri, 1.0)
        with pytest.raises(ValueError, match="rows"):
            fn(v, tri, 1.0, attrs={"c": torch.zeros(3, 3)})
        with pytest.raises(ValueError, match="rows"):
            fn(v, tri, 1.0, attrs=[torch.zeros(4, 3), torch.zeros(5)])
        with pytest.raises(ValueError, match=r"\[V, 3\]"):
            fn(torch.zeros(4, 2), tri, 1.0)
        with pytest.raises(ValueError, match=r"\[T, 3\]"):
            fn(v, torch.zeros(4, 2, dtype=torch.int32), 1.0)
        with pytest.raises(ValueError, match="int32 or int64"):
            fn(v, torch.zeros(1, 3), 1.0)


def _buffers():
    """Host memory standing in for every pointer: the entries refuse their arguments before they touch any of it."""
    return {k: ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p) for k in "vtwxyzmr"}


def _count(lib, b, nv=4, nt=2, origin=(0, 0, 0), cell=1.0, dims=(2, 2, 2), ws_bytes=1 << 30, null=()):
    o, d = (ctypes.c_float * 3)(*origin), (ctypes.c_int32 * 3)(*dims)
    a = dict(b, o=ctypes.cast(o, ctypes.c_void_p), d=ctypes.cast(d, ctypes.c_void_p))
    a.update({k: None for k in null})
    return lib.anerf_mesh_simplify_count(a["v"], nv, a["t"], nt, a["o"], cell, a["d"], a["w"], ws_bytes, a["x"], None)


def _emit(lib, b, nv=4, nt=2, n_out_v=1, n_out_t=1, ws_bytes=1 << 30, cell=1.0, null=()):
    o, d = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int32 * 3)(2, 2, 2)
    a = dict(v=b["v"], t=b["t"], w=b["w"], y=b["y"], z=b["z"], m=b["m"], r=b["r"])
    a.update({k: None for k in null})
    return lib.anerf_mesh_simplify_emit(a["v"], nv, a["t"], nt, ctypes.cast(o, ctypes.c_void_p), cell,
                                        ctypes.cast(d, ctypes.c_void_p), a["w"], ws_bytes, a["y"], n_out_v, a["z"],
                                        n_out_t, a["m"], a["r"], None)


def test_c_entries_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    b = _buffers()
    err = lib.anerf_last_error
    need = lib.anerf_mesh_simplify_workspace(4, 2, 8)
    assert need > 0 and need % 8 == 0
    assert lib.anerf_mesh_simplify_workspace(126194, 253036, 128 ** 3) > 4 * 128 ** 3
    for bad in ((-1, 2, 8), (4, 2 ** 31, 8), (4, 2, 0), (4, 2, 2 ** 26 + 1)):
        assert lib.anerf_mesh_simplify_workspace(*bad) == 0 and b"2^26" in err()
    assert lib.anerf_mesh_simplify_workspace(0, 0, 2 ** 26) > 2 ** 28
    for call in (_count, _emit):
        for null in ("v", "t", "w"):
            assert call(lib, b, null=(null,)) == -1 and b"NULL" in err(), null
        assert call(lib, b, nv=-1) == -1 and b"2^31" in err()
        assert call(lib, b, nt=2 ** 31) == -1 and b"2^31" in err()
        for cell in (0.0, -2.0, float("nan"), float("inf")):
            assert call(lib, b, cell=cell) == -1 and b"cell" in err()
        assert call(lib, b, ws_bytes=need - 8) == -1 and b"anerf_mesh_simplify_workspace" in err()
    for null in ("o", "d", "x"):
        assert _count(lib, b, null=(null,)) == -1 and b"NULL" in err(), null
    assert _count(lib, b, origin=(0, float("inf"), 0)) == -1 and b"origin" in err()
    for dims in ((0, 2, 2), (2, -1, -1), (1024, 1024, 65), (2 ** 26, 2, 1), (2 ** 30, 2 ** 30, 2 ** 30)):
        assert _count(lib, b, dims=dims) == -1 and b"2^26" in err(), dims
    misaligned = dict(b, w=ctypes.c_void_p(b["w"].value + 4))
    assert _count(lib, misaligned) == -1 and b"aligned" in err()
    # emit: sizes that no count can give, outputs missing for a non-zero extent
    for sizes in (dict(n_out_v=5), dict(n_out_v=-1), dict(n_out_t=3), dict(n_out_t=-1)):
        assert _emit(lib, b, **sizes) == -1 and b"counted totals" in err(), sizes
    for null in ("y", "z", "m", "r"):
        assert _emit(lib, b, null=(null,)) == -1 and b"NULL output" in err(), null

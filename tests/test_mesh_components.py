"""CPU: the checkers of the mesh-component path (meshops.mesh_components_reference, filter_mesh_reference) against
scipy and against mesh properties, the argument checks of the C entries that return before any HIP call, and the
torch-side range check of mesh_components (no kernel of csrc/anerf_mesh.hip is launched here)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _iso_cases as C
import _mesh_cases as M

anerf = importlib.import_module("a-nerf_amd")
meshops = importlib.import_module("a-nerf_amd.meshops")
_lib = importlib.import_module("a-nerf_amd._lib")


def test_exports():
    for name in ("mesh_components", "mesh_components_reference", "filter_mesh"):
        assert getattr(anerf, name) is getattr(meshops, name) and name in anerf.__all__
    import inspect
    iso = importlib.import_module("a-nerf_amd.isosurface")
    train = importlib.import_module("a-nerf_amd.train")
    for fn in (iso.mesh_from_grid, iso.render_mesh, anerf.RayCaster.extract_mesh, train.StagedCaster.extract_mesh):
        p = inspect.signature(fn).parameters
        assert p["keep_largest"].default is None and p["min_triangles"].default == 0


@pytest.mark.parametrize("name", list(M.MESHES))
def test_reference_against_scipy(name):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    v, t = M.mesh(name)
    nv = len(v)
    comp = M.components(name)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]]).astype(np.int64)
    g = sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(nv, nv))
    n, lab = csgraph.connected_components(g, directed=False)
    assert n == len(comp.roots) == M.MESHES[name][2]
    # the same partition: scipy's label <-> our rank is a bijection
    pairs = np.unique(np.stack([lab, comp.labels], -1), axis=0)
    assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n
    # roots: each part's minimum id; counts
    mins = np.full(n, nv, np.int64)
    np.minimum.at(mins, lab, np.arange(nv))
    np.testing.assert_array_equal(comp.roots[comp.labels], mins[lab])
    np.testing.assert_array_equal(comp.vertex_counts[comp.labels], np.bincount(lab)[lab])
    np.testing.assert_array_equal(comp.triangle_counts[comp.labels], np.bincount(lab[t[:, 0]], minlength=n)[lab])
    # ranked: counts descend, ties by the smaller root
    tc, r = comp.triangle_counts, comp.roots
    assert ((tc[:-1] > tc[1:]) | ((tc[:-1] == tc[1:]) & (r[:-1] < r[1:]))).all()
    assert comp.labels.dtype == np.int32 and r.dtype == np.int32 and tc.dtype == np.int64
    assert int(tc.sum()) == len(t) and int(comp.vertex_counts.sum()) == nv


def test_expected_component_counts():
    assert [len(M.components(n).roots) for n in M.MESHES] == [1, 1, 2, 5, 358]
    two = M.components("two_spheres")
    assert two.triangle_counts.tolist() == [524, 524] and two.roots[0] == 0 and two.roots[0] < two.roots[1]
    big = M.components("random33")
    assert int(big.triangle_counts[0]) == 92772 and int(big.triangle_counts[1]) <= 48
    assert (len(M.mesh("random33")[0]), len(M.mesh("random33")[1])) == (46008, 96348)


@pytest.mark.parametrize("name", ["no_triangles", "no_vertices", "one_triangle", "degenerate", "duplicated", "disjoint"])
def test_reference_on_small_lists(name):
    tri, nv, comp = M.synthetic(name)
    ref = meshops.mesh_components_reference(tri, nv)
    for a, b in zip(ref, comp):
        np.testing.assert_array_equal(a, b)
    expected = {"no_triangles": ([0, 1, 2, 3, 4, 5, 6], [0] * 7, [1] * 7), "no_vertices": ([], [], []),
                "one_triangle": ([2, 0, 1, 5], [1, 0, 0, 0], [3, 1, 1, 1]),
                "degenerate": ([1, 0, 2], [1, 0, 0], [2, 1, 1]), "duplicated": ([0], [2], [3])}
    if name in expected:
        assert [x.tolist() for x in ref[1:]] == [list(x) for x in expected[name]]
    else:
        assert len(ref.roots) == 10000 and ref.labels[4 * 17 + 3] == 5017


def test_filter_contract_on_the_reference():
    v, t = M.mesh("two_spheres")
    a_f, a_u = M.attributes(len(v))
    fv, ft, fa = meshops.filter_mesh_reference(v, t, {"f": a_f, "u": a_u}, keep_largest=1)
    assert len(ft) == 524 and not C.directed_edge_imbalance(ft) and C.euler(fv, ft) == 2
    keep, kept, out = M.filter_expected(M.components("two_spheres"), t, 1, 0)
    np.testing.assert_array_equal(ft, out)
    np.testing.assert_array_equal(fv, v[kept])
    np.testing.assert_array_equal(fa["f"], a_f[kept])
    np.testing.assert_array_equal(fa["u"], a_u[kept])
    assert ft.dtype == np.int32 and fa["u"].dtype == np.uint8
    # order preserved, ids remapped: the kept rows ascend, and each surviving triangle is the original's image
    assert (np.diff(kept) > 0).all()
    alive = keep[t].all(axis=1)
    np.testing.assert_array_equal(kept[ft], t[alive])
    np.testing.assert_array_equal(fv[ft], v[t[alive]])
    # the rule: rank < keep_largest and triangle_count >= min_triangles
    v3, t3 = M.mesh("random33")
    comp = M.components("random33")
    for kl, mt in ((1, 0), (2, 40), (None, 40), (3, 0), (0, 0), (None, 10 ** 6)):
        fv, ft = meshops.filter_mesh_reference(v3, t3, keep_largest=kl, min_triangles=mt)
        _, kept, out = M.filter_expected(comp, t3, kl, mt)
        np.testing.assert_array_equal(ft, out)
        np.testing.assert_array_equal(fv, v3[kept])
        n_kept = int(((comp.triangle_counts >= mt) & (np.arange(358) < (358 if kl is None else kl))).sum())
        assert len(np.unique(comp.labels[kept])) == n_kept
        assert fv.shape[1:] == (3,) and ft.shape[1:] == (3,)
    assert len(fv) == 0 and len(ft) == 0
    # the defaults return the inputs themselves
    assert meshops.filter_mesh_reference(v, t)[0] is v and meshops.filter_mesh(v, t)[1] is t
    out = meshops.filter_mesh(v, t, [a_f])
    assert out[0] is v and out[2][0] is a_f


def test_c_abi_validation():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def err():
        return lib.anerf_last_error()
    # components
    assert lib.anerf_mesh_components(None, 1, 3, p, p, p, p, p, 12, None) == -1 and b"triangles" in err()
    assert lib.anerf_mesh_components(p, -1, 3, p, p, p, p, p, 12, None) == -1 and b"n_tri" in err()
    assert lib.anerf_mesh_components(p, 1, -3, p, p, p, p, p, 12, None) == -1 and b"n_vertices" in err()
    assert lib.anerf_mesh_components(p, 1, 1 << 31, p, p, p, p, p, 1 << 40, None) == -1
    assert lib.anerf_mesh_components(p, 1, 3, None, p, p, p, p, 12, None) == -1 and b"NULL" in err()
    assert lib.anerf_mesh_components(p, 1, 3, p, None, p, p, p, 12, None) == -1
    assert lib.anerf_mesh_components(p, 1, 3, p, p, None, p, p, 12, None) == -1
    assert lib.anerf_mesh_components(p, 1, 3, p, p, p, None, p, 12, None) == -1 and b"n_components" in err()
    assert lib.anerf_mesh_components(p, 1, 3, p, p, p, p, None, 12, None) == -1 and b"workspace" in err()
    assert lib.anerf_mesh_components(p, 1, 3, p, p, p, p, p, 11, None) == -1
    assert b"anerf_mesh_components_workspace" in err()
    assert lib.anerf_mesh_components_workspace(3, 1) == 12 and lib.anerf_mesh_components_workspace(0, 0) == 0
    assert lib.anerf_mesh_components_workspace(-1, 0) == 0 and b"anerf_mesh_components_workspace" in err()
    # compaction
    need = lib.anerf_mesh_compact_workspace(3, 1)
    assert need == 24 and lib.anerf_mesh_compact_workspace(0, 0) == 24
    assert lib.anerf_mesh_compact_workspace(1025, 7) == 48 and lib.anerf_mesh_compact_workspace(7, 2049) == 72
    assert lib.anerf_mesh_compact_workspace(0, -1) == 0 and b"anerf_mesh_compact_workspace" in err()
    assert lib.anerf_mesh_compact_count(None, 3, p, 1, p, need, p, None) == -1 and b"NULL" in err()
    assert lib.anerf_mesh_compact_count(p, 3, None, 1, p, need, p, None) == -1
    assert lib.anerf_mesh_compact_count(p, 3, p, 1, None, need, p, None) == -1
    assert lib.anerf_mesh_compact_count(p, 3, p, 1, p, need, None, None) == -1 and b"totals" in err()
    assert lib.anerf_mesh_compact_count(p, -3, p, 1, p, need, p, None) == -1 and b"n_vertices" in err()
    assert lib.anerf_mesh_compact_count(p, 3, p, -1, p, need, p, None) == -1
    assert lib.anerf_mesh_compact_count(p, 3, p, 1, p, need - 1, p, None) == -1
    assert b"anerf_mesh_compact_workspace" in err()
    assert lib.anerf_mesh_compact_count(p, 3, p, 1, ctypes.c_void_p(p.value + 4), need, p, None) == -1
    assert b"aligned" in err()
    assert lib.anerf_mesh_compact_emit(p, 3, p, 1, p, need - 1, p, p, 3, p, 1, None) == -1
    assert lib.anerf_mesh_compact_emit(p, 3, p, 1, p, need, None, p, 3, p, 1, None) == -1 and b"NULL output" in err()
    assert lib.anerf_mesh_compact_emit(p, 3, p, 1, p, need, p, None, 3, p, 1, None) == -1
    assert lib.anerf_mesh_compact_emit(p, 3, p, 1, p, need, p, p, 3, None, 1, None) == -1
    assert lib.anerf_mesh_compact_emit(p, 3, p, 1, p, need, p, p, -1, p, 1, None) == -1 and b"capacities" in err()
    assert lib.anerf_mesh_compact_emit(p, 3, p, 1, p, need, p, p, 3, p, 1 << 31, None) == -1


def test_range_check_raises_before_any_launch(monkeypatch):
    def no_library():
        raise AssertionError("the range check must come before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    ok = [[0, 1, 2], [2, 1, 3]]
    for bad, nv in (([[0, 1, 4]], 4), ([[0, -1, 2]], 4), ([[5, 1, 2]], 5)):
        for dtype in (torch.int32, torch.int64):
            tri = torch.tensor(ok + bad, dtype=dtype)
            with pytest.raises(ValueError, match="outside"):
                meshops.mesh_components(tri, nv)
            with pytest.raises(ValueError, match="outside"):
                meshops.filter_mesh(torch.zeros(nv, 3), tri, keep_largest=1)
        with pytest.raises(ValueError, match="outside"):
            meshops.mesh_components(np.array(ok + bad, np.int32), nv)
        with pytest.raises(ValueError, match="outside"):
            meshops.mesh_components_reference(np.array(ok + bad), nv)
    with pytest.raises(ValueError, match=r"\[T, 3\]"):
        meshops.mesh_components(torch.zeros(4, 2, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="keep_largest"):
        meshops.filter_mesh(torch.zeros(4, 3), torch.tensor(ok, dtype=torch.int32), keep_largest=-1)

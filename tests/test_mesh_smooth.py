"""CPU: the checkers of the adjacency / smoothing path (meshops.vertex_adjacency_reference, smooth_mesh_reference)
against scipy, against a dense float64 operator and against what smoothing is for (a noisy sphere gets smoother, Taubin
keeps its volume and the Laplacian does not, a pinned rim stays), the argument errors that come before any launch, and
the argument checks of the C entries that return before any HIP call (no kernel of csrc/anerf_mesh.hip is launched)."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest
import torch

import _iso_cases as C
import _mesh_cases as M
import _smooth_cases as S

anerf = importlib.import_module("a-nerf_amd")
meshops = importlib.import_module("a-nerf_amd.meshops")
_lib = importlib.import_module("a-nerf_amd._lib")


def test_exports():
    for name in ("vertex_adjacency", "vertex_adjacency_reference", "smooth_mesh", "smooth_mesh_reference"):
        assert getattr(anerf, name) is getattr(meshops, name) and name in anerf.__all__
    iso = importlib.import_module("a-nerf_amd.isosurface")
    train = importlib.import_module("a-nerf_amd.train")
    for fn in (iso.mesh_from_grid, iso.render_mesh, anerf.RayCaster.extract_mesh, train.StagedCaster.extract_mesh):
        p = inspect.signature(fn).parameters
        assert p["smooth"].default == 0 and p["smooth_lambda"].default == 0.5 and p["smooth_mu"].default == -0.53
    p = inspect.signature(meshops.smooth_mesh).parameters
    assert (p["iterations"].default, p["lam"].default, p["mu"].default, p["pin"].default) == (10, 0.5, -0.53, "boundary")
    assert inspect.signature(meshops.smooth_mesh_reference).parameters.keys() == p.keys()


# ------------------------------------------------------------------ adjacency
@pytest.mark.parametrize("case", S.CLOSED + ("hemisphere",))
def test_adjacency_reference_against_scipy(case):
    sparse = pytest.importorskip("scipy.sparse")
    tri, nv = S.triangle_list(case)
    adj = S.adjacency(case)
    t = np.asarray(tri, np.int64)
    a, b = t[:, [0, 0, 1, 1, 2, 2]].reshape(-1), t[:, [1, 2, 0, 2, 0, 1]].reshape(-1)
    m = sparse.coo_matrix((np.ones(len(a)), (a, b)), shape=(nv, nv)).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    assert adj.offsets.dtype == np.int32 and adj.neighbors.dtype == np.int32 and adj.boundary.dtype == bool
    np.testing.assert_array_equal(adj.offsets, m.indptr)
    np.testing.assert_array_equal(adj.neighbors, m.indices)
    once = np.zeros(nv, bool)
    once[np.repeat(np.arange(nv), np.diff(m.indptr))[m.data == 1]] = True  # a stored 1: a pair listed once
    np.testing.assert_array_equal(adj.boundary, once)
    if case in S.CLOSED:
        assert not adj.boundary.any() and 9 <= np.diff(adj.offsets).max() <= 13
        assert not C.directed_edge_imbalance(tri)


def test_hemisphere_is_the_sphere_cut_open():
    v, t = S.hemisphere()
    adj = S.adjacency("hemisphere")
    assert (len(v), len(t), int(adj.boundary.sum())) == (288, 526, 48)
    assert len(M.mesh("sphere")[0]) == 576


@pytest.mark.parametrize("name", S.SMALL)
def test_adjacency_reference_on_small_lists(name):
    adj = S.adjacency(name)
    exp = {"no_triangles": ([0] * 8, [], [0] * 7),
           "no_vertices": ([0], [], []),
           "one_triangle": ([0, 0, 0, 2, 4, 6, 6], [3, 4, 2, 4, 2, 3], [0, 0, 1, 1, 1, 0]),
           "degenerate": ([0, 0, 1, 1, 2], [3, 1], [0, 0, 0, 0]),  # (1,3) and (3,1) are listed twice each
           "duplicated": ([0, 2, 4, 6], [1, 2, 0, 2, 0, 1], [0, 0, 0])}[name]
    np.testing.assert_array_equal(adj.offsets, np.array(exp[0], np.int32))
    np.testing.assert_array_equal(adj.neighbors, np.array(exp[1], np.int32))
    np.testing.assert_array_equal(adj.boundary, np.array(exp[2], bool))


@pytest.mark.parametrize("n", [3, 32, 40, 5000])
def test_adjacency_reference_on_the_wheel(n):
    adj = S.adjacency(f"wheel{n}")
    deg = np.diff(adj.offsets)
    assert deg[0] == n and (deg[1:] == 3).all()  # (the hub and the two rim neighbours)
    np.testing.assert_array_equal(adj.neighbors[:n], np.arange(1, n + 1))
    assert not adj.boundary[0] and adj.boundary[1:].all()


@pytest.mark.parametrize("case", sorted(S.WHEEL_SETS))
def test_adjacency_reference_on_disjoint_wheels(case):
    """Every wheel of the list has its own wheel's adjacency, at its id offset."""
    ns = S.WHEEL_SETS[case]
    tri, nv = S.triangle_list(case)
    adj = S.adjacency(case)
    assert (nv, len(tri)) == {"many_wheels": (37400, 36300), "mixed_wheels": (5076, 5073)}[case]
    assert adj.offsets[-1] == 4 * sum(ns) and np.diff(adj.offsets).max() == max(ns)
    assert int(adj.boundary.sum()) == sum(ns)  # every rim vertex, no hub
    for n in sorted(set(ns)):  # (the first wheel of every size)
        first = sum(m + 1 for m in ns[:ns.index(n)])
        one = S.adjacency(f"wheel{n}")
        b, e = adj.offsets[first], adj.offsets[first + n + 1]
        np.testing.assert_array_equal(adj.offsets[first:first + n + 2] - b, one.offsets)
        np.testing.assert_array_equal(adj.neighbors[b:e] - first, one.neighbors)
        np.testing.assert_array_equal(adj.boundary[first:first + n + 1], one.boundary)


# ------------------------------------------------------------------ smoothing
@pytest.mark.parametrize("w", [0.5, -0.53])
@pytest.mark.parametrize("case", ["sphere", "torus", "hemisphere"])
def test_one_step_against_the_dense_operator(case, w):
    """p + w (D^-1 A p - p) in float64 with the same float32 w.  The fp32 result's error, in units of u max|p| with
    u = 2^-24 and d the row's degree: the k-th addition rounds a partial sum of at most k max|p|, so the sum is off by
    at most (d (d + 1) / 2) u max|p| and the mean by (d + 1) / 2 of them; the division adds 1; the difference m - p
    (at most 2 max|p|) 2; times |w| <= 1, the product rounds 2 |w| more; the last addition (at most 3 max|p|) 3:
    below (d + 6) u max|p| for every d >= 1."""
    v, t = S.hemisphere() if case == "hemisphere" else M.mesh(case)
    adj = S.adjacency(case)
    p = S.noisy(v)
    nv = len(p)
    got = meshops.smooth_mesh_reference(p, t, iterations=1, lam=w, mu=None, pin=None)
    assert got.dtype == np.float32 and got.shape == p.shape
    A = np.zeros((nv, nv))
    A[np.repeat(np.arange(nv), np.diff(adj.offsets)), adj.neighbors] = 1.0
    deg = A.sum(1)
    assert deg.min() > 0
    p64 = p.astype(np.float64)
    want = p64 + float(np.float32(w)) * ((A @ p64) / deg[:, None] - p64)
    bound = (deg.max() + 6) * 2.0 ** -24 * np.abs(p).max()
    err = np.abs(got - want).max()
    print(f"{case} w={w}: max error {err:.3e}, bound {bound:.3e}, largest degree {int(deg.max())}")
    assert err <= bound
    assert np.abs(got - p).max() > 1e-3  # (and it did move)


def _volume_ratio(v, t, clean):
    return C.signed_volume(v, t) / C.signed_volume(clean, t)


def test_noisy_sphere_taubin_smooths_and_keeps_the_volume():
    v, t = M.mesh("sphere")
    assert len(v) == 576
    vn = S.noisy(v)
    taubin = meshops.smooth_mesh_reference(vn, t)  # the defaults: 10 iterations, 0.5 | -0.53
    lap = meshops.smooth_mesh_reference(vn, t, mu=None)
    ratio = S.radial_std(taubin, v) / S.radial_std(vn, v)
    vol_t, vol_l = _volume_ratio(taubin, t, v), _volume_ratio(lap, t, v)
    clean = _volume_ratio(meshops.smooth_mesh_reference(v, t), t, v)
    print(f"taubin: radial std ratio {ratio:.4f}, volume {vol_t:.4f}; laplacian: radial std ratio "
          f"{S.radial_std(lap, v) / S.radial_std(vn, v):.4f}, volume {vol_l:.4f}; clean sphere under taubin {clean:.4f}")
    assert ratio < 0.6
    assert abs(vol_t - 1.0) < 0.03
    assert vol_l < 0.9
    assert abs(clean - 1.0) < 0.02
    assert taubin.dtype == np.float32


def test_open_mesh_pins_its_rim():
    v, t = S.hemisphere()
    rim = S.adjacency("hemisphere").boundary
    pinned = meshops.smooth_mesh_reference(v, t, pin="boundary")
    np.testing.assert_array_equal(pinned[rim].view(np.int32), v[rim].view(np.int32))
    assert (np.abs(pinned[~rim] - v[~rim]).max(axis=1) > 0).all()
    free = meshops.smooth_mesh_reference(v, t, pin=None)
    assert np.abs(free[rim] - v[rim]).max() > 1e-2
    # a mask of one's own, and a precomputed adjacency
    mask = np.zeros(len(v), np.uint8)
    mask[::3] = 1
    own = meshops.smooth_mesh_reference(v, t, pin=mask, adjacency=S.adjacency("hemisphere"))
    np.testing.assert_array_equal(own[::3].view(np.int32), v[::3].view(np.int32))
    np.testing.assert_array_equal(own, meshops.smooth_mesh_reference(v, t, pin=torch.from_numpy(mask).bool()))


def test_smoothing_small_lists():
    p = np.arange(21, dtype=np.float32).reshape(7, 3) ** 2
    np.testing.assert_array_equal(meshops.smooth_mesh_reference(p, np.zeros((0, 3), np.int32), pin=None), p)
    out = meshops.smooth_mesh_reference(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert out.shape == (0, 3) and out.dtype == np.float32
    # one triangle: all three on the boundary (nothing moves when pinned); free, each moves halfway to the others' mean
    tri = np.array([[4, 2, 3]], np.int32)
    np.testing.assert_array_equal(meshops.smooth_mesh_reference(p[:6], tri, iterations=3), p[:6])
    got = meshops.smooth_mesh_reference(p[:6], tri, iterations=1, mu=None, pin=None)
    want = p[:6].copy()
    want[2] = p[2] + np.float32(0.5) * ((p[3] + p[4]) / np.float32(2) - p[2])
    want[3] = p[3] + np.float32(0.5) * ((p[2] + p[4]) / np.float32(2) - p[3])
    want[4] = p[4] + np.float32(0.5) * ((p[2] + p[3]) / np.float32(2) - p[4])
    np.testing.assert_array_equal(got, want)
    # the degenerate (1, 1, 3): 1 and 3 are neighbours, not boundary; a duplicated triangle has no boundary either
    got = meshops.smooth_mesh_reference(p[:4], np.array([[1, 1, 3]], np.int32), iterations=1, lam=1.0, mu=None)
    np.testing.assert_array_equal(got, p[[0, 3, 2, 1]])
    dup = meshops.smooth_mesh_reference(p[:3], np.array([[0, 1, 2], [0, 1, 2]], np.int32), iterations=1, mu=None)
    assert (dup != p[:3]).any()
    # iterations=0: the positions as they are, as float32
    np.testing.assert_array_equal(meshops.smooth_mesh_reference(p, tri, iterations=0), p)


def test_nan_spreads_over_neighbours_only():
    v, t = S.hemisphere()
    adj = S.adjacency("hemisphere")
    p = np.array(v)
    p[100, 1] = np.nan
    out = meshops.smooth_mesh_reference(p, t, iterations=1, mu=None, pin=None)
    ring = adj.neighbors[adj.offsets[100]:adj.offsets[101]]
    exp = np.zeros(p.shape, bool)
    exp[ring, 1] = True
    exp[100, 1] = True
    np.testing.assert_array_equal(np.isnan(out), exp)


# ------------------------------------------------------------------ argument errors
def test_argument_errors_come_before_any_launch(monkeypatch):
    def no_library():
        raise AssertionError("the argument checks must come before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    tri = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    v = torch.zeros(4, 3)
    for fn in (meshops.smooth_mesh, meshops.smooth_mesh_reference):
        with pytest.raises(ValueError, match="iterations"):
            fn(v, tri, iterations=-1)
        with pytest.raises(ValueError, match="finite"):
            fn(v, tri, lam=float("nan"))
        with pytest.raises(ValueError, match="finite"):
            fn(v, tri, mu=float("inf"))
        with pytest.raises(ValueError, match="mask"):
            fn(v, tri, pin=torch.zeros(5, dtype=torch.bool))
        with pytest.raises(ValueError, match="pin"):
            fn(v, tri, pin="rim")
        with pytest.raises(ValueError, match=r"\[V, 3\]"):
            fn(torch.zeros(4, 2), tri)
        with pytest.raises(ValueError, match=r"\[V, 3\]"):
            fn(torch.zeros(12), tri)
    assert meshops.smooth_mesh(v, tri, iterations=0) is v  # (and nothing was loaded)
    for bad, nv in (([[0, 1, 4]], 4), ([[0, -1, 2]], 4)):
        with pytest.raises(ValueError, match="outside"):
            meshops.vertex_adjacency(torch.tensor(bad, dtype=torch.int32), nv)
        with pytest.raises(ValueError, match="outside"):
            meshops.vertex_adjacency(np.array(bad, np.int64), nv)
        with pytest.raises(ValueError, match="outside"):
            meshops.smooth_mesh(torch.zeros(nv, 3), torch.tensor(bad, dtype=torch.int32))
        with pytest.raises(ValueError, match="outside"):
            meshops.vertex_adjacency_reference(np.array(bad), nv)
    with pytest.raises(ValueError, match=r"\[T, 3\]"):
        meshops.vertex_adjacency(torch.zeros(4, 2, dtype=torch.int32), 4)


def test_c_abi_validation():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def at(nbytes):
        return ctypes.c_void_p(p.value + nbytes)

    def err():
        return lib.anerf_last_error()
    # workspace: ints raw_off [V + 1] | cnt [V] | long_list [V] | n_long | 3 x blocks | raw [6 T]
    need = lib.anerf_mesh_adjacency_workspace(3, 1)
    assert need == 4 * (4 + 3 + 3 + 1 + 3 + 6) and lib.anerf_mesh_adjacency_workspace(0, 0) == 4 * 5
    assert lib.anerf_mesh_adjacency_workspace(1025, 0) == 4 * (1026 + 1025 + 1025 + 1 + 6)
    assert lib.anerf_mesh_adjacency_workspace(-1, 0) == 0 and b"anerf_mesh_adjacency_workspace" in err()
    assert lib.anerf_mesh_adjacency_workspace(3, (1 << 31) // 6 + 1) == 0
    assert lib.anerf_mesh_adjacency_workspace(3, (1 << 31) // 6) > 0  # (6 T = 2^31 - 2)
    # count
    assert lib.anerf_mesh_adjacency_count(None, 1, 3, p, need, p, p, p, None) == -1 and b"NULL" in err()
    assert lib.anerf_mesh_adjacency_count(p, 1, 3, None, need, p, p, p, None) == -1
    assert lib.anerf_mesh_adjacency_count(p, 1, 3, p, need, None, p, p, None) == -1
    assert lib.anerf_mesh_adjacency_count(p, 1, 3, p, need, p, None, p, None) == -1
    assert lib.anerf_mesh_adjacency_count(p, 1, 3, p, need, p, p, None, None) == -1
    assert lib.anerf_mesh_adjacency_count(p, -1, 3, p, need, p, p, p, None) == -1 and b"n_tri" in err()
    assert lib.anerf_mesh_adjacency_count(p, 1, -3, p, need, p, p, p, None) == -1 and b"n_vertices" in err()
    assert lib.anerf_mesh_adjacency_count(p, (1 << 31) // 6 + 1, 3, p, 1 << 40, p, p, p, None) == -1
    assert lib.anerf_mesh_adjacency_count(p, 1, 3, p, need - 1, p, p, p, None) == -1
    assert b"anerf_mesh_adjacency_workspace" in err()
    assert lib.anerf_mesh_adjacency_count(p, 1, 3, at(2), need, p, p, p, None) == -1 and b"aligned" in err()
    # emit
    assert lib.anerf_mesh_adjacency_emit(3, None, need, p, p, 6, None) == -1 and b"NULL" in err()
    assert lib.anerf_mesh_adjacency_emit(3, p, need, None, p, 6, None) == -1
    assert lib.anerf_mesh_adjacency_emit(3, p, need, p, None, 6, None) == -1
    assert lib.anerf_mesh_adjacency_emit(-3, p, need, p, p, 6, None) == -1 and b"n_vertices" in err()
    assert lib.anerf_mesh_adjacency_emit(3, p, need, p, p, -1, None) == -1
    assert lib.anerf_mesh_adjacency_emit(3, p, need, p, p, 1 << 31, None) == -1
    assert lib.anerf_mesh_adjacency_emit(3, p, 4 * 14 - 1, p, p, 6, None) == -1
    assert b"anerf_mesh_adjacency_workspace" in err()
    assert lib.anerf_mesh_adjacency_emit(3, at(2), need, p, p, 6, None) == -1 and b"aligned" in err()
    assert lib.anerf_mesh_adjacency_emit(0, p, need, p, None, 0, None) == 0  # (nothing to emit: no launch)
    # smooth: positions at 0, out at 64, scratch at 128 (3 vertices are 36 bytes each)
    def smooth(pos, nv, off, nb, ne, pin, it, flags, out, scr):
        return lib.anerf_mesh_smooth(pos, nv, off, nb, ne, pin, it, 0.5, -0.53, flags, out, scr, None)
    o, s = at(64), at(128)
    assert smooth(p, 3, p, p, 6, None, 1, 1, p, s) == -1 and b"overlap" in err()
    assert smooth(p, 3, p, p, 6, None, 1, 1, at(32), s) == -1 and b"overlap" in err()
    assert smooth(p, 3, p, p, 6, None, 1, 1, o, p) == -1 and b"overlap" in err()
    assert smooth(p, 3, p, p, 6, None, 1, 1, o, at(96)) == -1 and b"overlap" in err()
    assert smooth(None, 3, p, p, 6, None, 1, 1, o, s) == -1 and b"NULL" in err()
    assert smooth(p, 3, None, p, 6, None, 1, 1, o, s) == -1
    assert smooth(p, 3, p, None, 6, None, 1, 1, o, s) == -1 and b"neighbors" in err()
    assert smooth(p, 3, p, p, 6, None, 1, 1, None, s) == -1
    assert smooth(p, 3, p, p, 6, None, 1, 1, o, None) == -1 and b"scratch" in err()  # (Taubin: two steps)
    assert smooth(p, 3, p, p, 6, None, -1, 1, o, s) == -1 and b"iterations" in err()
    assert smooth(p, 3, p, p, 6, None, 1, 2, o, s) == -1 and b"flags" in err()
    assert smooth(p, -3, p, p, 6, None, 1, 1, o, s) == -1 and b"n_vertices" in err()
    assert smooth(p, 3, p, p, -6, None, 1, 1, o, s) == -1
    assert smooth(None, 0, None, None, 0, None, 5, 1, None, None) == 0  # (no vertices: nothing to do, no launch)

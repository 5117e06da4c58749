"""GPU: the mesh-component kernels (csrc/anerf_mesh.hip through meshops.mesh_components / compact_mesh / filter_mesh)
against the NumPy checkers of the same contract (themselves held to scipy and to mesh properties in
test_mesh_components.py) and against lists whose answer is known by construction, and the filter end to end through
mesh_from_grid, RayCaster.extract_mesh and render_mesh.  Every result is an integer or a copied row: all comparisons
are exact."""
import importlib

import numpy as np
import pytest
import torch

import _iso_cases as C
import _mesh_cases as M
from _golden import Golden

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
iso = importlib.import_module("a-nerf_amd.isosurface")
meshops = importlib.import_module("a-nerf_amd.meshops")


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _assert_components(got, ref, what):
    assert isinstance(got, meshops.MeshComponents)
    for name, g, r in zip(got._fields, got, ref):
        assert g.is_cuda and g.dtype == (torch.int32 if name in ("labels", "roots") else torch.int64), (what, name)
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg=f"{what}: {name}")


def _list(case):
    """(triangles, V, components) of a case: a named mesh, a relabelled mesh "name/kind", or a synthetic list."""
    if case in M.MESHES:
        v, t = M.mesh(case)
        return t, len(v), M.components(case)
    if "/" in case:
        return M.relabelled(*case.split("/"))
    return M.synthetic(case)


RELABELLED = [f"{n}/{k}" for n in M.MESHES for k in ("permuted", "reversed")]


@pytest.mark.parametrize("case", list(M.MESHES) + RELABELLED + list(M.SYNTHETIC))
def test_components_match(case):
    tri, nv, ref = _list(case)
    got = meshops.mesh_components(torch.from_numpy(np.array(tri)).cuda(), nv)
    _assert_components(got, ref, case)
    if case in M.MESHES:
        assert len(got.roots) == M.MESHES[case][2]


def test_raw_outputs_of_the_entry():
    """root / tri_count / vert_count / n_components as the C entry leaves them (include/anerf.h): the counts sit at
    the roots and are 0 elsewhere."""
    tri, nv, ref = _list("random33")
    t = torch.from_numpy(np.array(tri)).cuda()
    root, tc, vc, n = meshops._components_raw(t, nv)
    assert n == 358
    np.testing.assert_array_equal(root.cpu().numpy(), ref.roots[ref.labels])
    exp_t, exp_v = np.zeros(nv, np.int32), np.zeros(nv, np.int32)
    exp_t[ref.roots], exp_v[ref.roots] = ref.triangle_counts, ref.vertex_counts
    np.testing.assert_array_equal(tc.cpu().numpy(), exp_t)
    np.testing.assert_array_equal(vc.cpu().numpy(), exp_v)


def test_int64_and_host_input():
    tri, nv, ref = _list("blobs")
    _assert_components(meshops.mesh_components(torch.from_numpy(np.array(tri)).long(), nv), ref, "int64 host")
    _assert_components(meshops.mesh_components(np.array(tri), nv), ref, "numpy")


# ------------------------------------------------------------------ compaction
def _assert_filter(case, keep_largest, min_triangles):
    tri, nv, comp = _list(case)
    vertices = M.attributes(nv, seed=3)[0]
    a_f, a_u = M.attributes(nv)
    _, kept, exp_t = M.filter_expected(comp, tri, keep_largest, min_triangles)
    dev = [torch.from_numpy(np.array(x)).cuda() for x in (vertices, tri, a_f, a_u)]
    v, t, a = meshops.filter_mesh(dev[0], dev[1], {"f": dev[2], "u": dev[3]}, keep_largest=keep_largest,
                                  min_triangles=min_triangles)
    assert v.is_cuda and t.is_cuda and t.dtype == torch.int32 and v.dtype == torch.float32
    assert a["f"].dtype == torch.float32 and a["u"].dtype == torch.uint8
    assert tuple(v.shape) == (len(kept), 3) and tuple(t.shape) == (len(exp_t), 3)
    np.testing.assert_array_equal(t.cpu().numpy(), exp_t)
    np.testing.assert_array_equal(v.cpu().numpy(), vertices[kept])
    np.testing.assert_array_equal(a["f"].cpu().numpy(), a_f[kept])
    np.testing.assert_array_equal(a["u"].cpu().numpy(), a_u[kept])
    return v, t


@pytest.mark.parametrize("min_triangles", [0, 40])
@pytest.mark.parametrize("keep_largest", [1, 2])
@pytest.mark.parametrize("case", list(M.MESHES) + RELABELLED + list(M.SYNTHETIC))
def test_filter_matches(case, keep_largest, min_triangles):
    _assert_filter(case, keep_largest, min_triangles)


def test_filter_equals_the_numpy_reference_and_keeps_a_watertight_body():
    v, t = M.mesh("two_spheres")
    fv, ft = meshops.filter_mesh(torch.from_numpy(v.copy()).cuda(), torch.from_numpy(t.copy()).cuda(), keep_largest=1)
    rv, rt = meshops.filter_mesh_reference(v, t, keep_largest=1)
    np.testing.assert_array_equal(fv.cpu().numpy(), rv)
    np.testing.assert_array_equal(ft.cpu().numpy(), rt)
    assert len(ft) == 524 and not C.directed_edge_imbalance(rt) and C.euler(rv, rt) == 2
    # min_triangles alone; nothing kept; the defaults
    v3, t3 = (torch.from_numpy(x.copy()).cuda() for x in M.mesh("random33"))
    fv, ft = meshops.filter_mesh(v3, t3, min_triangles=49)
    assert len(ft) == 92772
    fv, ft, fa = meshops.filter_mesh(v3, t3, [v3], min_triangles=10 ** 6)
    assert tuple(fv.shape) == (0, 3) and tuple(ft.shape) == (0, 3) and tuple(fa[0].shape) == (0, 3)
    assert fv.is_cuda and ft.dtype == torch.int32
    fv, ft = meshops.filter_mesh(v3, t3)
    assert fv is v3 and ft is t3


def _assert_compact(keep, tri, what):
    vm, kept, out = meshops.compact_mesh(torch.from_numpy(keep).cuda(), torch.from_numpy(np.array(tri)).cuda())
    evm, ekept, eout = M.compact_expected(keep, tri)
    assert vm.dtype == kept.dtype == out.dtype == torch.int32
    np.testing.assert_array_equal(vm.cpu().numpy(), evm, err_msg=what)
    np.testing.assert_array_equal(kept.cpu().numpy(), ekept, err_msg=what)
    np.testing.assert_array_equal(out.cpu().numpy(), eout, err_msg=what)
    return kept, out


def test_compact_masks():
    v, tri = M.mesh("blobs")
    nv = len(v)
    rng = np.random.default_rng(21)
    first_off = np.ones(nv, np.uint8)
    first_off[0] = 0
    last_off = np.ones(nv, np.uint8)
    last_off[-1] = 0
    _assert_compact(first_off, tri, "first dropped, last kept")
    _assert_compact(last_off, tri, "first kept, last dropped")
    _assert_compact((rng.random(nv) < 0.7).astype(np.uint8) * 255, tri, "random mask, values 0 / 255")
    _assert_compact(np.zeros(nv, np.uint8), tri, "nothing kept")
    _assert_compact(np.ones(nv, bool), tri, "bool mask, everything kept")
    _assert_compact(np.ones(5, np.uint8), np.zeros((0, 3), np.int32), "no triangles")
    _assert_compact(np.zeros(0, np.uint8), np.zeros((0, 3), np.int32), "no vertices")


def test_compact_alternating_runs_of_the_strip():
    tri, nv, _ = M.strip()
    keep = ((np.arange(nv) // 1000) % 2 == 0).astype(np.uint8)
    kept, out = _assert_compact(keep, tri, "alternating runs")
    # by construction: 150 whole runs and the 2 vertices of run 300; 998 triangles inside each whole run
    assert len(kept) == 150 * 1000 + 2 and len(out) == 150 * 998
    i = np.arange(150 * 998)
    first = (i // 998) * 1000 + i % 998  # new ids are consecutive within a run: the triangle's first new id
    np.testing.assert_array_equal(out.cpu().numpy(), (first[:, None] + np.arange(3)).astype(np.int32))
    old = (i // 998) * 2000 + i % 998
    np.testing.assert_array_equal(kept.cpu().numpy()[first], old)


@pytest.mark.parametrize("nv", M.TILE_EDGES)
def test_compact_at_the_scan_tile_edges(nv):
    """One tile of 1024 items and the 256 tiles of one round of the block-sum scan, each -1, +0, +1 vertices: runs of
    5 kept / 5 dropped, so every tile counts vertices and triangles; the last vertex is kept at each of these sizes,
    and in the + 1 lists it is the last tile's only item (its new id is that tile's base)."""
    tri = M.strip_triangles(nv)
    keep = ((np.arange(nv) // 5) % 2 == 0).astype(np.uint8)
    kept, out = _assert_compact(keep, tri, f"strip of {nv} vertices")
    runs, tail = divmod(nv, 10)  # by construction: 5 vertices and 3 triangles per whole kept run
    assert len(kept) == 5 * runs + min(tail, 5) and len(out) == 3 * runs + max(min(tail, 5) - 2, 0)
    assert int(kept[-1]) == nv - 1


def test_deterministic_and_stream_independent():
    tri, nv, ref = _list("random33/permuted")
    t = torch.from_numpy(np.array(tri)).cuda()
    v = torch.from_numpy(M.attributes(nv)[0]).cuda()

    def run():
        return tuple(meshops.mesh_components(t, nv)) + tuple(meshops.filter_mesh(v, t, keep_largest=2, min_triangles=40))
    a, b = run(), run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = run()
    s.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    _assert_components(meshops.MeshComponents(*c[:4]), ref, "side stream")


# ------------------------------------------------------------------ integration
def test_mesh_from_grid_queries_only_the_kept_vertices():
    # (+ 1, threshold 1: mesh_from_grid clamps at 0 as it reads, and the two spheres' outside is negative)
    grid = torch.from_numpy(C.two_spheres_field() + np.float32(1.0)).cuda()
    kps = torch.zeros(1, 1, 3)
    seen = []

    def stub(pts, dirs, cams):
        seen.append((pts.shape[0], dirs.shape[0]))
        return torch.zeros(pts.shape[0], 4, device=pts.device)
    pv, pt, pa = iso.mesh_from_grid(grid, kps, 1.0, 23, 1.0, coords="index", normals=True)
    v, t, a = iso.mesh_from_grid(grid, kps, 1.0, 23, 1.0, coords="index", normals=True, colors=True, radiance=stub,
                                 keep_largest=1)
    assert len(pt) == 1048 and len(t) == 524 and 0 < len(v) < len(pv)
    assert seen == [(len(v), len(v))]
    fv, ft, fa = meshops.filter_mesh(pv, pt, pa, keep_largest=1)
    assert torch.equal(v, fv) and torch.equal(t, ft) and torch.equal(a["normals"], fa["normals"])
    assert tuple(a["colors"].shape) == (len(v), 3)
    assert not C.directed_edge_imbalance(t.cpu().numpy()) and C.euler(v.cpu().numpy(), t.cpu().numpy()) == 2
    # the second sphere alone has rank 1: keep_largest=2 keeps all, and nothing kept queries nothing
    v2, t2 = iso.mesh_from_grid(grid, kps, 1.0, 23, 1.0, coords="index", keep_largest=2)
    assert torch.equal(v2, pv) and torch.equal(t2, pt)
    seen.clear()
    v0, t0, a0 = iso.mesh_from_grid(grid, kps, 1.0, 23, 1.0, colors=True, radiance=stub, min_triangles=525)
    assert seen == [] and tuple(v0.shape) == (0, 3) and tuple(t0.shape) == (0, 3) and tuple(a0["colors"].shape) == (0, 3)


THR = 0.3  # (test_gpu_isosurface.py: no grid value of dm_fine_d8w256 is near it)


def _pose(g):
    return torch.from_numpy(g["kps"]), torch.from_numpy(g["skts"]), torch.from_numpy(g["bones"])


def test_extract_mesh_forwards_the_filter():
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    kw = dict(radius=radius, res=res, threshold=THR)
    for coords in ("index", "unit", "world"):
        pv, pt, pa = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, **kw)
        v, t, a = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, keep_largest=1, **kw)
        fv, ft, fa = meshops.filter_mesh(pv, pt, pa, keep_largest=1)
        assert len(t) > 0 and torch.equal(v, fv) and torch.equal(t, ft) and torch.equal(a["normals"], fa["normals"])
    pv, pt = rc.extract_mesh(kps, skts, bones, **kw)
    v, t = rc.extract_mesh(kps, skts, bones, min_triangles=len(pt) + 1, **kw)
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3)
    v, t, a = rc.extract_mesh(kps, skts, bones, colors=True, keep_largest=1, **kw)
    fv, ft = meshops.filter_mesh(pv, pt, keep_largest=1)
    assert torch.equal(v, fv) and torch.equal(t, ft) and tuple(a["colors"].shape) == (len(v), 3)


def test_staged_caster_forwards_the_filter():
    g = Golden("sgd1_relpos_mrb2_density")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    kw = dict(radius=radius, res=res, threshold=2.0, coords="index")
    for caster in (rc._staged.eval_caster(), rc):
        pv, pt = caster.extract_mesh(kps, skts, bones, **kw)
        v, t = caster.extract_mesh(kps, skts, bones, keep_largest=1, **kw)
        fv, ft = meshops.filter_mesh(pv, pt, keep_largest=1)
        assert len(pt) > 0 and torch.equal(v, fv) and torch.equal(t, ft)


def test_render_mesh_writes_the_filtered_mesh(tmp_path):
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    data = {"kp": torch.cat([kps, kps + 0.04]), "skts": torch.cat([skts, skts]), "bones": torch.cat([bones, bones])}
    out = anerf.render_mesh(str(tmp_path), {"ray_caster": rc, "preproc_kwargs": {}}, data, radius=radius, res=res,
                            threshold=THR, normals=True, keep_largest=1)
    assert len(out) == 2
    for i, (v, t, a) in enumerate(out):
        pv, pt, pa = rc.extract_mesh(data["kp"][i:i + 1], data["skts"][i:i + 1], data["bones"][i:i + 1], radius=radius,
                                     res=res, threshold=THR, normals=True)
        fv, ft, fa = meshops.filter_mesh(pv, pt, pa, keep_largest=1)
        assert len(ft) > 0 and torch.equal(v, fv) and torch.equal(t, ft)
        rv, rt, ra = iso.read_ply(str(tmp_path / "meshes" / f"{i:03d}.ply"), attributes=True)
        np.testing.assert_array_equal(rv, fv.cpu().numpy())
        np.testing.assert_array_equal(rt, ft.cpu().numpy())
        np.testing.assert_array_equal(ra["normals"], fa["normals"].cpu().numpy())

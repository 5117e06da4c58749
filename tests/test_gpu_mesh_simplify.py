"""GPU: vertex clustering (csrc/anerf_simplify.hip through meshops.simplify_mesh) against the NumPy checker of the same
contract (itself held to a brute force and to the contract's consequences in test_mesh_simplify.py), and simplify= end
to end through extract_mesh and render_mesh.  Every decision of the contract is an integer one and every rounding has
its place: all comparisons are exact, positions through their int32 views."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _mesh_cases as M
import _simplify_cases as C
from _golden import Golden

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
iso = importlib.import_module("a-nerf_amd.isosurface")
meshops = importlib.import_module("a-nerf_amd.meshops")
_lib = importlib.import_module("a-nerf_amd._lib")


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def _assert_same(got, ref, what):
    """Zero differing words between a device result and the checker's, in all four outputs."""
    assert isinstance(got, meshops.SimplifiedMesh)
    for name, g, r in zip(C.FIELDS, got, ref):
        assert g.is_cuda and g.dtype == (torch.float32 if name == "vertices" else torch.int32), (what, name)
        assert tuple(g.shape) == r.shape, (what, name, tuple(g.shape), r.shape)
        g = g.cpu().numpy()
        diff = int((g.view(np.int32) != r.view(np.int32)).sum())
        print(f"{what}: {name}: {diff} differing words of {r.size}")
        assert diff == 0, (what, name)


def _run(v, t, cell, origin=None, **kw):
    out = meshops.simplify_mesh(_dev(v), _dev(t), cell, origin=origin, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cell", C.CELLS)
@pytest.mark.parametrize("case", C.NAMED)
def test_named_meshes_match(case, cell):
    v, t = C.mesh(case)
    _assert_same(_run(v, t, cell), C.reference(case, cell), f"{case} at {cell}")


@pytest.mark.parametrize("origin", ((0, 0, 0), (-1.25, -0.5, -3)))
def test_a_given_origin(origin):
    v, t = C.mesh("blobs")
    for cell in C.CELLS:
        _assert_same(_run(v, t, cell, origin), C.reference("blobs", cell, origin), f"blobs from {origin} at {cell}")


@pytest.mark.parametrize("case", ("blobs/permuted", "blobs/reversed", "random33/permuted", "random33/reversed"))
def test_relabelled_meshes_match(case):
    """The vertices of a cell arrive in any order: the smallest id is the representative all the same."""
    v, t = C.mesh(case)
    _assert_same(_run(v, t, 2.0), C.reference(case, 2.0), case)


@pytest.mark.parametrize("nv", M.TILE_EDGES)
def test_at_the_scan_tile_edges(nv):
    v, t = C.strip(nv)
    ref = meshops.simplify_mesh_reference(v, t, 1.0, origin=(0, 0, 0))
    assert 0 < len(ref.vertices) < nv and 0 < len(ref.triangles) < len(t)
    assert len(ref.vertices) == (nv + 3) // 4 * 2 - (1 if nv % 4 == 1 else 0)  # (two per cell column; the last: one)
    _assert_same(_run(v, t, 1.0, (0, 0, 0)), ref, f"strip of {nv}")


@pytest.mark.parametrize("n", (32, 33, 40, 5000))
def test_a_long_owner_row(n):
    """Nothing merges: the hub owns all n triangles, a row on either side of the switch from the triangles' own
    threads to the workgroup sort, and far beyond it."""
    v, t = C.wheel(n)
    got = _run(v, t, 1.0, (0, 0, 0))
    np.testing.assert_array_equal(got.triangles.cpu().numpy(), t)
    np.testing.assert_array_equal(got.vertex_map.cpu().numpy(), np.arange(n + 1))
    _assert_same(got, meshops.simplify_mesh_reference(v, t, 1.0, origin=(0, 0, 0)), f"wheel of {n}")


def test_a_long_row_of_copies():
    """5000 triangles around the hub whose rim falls into 7 cells: 7 sets survive, each the first of its copies; the
    last triangle, (0, 5000, 1) -> (0, 2, 1), is the first one's set in the opposite winding and goes too."""
    v, t = C.wheel(5000, period=7)
    got = _run(v, t, 1.0, (0, 0, 0))
    assert got.vertices.shape == (8, 3)
    want = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 6], [0, 6, 7], [0, 7, 1]]
    np.testing.assert_array_equal(got.triangles.cpu().numpy(), np.array(want, np.int32))
    np.testing.assert_array_equal(got.representatives.cpu().numpy(), np.arange(8))
    np.testing.assert_array_equal(got.vertex_map.cpu().numpy()[1:], 1 + np.arange(5000) % 7)
    _assert_same(got, meshops.simplify_mesh_reference(v, t, 1.0, origin=(0, 0, 0)), "wheel of 5000 in 7 cells")


def test_many_long_owner_rows():
    """1100 hubs that own 33 triangles each, more than the 1024 workgroups of the long-row kernel: 76 of them sort a
    second row.  Nothing merges."""
    v, t = C.wheels("many_wheels")
    assert (len(v), len(t)) == (37400, 36300)
    got = _run(v, t, 1.0, (0, 0, 0))
    np.testing.assert_array_equal(got.triangles.cpu().numpy(), t)
    np.testing.assert_array_equal(got.vertex_map.cpu().numpy(), np.arange(37400))
    _assert_same(got, meshops.simplify_mesh_reference(v, t, 1.0, origin=(0, 0, 0)), "many_wheels")


def test_mixed_owner_rows():
    """wheel33, wheel40 and wheel5000 in one list: two rows just over the switch and a far longer one on the same
    list of long rows."""
    v, t = C.wheels("mixed_wheels")
    assert (len(v), len(t)) == (5076, 5073)
    _assert_same(_run(v, t, 1.0, (0, 0, 0)), meshops.simplify_mesh_reference(v, t, 1.0, origin=(0, 0, 0)),
                 "mixed_wheels")


@pytest.mark.parametrize("name", ("no_triangles", "no_vertices", "one_triangle", "degenerate", "duplicated"))
def test_small_lists(name):
    v, t = C.small(name)
    got = _run(v, t.reshape(-1, 3), 0.25)
    _assert_same(got, meshops.simplify_mesh_reference(v, t.reshape(-1, 3), 0.25), name)
    assert got.triangles.shape[0] == {"one_triangle": 1, "duplicated": 1}.get(name, 0)


def test_c_entry_drops_what_it_cannot_place():
    """Four vertices, one of them NaN, and two triangles, one of which uses it: that vertex gets -1 and its triangle
    is dropped (meshops.simplify_mesh refuses such vertices before it launches anything; the C entry must be safe)."""
    lib = _lib.load()
    v = _dev(np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, float("nan"), 0.5], [0.5, 1.5, 0.5]], np.float32))
    t = _dev(np.array([[0, 1, 2], [3, 1, 0]], np.int32))
    o, d = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int32 * 3)(2, 2, 1)
    need = lib.anerf_mesh_simplify_workspace(4, 2, 4)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    totals = torch.empty(2, device="cuda", dtype=torch.int64)
    stream = _lib.stream_handle(v.device)
    args = (_lib.ptr(v), 4, _lib.ptr(t), 2, ctypes.cast(o, ctypes.c_void_p), 1.0, ctypes.cast(d, ctypes.c_void_p),
            _lib.ptr(ws), need)
    _lib.check(lib.anerf_mesh_simplify_count(*args, _lib.ptr(totals), stream), "count")
    assert totals.tolist() == [3, 1]
    out_v = torch.empty((3, 3), device="cuda")
    out_t = torch.empty((1, 3), device="cuda", dtype=torch.int32)
    vmap = torch.empty(4, device="cuda", dtype=torch.int32)
    reps = torch.empty(3, device="cuda", dtype=torch.int32)
    _lib.check(lib.anerf_mesh_simplify_emit(*args, _lib.ptr(out_v), 3, _lib.ptr(out_t), 1, _lib.ptr(vmap),
                                            _lib.ptr(reps), stream), "emit")
    torch.cuda.synchronize()
    assert vmap.tolist() == [0, 1, -1, 2] and reps.tolist() == [0, 1, 3] and out_t.tolist() == [[2, 1, 0]]
    assert out_v.tolist() == [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]
    # an id outside [0, V) and a vertex outside the grid go the same way
    t2 = _dev(np.array([[0, 1, 4], [3, 1, 0], [0, -1, 3]], np.int32))
    v2 = v.clone()
    v2[2] = torch.tensor([0.5, 0.5, 1.5])  # (cell (0, 0, 1) of dims (2, 2, 1))
    need2 = lib.anerf_mesh_simplify_workspace(4, 3, 4)
    ws2 = torch.empty(need2, device="cuda", dtype=torch.uint8)
    args2 = (_lib.ptr(v2), 4, _lib.ptr(t2), 3) + args[4:7] + (_lib.ptr(ws2), need2)
    _lib.check(lib.anerf_mesh_simplify_count(*args2, _lib.ptr(totals), stream), "count")
    assert totals.tolist() == [3, 1]


def test_two_runs_are_bit_identical():
    v, t = C.mesh("random33")
    a, b = _run(v, t, 1.0), _run(v, t, 1.0)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_attrs_follow_the_representatives():
    v, t = C.mesh("blobs")
    f, u = M.attributes(len(v))
    got = _run(v, t, 2.0, attrs={"f": _dev(f), "u": _dev(u)})
    reps = got.representatives.cpu().numpy()
    assert got.attrs["f"].dtype == torch.float32 and got.attrs["u"].dtype == torch.uint8
    np.testing.assert_array_equal(got.attrs["f"].cpu().numpy(), f[reps])
    np.testing.assert_array_equal(got.attrs["u"].cpu().numpy(), u[reps])
    as_list = _run(v, t, 2.0, attrs=[u])  # (a host array is moved to the device)
    assert isinstance(as_list.attrs, list) and as_list.attrs[0].is_cuda
    np.testing.assert_array_equal(as_list.attrs[0].cpu().numpy(), u[reps])
    # host and int64 inputs
    host = meshops.simplify_mesh(np.array(v), t.astype(np.int64), 2.0)
    _assert_same(host, C.reference("blobs", 2.0), "host input")


# ------------------------------------------------------------------ integration
THR = 0.3  # (test_gpu_isosurface.py: no grid value of dm_fine_d8w256 is near it)


def _pose(g):
    return torch.from_numpy(g["kps"]), torch.from_numpy(g["skts"]), torch.from_numpy(g["bones"])


def test_extract_mesh_simplifies_after_the_smoothing_and_before_the_colours():
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    kw = dict(radius=radius, res=res, threshold=THR, keep_largest=1, smooth=2)
    vi, ti, ai = rc.extract_mesh(kps, skts, bones, coords="index", normals=True, **kw)
    assert len(ti) > 0
    ref = meshops.simplify_mesh(vi, ti, 2.0, attrs=[ai["normals"]], origin=(0, 0, 0))
    assert 0 < len(ref.triangles) < len(ti) and 0 < len(ref.vertices) < len(vi)
    _assert_same(ref, meshops.simplify_mesh_reference(vi, ti, 2.0, origin=(0, 0, 0)), "the extracted body")
    sv, n_index = ref.vertices, ref.attrs[0]
    kp0 = kps.to(sv.device, torch.float32).reshape(-1, 3)[0]
    world = (-radius + (2.0 * radius / res) * sv[:, [1, 0, 2]]) + kp0
    mapped = {"index": sv, "unit": sv / res - .5, "world": world}
    # the colours: the field at the SIMPLIFIED world vertices, each seen against its representative's world normal
    _, wt, wa = rc.extract_mesh(kps, skts, bones, coords="world", normals=True, **kw)
    normals = {"index": n_index, "unit": n_index, "world": wa["normals"][ref.representatives.long()]}
    inward = 0.0 - normals["world"]
    dirs = torch.where((inward == 0).all(-1, keepdim=True), kp0 - world, inward).contiguous()
    raw = rc.render_pts_radiance(world.contiguous(), dirs, kps, skts, bones)
    colors = torch.sigmoid(raw[:, :3].to(torch.float32))
    for coords in ("index", "unit", "world"):
        v, t, a = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, colors=True, simplify=2.0, **kw)
        assert torch.equal(v.view(torch.int32), mapped[coords].view(torch.int32)), coords
        if coords == "world":  # (the winding's flag is reversed there before the extraction)
            want_t = meshops.simplify_mesh(vi, wt, 2.0, origin=(0, 0, 0)).triangles
        else:
            want_t = ref.triangles
        assert torch.equal(t, want_t), coords
        assert torch.equal(a["normals"], normals[coords]), coords
        assert torch.equal(a["colors"], colors), coords
    # simplify=None is today's call, bit for bit
    for coords in ("index", "world"):
        a = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, colors=True, simplify=None, **kw)
        b = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, colors=True, **kw)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
        assert all(torch.equal(a[2][k].view(torch.int32), b[2][k].view(torch.int32)) for k in ("normals", "colors"))
    # face normals are those of the final mesh
    v, t, a = rc.extract_mesh(kps, skts, bones, coords="index", normals="faces", simplify=2.0, **kw)
    assert torch.equal(v, sv) and torch.equal(t, ref.triangles)
    assert torch.equal(a["normals"], meshops.vertex_normals(v, t))
    with pytest.raises(ValueError, match="cell"):
        rc.extract_mesh(kps, skts, bones, simplify=0.0, **kw)


def test_staged_caster_forwards_simplify():
    g = Golden("sgd1_relpos_mrb2_density")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    kw = dict(radius=radius, res=res, threshold=2.0, coords="index", keep_largest=1)
    for caster in (rc._staged.eval_caster(), rc):
        pv, pt = caster.extract_mesh(kps, skts, bones, **kw)
        v, t = caster.extract_mesh(kps, skts, bones, simplify=2.0, **kw)
        assert 0 < len(t) < len(pt)
        ref = meshops.simplify_mesh_reference(pv, pt, 2.0, origin=(0, 0, 0))
        np.testing.assert_array_equal(v.cpu().numpy().view(np.int32), ref.vertices.view(np.int32))
        np.testing.assert_array_equal(t.cpu().numpy(), ref.triangles)


def test_render_mesh_writes_the_simplified_mesh(tmp_path):
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    data = {"kp": kps, "skts": skts, "bones": bones}
    rk = {"ray_caster": rc, "preproc_kwargs": {}}
    kw = dict(radius=radius, res=res, threshold=THR, normals=True, keep_largest=1)
    out = anerf.render_mesh(str(tmp_path / "s"), rk, data, simplify=2.0, **kw)
    v, t, a = out[0]
    ev, et, ea = rc.extract_mesh(kps, skts, bones, simplify=2.0, **kw)
    assert len(t) > 0 and torch.equal(v, ev) and torch.equal(t, et) and torch.equal(a["normals"], ea["normals"])
    rv, rt, ra = iso.read_ply(str(tmp_path / "s" / "meshes" / "000.ply"), attributes=True)
    np.testing.assert_array_equal(rv.view(np.int32), v.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(rt, t.cpu().numpy())
    np.testing.assert_array_equal(ra["normals"], a["normals"].cpu().numpy())
    # simplify=None: the file of the call without the argument, byte for byte, and a denser one
    anerf.render_mesh(str(tmp_path / "a"), rk, data, simplify=None, **kw)
    plain = anerf.render_mesh(str(tmp_path / "b"), rk, data, **kw)
    assert (tmp_path / "a" / "meshes" / "000.ply").read_bytes() == (tmp_path / "b" / "meshes" / "000.ply").read_bytes()
    assert len(plain[0][0]) > len(v) and len(plain[0][1]) > len(t)

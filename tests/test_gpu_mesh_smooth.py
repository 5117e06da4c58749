"""GPU: the adjacency and smoothing kernels (csrc/anerf_mesh.hip through meshops.vertex_adjacency / smooth_mesh) against
the NumPy checkers of the same contract (themselves held to scipy, to a dense operator and to what smoothing is for in
test_mesh_smooth.py), and smooth= end to end through extract_mesh and render_mesh.  The adjacency is integers; every
operation of a smoothing step is a correctly rounded fp32 operation on both sides, in the same order: all comparisons
are exact, positions through their int32 views."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _mesh_cases as M
import _smooth_cases as S
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


def _assert_adjacency(got, ref, what):
    assert isinstance(got, meshops.VertexAdjacency)
    for name, g, r in zip(got._fields, got, ref):
        assert g.is_cuda and g.dtype == (torch.bool if name == "boundary" else torch.int32), (what, name)
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg=f"{what}: {name}")


def _assert_bits(got, ref, what):
    """Zero differing 32-bit words between a device result and the checker's."""
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape, what
    diff = int((got.cpu().numpy().view(np.int32) != ref.view(np.int32)).sum())
    print(f"{what}: {diff} differing words of {ref.size}")
    assert diff == 0, what


# ------------------------------------------------------------------ adjacency
RELABELLED = tuple(f"{n}/{k}" for n in S.CLOSED for k in ("permuted", "reversed"))
# wheel32 / wheel33: 64 and 66 listed pairs at the hub, either side of the switch to the workgroup sort; wheel40: a
# long row sorted over LDS; wheel5000: 10,000 listed pairs, padded to 16,384, sorted over global memory
WHEELS = ("wheel32", "wheel33", "wheel40", "wheel5000")


@pytest.mark.parametrize("case", S.CLOSED + RELABELLED + ("hemisphere",) + S.SMALL + ("strip", "strip_shuffled") + WHEELS)
def test_adjacency_matches(case):
    tri, nv = S.triangle_list(case)
    _assert_adjacency(meshops.vertex_adjacency(_dev(tri), nv), S.adjacency(case), case)


@pytest.mark.parametrize("nv", M.TILE_EDGES)
def test_adjacency_at_the_scan_tile_edges(nv):
    """Strips of one tile of 1024 vertices and of the 256 tiles of one round of the base scan, each -1, +0, +1: both
    scans of the count entry (raw offsets, then offsets) and the last tile's base in the emit pass."""
    tri = M.strip_triangles(nv)
    adj = meshops.vertex_adjacency(_dev(tri), nv)
    _assert_adjacency(adj, meshops.vertex_adjacency_reference(tri, nv), f"strip of {nv} vertices")
    assert int(adj.offsets[-1]) == 4 * nv - 6  # by construction: degree 4 inside, 2 and 3 at either end


def test_wheel_by_construction():
    tri, nv = S.wheel(5000)
    adj = meshops.vertex_adjacency(_dev(tri), nv)
    off = adj.offsets.cpu().numpy()
    assert off[1] == 5000 and (np.diff(off)[1:] == 3).all()
    np.testing.assert_array_equal(adj.neighbors[:5000].cpu().numpy(), np.arange(1, 5001))
    b = adj.boundary.cpu().numpy()
    assert not b[0] and b[1:].all()


def test_adjacency_of_many_long_rows():
    """1100 hubs of 66 listed pairs each, more than the 1024 workgroups of the long-row kernels: 76 of them sort and
    emit a second row, over the same LDS."""
    tri, nv = S.triangle_list("many_wheels")
    assert (nv, len(tri)) == (37400, 36300)
    adj = meshops.vertex_adjacency(_dev(tri), nv)
    _assert_adjacency(adj, S.adjacency("many_wheels"), "many_wheels")
    off = adj.offsets.cpu().numpy()
    assert off[-1] == 145200 and np.diff(off).max() == 33  # by construction: 33 + 33 x 3 per wheel
    assert int(adj.boundary.sum()) == 36300  # every rim vertex, no hub


def test_adjacency_of_mixed_long_rows():
    """wheel33, wheel40 and wheel5000 in one list: rows sorted over LDS and a row sorted over global memory on the
    same list of long rows."""
    tri, nv = S.triangle_list("mixed_wheels")
    assert (nv, len(tri)) == (5076, 5073)
    _assert_adjacency(meshops.vertex_adjacency(_dev(tri), nv), S.adjacency("mixed_wheels"), "mixed_wheels")


def test_adjacency_int64_and_host_input():
    tri, nv = S.triangle_list("blobs")
    ref = S.adjacency("blobs")
    _assert_adjacency(meshops.vertex_adjacency(torch.from_numpy(np.array(tri)).long(), nv), ref, "int64 host")
    _assert_adjacency(meshops.vertex_adjacency(np.array(tri), nv), ref, "numpy")
    _assert_adjacency(meshops.vertex_adjacency(_dev(tri).long(), nv), ref, "int64 device")


def test_out_of_range_id_raises_before_a_launch(monkeypatch):
    def no_library():
        raise AssertionError("the range check must come before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    tri = torch.tensor([[0, 1, 2], [2, 1, 4]], dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="outside"):
        meshops.vertex_adjacency(tri, 4)
    with pytest.raises(ValueError, match="outside"):
        meshops.smooth_mesh(torch.zeros(4, 3).cuda(), tri)


# ------------------------------------------------------------------ smoothing
def _positions(case):
    """(positions float32 [V, 3], triangles) of a smoothing case, the positions noisy so that every step moves them."""
    if case == "hemisphere":
        v, t = S.hemisphere()
    elif case.startswith("wheel"):
        t, nv = S.triangle_list(case)
        return S.wheel_vertices(nv - 1), t
    else:
        v, t = M.mesh(case)
    return S.noisy(v), t


# (every Taubin count is an even number of steps: the odd Laplacian counts are the ones that end through the other
# buffer, 1 step being the case with no scratch use at all)
@pytest.mark.parametrize("case, kw", [
    ("random33", dict(iterations=1, mu=None)),
    ("random33", dict(iterations=3)),
    ("random33", dict()),  # the defaults: 10 Taubin iterations
    ("random33", dict(iterations=4, mu=None)),
    ("random33", dict(iterations=5, mu=None)),
    ("sphere", dict(iterations=2, lam=0.33, mu=-0.34)),
    ("wheel5000", dict(iterations=2, pin=None)),
    ("wheel5000", dict(iterations=3, mu=None)),  # the rim is pinned: only the hub moves
    ("wheel40", dict(iterations=1, pin=None)),
])
def test_smoothing_is_bit_identical(case, kw):
    p, t = _positions(case)
    got = meshops.smooth_mesh(_dev(p), _dev(t), **kw)
    ref = meshops.smooth_mesh_reference(p, t, **kw)
    _assert_bits(got, ref, f"{case} {kw}")
    assert (ref != p).any()


def test_open_mesh_and_the_three_pin_forms():
    p, t = _positions("hemisphere")
    rim = S.adjacency("hemisphere").boundary
    mask = np.zeros(len(p), np.uint8)
    mask[::3] = 1
    dp, dt = _dev(p), _dev(t)
    got = meshops.smooth_mesh(dp, dt, pin="boundary")
    _assert_bits(got, meshops.smooth_mesh_reference(p, t, pin="boundary"), "pin='boundary'")
    np.testing.assert_array_equal(got.cpu().numpy()[rim].view(np.int32), p[rim].view(np.int32))
    assert (got.cpu().numpy()[~rim] != p[~rim]).any(axis=1).all()
    free = meshops.smooth_mesh(dp, dt, pin=None)
    _assert_bits(free, meshops.smooth_mesh_reference(p, t, pin=None), "pin=None")
    assert (free.cpu().numpy()[rim] != p[rim]).any()
    for m in (_dev(mask), _dev(mask).bool(), mask):
        _assert_bits(meshops.smooth_mesh(dp, dt, pin=m), meshops.smooth_mesh_reference(p, t, pin=mask), "pin=mask")


def test_nan_spreads_as_in_the_checker():
    p, t = _positions("hemisphere")
    p[100, 1] = np.nan
    for kw in (dict(iterations=1, mu=None, pin=None), dict(iterations=2, pin=None)):
        got = meshops.smooth_mesh(_dev(p), _dev(t), **kw)
        ref = meshops.smooth_mesh_reference(p, t, **kw)
        np.testing.assert_array_equal(np.isnan(got.cpu().numpy()), np.isnan(ref))
        assert 1 < np.isnan(ref).sum() < ref.size // 3
        _assert_bits(got, ref, f"one NaN vertex {kw}")


def test_iterations_zero_and_adjacency_reuse():
    p, t = _positions("blobs")
    dp, dt = _dev(p), _dev(t)
    assert meshops.smooth_mesh(dp, dt, iterations=0) is dp
    adj = meshops.vertex_adjacency(dt, len(p))
    a = meshops.smooth_mesh(dp, dt, iterations=3)
    b = meshops.smooth_mesh(dp, None, iterations=3, adjacency=adj)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _assert_bits(b, meshops.smooth_mesh_reference(p, t, iterations=3, adjacency=S.adjacency("blobs")), "adjacency=")
    # no vertices: an empty result
    e = meshops.smooth_mesh(torch.zeros(0, 3).cuda(), torch.zeros((0, 3), dtype=torch.int32).cuda())
    assert tuple(e.shape) == (0, 3) and e.is_cuda


def test_deterministic_stream_independent_and_input_untouched():
    p, t = _positions("random33")
    tri, nv, _ = M.relabelled("random33", "permuted")
    dp, dt, dr = _dev(p), _dev(t), _dev(tri)
    keep = dp.clone()

    def run():
        return tuple(meshops.vertex_adjacency(dr, nv)) + (meshops.smooth_mesh(dp, dt, iterations=3),)
    a, b = run(), run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = run()
    s.synchronize()
    for x, y, z in zip(a, b, c):
        x, y, z = (w.view(torch.int32) if w.dtype == torch.float32 else w for w in (x, y, z))
        assert torch.equal(x, y) and torch.equal(x, z)
    _assert_adjacency(meshops.VertexAdjacency(*c[:3]), S.adjacency("random33/permuted"), "side stream")
    assert torch.equal(dp.view(torch.int32), keep.view(torch.int32))


# ------------------------------------------------------------------ the C entries' guards
def _smooth_raw(pos, offsets, neighbors, out, scratch, iterations=1, flags=0, nv=None):
    lib = _lib.load()
    nv = pos.shape[0] if nv is None else nv
    return lib.anerf_mesh_smooth(_lib.ptr(pos), nv, _lib.ptr(offsets), _lib.ptr(neighbors), neighbors.shape[0], None,
                                 iterations, 0.5, -0.53, flags, _lib.ptr(out), _lib.ptr(scratch),
                                 _lib.stream_handle(pos.device))


def test_entry_guards():
    lib = _lib.load()
    p, t = _positions("sphere")
    ref = S.adjacency("sphere")
    dp, off, nb = _dev(p), _dev(ref.offsets), _dev(ref.neighbors)
    out, scratch = torch.empty_like(dp), torch.empty_like(dp)
    assert _smooth_raw(dp, off, nb, dp, scratch) == -1 and b"overlap" in lib.anerf_last_error()
    assert _smooth_raw(dp, off, nb, out, out, iterations=2) == -1 and b"overlap" in lib.anerf_last_error()
    # a short workspace
    dt = _dev(t)
    nv, nt = len(p), len(t)
    need = lib.anerf_mesh_adjacency_workspace(nv, nt)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    offsets = torch.empty(nv + 1, device="cuda", dtype=torch.int32)
    boundary = torch.empty(nv, device="cuda", dtype=torch.uint8)
    totals = torch.empty(2, device="cuda", dtype=torch.int64)
    stream = _lib.stream_handle(dt.device)
    assert lib.anerf_mesh_adjacency_count(_lib.ptr(dt), nt, nv, _lib.ptr(ws), need - 4, _lib.ptr(offsets),
                                          _lib.ptr(boundary), _lib.ptr(totals), stream) == -1
    assert b"anerf_mesh_adjacency_workspace" in lib.anerf_last_error()
    # the totals: E and the largest distinct degree; an emit capacity below E stores nothing past it
    _lib.check(lib.anerf_mesh_adjacency_count(_lib.ptr(dt), nt, nv, _lib.ptr(ws), need, _lib.ptr(offsets),
                                              _lib.ptr(boundary), _lib.ptr(totals), stream), "count")
    assert totals.tolist() == [len(ref.neighbors), int(np.diff(ref.offsets).max())]
    cap = len(ref.neighbors) - 100
    buf = torch.full((len(ref.neighbors),), -7, device="cuda", dtype=torch.int32)
    _lib.check(lib.anerf_mesh_adjacency_emit(nv, _lib.ptr(ws), need, _lib.ptr(offsets), _lib.ptr(buf), cap, stream),
               "emit")
    np.testing.assert_array_equal(buf[:cap].cpu().numpy(), ref.neighbors[:cap])
    assert (buf[cap:] == -7).all()


def test_a_bad_csr_is_ignored_not_followed():
    """Neighbour ids outside [0, V) are skipped and not counted; a row bound beyond E is clamped."""
    p, t = _positions("sphere")
    ref = S.adjacency("sphere")
    nv, ne = len(p), len(ref.neighbors)
    rng = np.random.default_rng(3)
    bad = rng.choice(ne, 200, replace=False)
    nb = ref.neighbors.copy()
    nb[bad[:100]] = nv + rng.integers(0, 1 << 20, 100)
    nb[bad[100:]] = -1 - rng.integers(0, 1 << 20, 100)
    ok = np.ones(ne, bool)
    ok[bad] = False
    row = np.repeat(np.arange(nv), np.diff(ref.offsets))
    clean_off = np.concatenate([[0], np.cumsum(np.bincount(row[ok], minlength=nv))]).astype(np.int32)
    clean = meshops.VertexAdjacency(clean_off, ref.neighbors[ok], ref.boundary)
    want = meshops.smooth_mesh_reference(p, t, iterations=3, pin=None, adjacency=clean)
    off = ref.offsets.copy()
    off[-1] = ne + 12345
    dp = _dev(p)
    out, scratch = torch.empty_like(dp), torch.empty_like(dp)
    assert _smooth_raw(dp, _dev(off), _dev(nb), out, scratch, iterations=3, flags=_lib.ANERF_SMOOTH_TAUBIN) == 0
    torch.cuda.synchronize()
    _assert_bits(out, want, "bad CSR")


# ------------------------------------------------------------------ integration
THR = 0.3  # (test_gpu_isosurface.py: no grid value of dm_fine_d8w256 is near it)


def _pose(g):
    return torch.from_numpy(g["kps"]), torch.from_numpy(g["skts"]), torch.from_numpy(g["bones"])


def test_extract_mesh_smooths_after_the_filter_and_before_the_colours():
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    kw = dict(radius=radius, res=res, threshold=THR, keep_largest=1)
    vi, ti = rc.extract_mesh(kps, skts, bones, coords="index", **kw)
    assert len(ti) > 0
    ref = torch.from_numpy(meshops.smooth_mesh_reference(vi, ti, iterations=5)).cuda()
    assert not torch.equal(ref, vi)
    kp0 = kps.to(ref.device, torch.float32).reshape(-1, 3)[0]
    world = (-radius + (2.0 * radius / res) * ref[:, [1, 0, 2]]) + kp0
    mapped = {"index": ref, "unit": ref / res - .5, "world": world}
    # the colours: the field at the SMOOTHED world vertices, each seen against its (unsmoothed) world normal
    inward = 0.0 - rc.extract_mesh(kps, skts, bones, coords="world", normals=True, **kw)[2]["normals"]
    dirs = torch.where((inward == 0).all(-1, keepdim=True), kp0 - world, inward).contiguous()
    raw = rc.render_pts_radiance(world.contiguous(), dirs, kps, skts, bones)
    colors = torch.sigmoid(raw[:, :3].to(torch.float32))
    for coords in ("index", "unit", "world"):
        pv, pt, pa = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, **kw)
        v, t, a = rc.extract_mesh(kps, skts, bones, coords=coords, normals=True, colors=True, smooth=5, **kw)
        assert torch.equal(t, pt) and torch.equal(a["normals"], pa["normals"])
        assert torch.equal(v.view(torch.int32), mapped[coords].view(torch.int32)), coords
        assert torch.equal(a["colors"], colors), coords
    # smooth=0 is today's call; the other two arguments reach smooth_mesh
    v0, t0 = rc.extract_mesh(kps, skts, bones, coords="index", smooth=0, **kw)
    assert torch.equal(v0, vi) and torch.equal(t0, ti)
    vl, _ = rc.extract_mesh(kps, skts, bones, coords="index", smooth=2, smooth_lambda=0.3, smooth_mu=None, **kw)
    _assert_bits(vl, meshops.smooth_mesh_reference(vi, ti, iterations=2, lam=0.3, mu=None), "smooth_lambda / smooth_mu")


def test_staged_caster_forwards_smooth():
    g = Golden("sgd1_relpos_mrb2_density")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    kw = dict(radius=radius, res=res, threshold=2.0, coords="index", keep_largest=1)
    for caster in (rc._staged.eval_caster(), rc):
        pv, pt = caster.extract_mesh(kps, skts, bones, **kw)
        v, t = caster.extract_mesh(kps, skts, bones, smooth=3, **kw)
        assert len(pt) > 0 and torch.equal(t, pt)
        _assert_bits(v, meshops.smooth_mesh_reference(pv, pt, iterations=3), "staged caster")


def test_render_mesh_writes_the_smoothed_mesh(tmp_path):
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    data = {"kp": kps, "skts": skts, "bones": bones}
    rk = {"ray_caster": rc, "preproc_kwargs": {}}
    kw = dict(radius=radius, res=res, threshold=THR, normals=True, keep_largest=1)
    out = anerf.render_mesh(str(tmp_path / "s"), rk, data, smooth=5, **kw)
    v, t, a = out[0]
    ev, et, ea = rc.extract_mesh(kps, skts, bones, smooth=5, **kw)
    assert len(t) > 0 and torch.equal(v, ev) and torch.equal(t, et) and torch.equal(a["normals"], ea["normals"])
    rv, rt, ra = iso.read_ply(str(tmp_path / "s" / "meshes" / "000.ply"), attributes=True)
    np.testing.assert_array_equal(rv.view(np.int32), v.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(rt, t.cpu().numpy())
    np.testing.assert_array_equal(ra["normals"], a["normals"].cpu().numpy())
    # smooth=0: the file of the call without the argument, byte for byte
    anerf.render_mesh(str(tmp_path / "a"), rk, data, smooth=0, **kw)
    plain = anerf.render_mesh(str(tmp_path / "b"), rk, data, **kw)
    assert (tmp_path / "a" / "meshes" / "000.ply").read_bytes() == (tmp_path / "b" / "meshes" / "000.ply").read_bytes()
    assert not torch.equal(plain[0][0], v) and torch.equal(plain[0][1], t)

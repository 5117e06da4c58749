"""GPU: the iso-surface kernels (csrc/anerf_iso.hip through isosurface.isosurface) against the NumPy reference of
the same contract (isosurface.isosurface_reference, itself held to mesh properties in test_isosurface.py), and the
mesh path end to end on the reference's own density grids (tests/golden/dm_fine_d8w256, sgd1_relpos_mrb2_density).

Parity: triangles identical, vertices in the same order and within 1 ulp per coordinate (the build has
-ffp-contract=off and fp32 division is correctly rounded, so they are expected to be bit-identical; `_assert_same`
reports the count of coordinates that are not)."""
import importlib

import numpy as np
import pytest
import torch

import _iso_cases as C
from _golden import Golden

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
iso = importlib.import_module("a-nerf_amd.isosurface")
train = importlib.import_module("a-nerf_amd.train")


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ulp_distance(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)  # (sign-magnitude -> ordered integers)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def _assert_same(got, ref, what=""):
    """Device result against the reference: same triangles, same vertex order, vertices within 1 ulp."""
    v, t = got[0].cpu().numpy(), got[1].cpu().numpy()
    rv, rt = ref
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert v.shape == rv.shape and t.shape == rt.shape, (what, v.shape, rv.shape, t.shape, rt.shape)
    np.testing.assert_array_equal(t, rt, err_msg=what)
    if v.size:
        d = _ulp_distance(v, rv)
        print(f"{what}: V {len(v)} T {len(t)} coordinates not bit-identical: {int((d > 0).sum())}, max {int(d.max())} ulp")
        assert int(d.max()) <= 1, what
    return v, t


CASES = {
    "random9_s0": (("random_field", 0), 0.5, False),
    "random9_s1": (("random_field", 1), 0.5, False),
    "random9_s2": (("random_field", 2), 0.5, False),
    "random_5x9x13": (("random_field", 3, (5, 9, 13), False), 0.5, False),  # (axis order; cut by the boundary)
    "sphere16": (("sphere_field",), 0.0, False),
    "blobs_67x61x71": (("blobs_field",), 0.5, False),  # (ragged, many workgroups, two scan tiles)
    "last_rows": (("last_rows_field",), 0.0, False),
    "relu": (("relu_field",), 0.25, True),
    "nan": (("nan_field",), 0.0, False),
    "nan_relu": (("nan_field",), 1.0, True),  # (the clamp keeps a NaN a NaN, as np.maximum)
}


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_reference(name):
    (fn, *args), thr, relu = CASES[name]
    field = getattr(C, fn)(*args)
    ref = C.reference(fn, *args, threshold=thr, relu=relu)
    assert len(ref[1]) > 0
    v, _ = _assert_same(iso.isosurface(field, thr, relu=relu), ref, name)
    assert np.isfinite(v).all()


@pytest.mark.parametrize("corner", [False, True], ids=["ball_3_in", "ball_in_the_corner"])
@pytest.mark.parametrize("shape", C.TILE_EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_the_reference_at_the_scan_tile_edges(shape, corner):
    """1024 and 1025 points, and 262143, 262144, 262145: one tile + 1, and one round of the block-sum scan -1, +0, +1
    (at 257 workgroups its carry starts: the totals come through it).  Positions and normals bit for bit.  With the
    ball in the corner the point (n0 - 1, n1 - 1, n2 - 3) owns the last vertex: the base of the last tile with edges."""
    points = int(np.prod(shape))
    assert points in (1024, 1025, 262143, 262144, 262145)
    rv, rt, rn = C.tile_edge_reference(shape, corner)
    assert len(rt) > 0
    if corner:
        owner = np.floor(rv).astype(np.int64) @ np.array([shape[1] * shape[2], shape[2], 1])
        assert int(owner.max()) == points - 3
    v, t, n = iso.isosurface(C.tile_edge_field(shape, corner), 0.0, normals=True)
    np.testing.assert_array_equal(t.cpu().numpy(), rt)
    for name, got, ref in (("positions", v, rv), ("normals", n, rn)):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.shape, ref.shape)
        diff = int((got.view(np.int32) != ref.view(np.int32)).sum())
        print(f"{shape} {name}: {diff} differing words of {ref.size}")
        assert diff == 0, name


def test_flip_reverses_the_winding():
    v, t = iso.isosurface(C.sphere_field(), 0.0, flip=True)
    _assert_same((v, t), C.reference("sphere_field", flip=True), "flip")
    assert C.signed_volume(v.cpu().numpy(), t.cpu().numpy()) < 0


def test_relu_differs_from_no_relu():
    f = torch.from_numpy(C.relu_field().copy()).cuda()
    v1, t1 = iso.isosurface(f, 0.25, relu=True)
    v0, t0 = iso.isosurface(f, 0.25, relu=False)
    _assert_same((v0, t0), C.reference("relu_field", threshold=0.25), "no relu")
    ref = iso.isosurface_reference(np.maximum(C.relu_field(), 0), 0.25)
    _assert_same((v1, t1), ref, "relu vs np.maximum")
    assert torch.equal(t0, t1) and float((v1 - v0).abs().max()) > 0.05


def test_empty_results():
    f = C.random_field(0)
    for thr in (-1.0, 2.0):
        v, t = iso.isosurface(f, thr)
        assert v.is_cuda and tuple(v.shape) == (0, 3) and v.dtype == torch.float32
        assert t.is_cuda and tuple(t.shape) == (0, 3) and t.dtype == torch.int32
    for shape in ((1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1)):
        v, t = iso.isosurface(np.random.default_rng(1).random(shape), 0.5)
        assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3)
    one = np.zeros((3, 3, 3), np.float32)
    one[1, 1, 1] = 1.0
    v, t = iso.isosurface(one, 0.25)
    assert (len(v), len(t)) == (6, 8)
    _assert_same((v, t), iso.isosurface_reference(one, 0.25), "octahedron")


def test_deterministic_and_stream_independent():
    f = torch.from_numpy(C.blobs_field().copy()).cuda()
    v0, t0 = iso.isosurface(f, 0.5)
    v1, t1 = iso.isosurface(f, 0.5)
    assert torch.equal(v0, v1) and torch.equal(t0, t1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        v2, t2 = iso.isosurface(f, 0.5)
    s.synchronize()
    assert torch.equal(v0, v2) and torch.equal(t0, t2)


# ------------------------------------------------------------------ end to end on the reference's grids
THR = 0.3  # dm_fine_d8w256: the nearest grid value is 9.2e-4 away (9 x the grid's 1e-4 parity bound): no case flips


def _pose(g):
    return torch.from_numpy(g["kps"]), torch.from_numpy(g["skts"]), torch.from_numpy(g["bones"])


def test_extract_mesh_on_the_reference_grid():
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    assert res == 16
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    v, t = rc.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=THR, coords="index")
    own = rc(kps=kps, skts=skts, bones=bones, radius=radius, res=res, render_kwargs={}, fwd_type="mesh")
    ref_own = iso.isosurface_reference(own.cpu().numpy(), THR, relu=True)
    np.testing.assert_array_equal(t.cpu().numpy(), ref_own[1])
    np.testing.assert_array_equal(v.cpu().numpy(), ref_own[0])
    # the reference's own grid: the same triangles, vertices within 0.02 grid units (a 1e-4 grid error over the
    # smallest value step across a crossing edge, 0.0271, moves a vertex by <= 0.011; without the relu: 0.099)
    rv, rt = iso.isosurface_reference(g["grid_density"], THR, relu=True)
    assert (len(rv), len(rt)) == (226, 416) and not C.directed_edge_imbalance(rt)
    np.testing.assert_array_equal(t.cpu().numpy(), rt)
    assert v.shape == rv.shape
    d = float(np.abs(v.cpu().numpy() - rv).max())
    print(f"extract_mesh vs the reference grid's mesh: max vertex distance {d:.4f} grid units")
    assert d <= 0.02
    # coordinates
    vu, tu = rc.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=THR)  # coords="unit"
    assert torch.equal(tu, t) and torch.equal(vu, v / 16 - .5)
    vw, tw = rc.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=THR, coords="world")
    assert torch.equal(tw, t[:, [0, 2, 1]])
    assert C.signed_volume(vw.cpu().numpy(), tw.cpu().numpy()) > 0
    assert C.signed_volume(v.cpu().numpy(), t.cpu().numpy()) > 0
    kp0 = g["kps"][0, 0].astype(np.float64)
    back = ((vw.cpu().numpy().astype(np.float64) - kp0 + radius) * res / (2 * radius))[:, [1, 0, 2]]
    assert float(np.abs(back - v.cpu().numpy()).max()) <= 1e-4
    vf, tf = rc.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=THR, coords="index", flip=True)
    assert torch.equal(vf, v) and torch.equal(tf, tw)
    with pytest.raises(ValueError, match="coords"):
        rc.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=THR, coords="metres")


@pytest.mark.parametrize("thr", [0.3, 2.0])
def test_staged_caster_extract_mesh(thr):
    """The staged fixture's densities lie in [1.6, 2.7]: the reference's threshold gives an empty mesh, 2.0 a surface."""
    g = Golden("sgd1_relpos_mrb2_density")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    sc = rc._staged.eval_caster()
    assert isinstance(sc, train.StagedCaster)
    kps, skts, bones = _pose(g)
    own = sc.render_mesh_density(kps, skts, bones, radius=radius, res=res)
    ref = iso.isosurface_reference(own.cpu().numpy(), thr, relu=True)
    assert (len(ref[1]) > 0) == (thr == 2.0)
    for caster in (sc, rc):
        v, t = caster.extract_mesh(kps, skts, bones, radius=radius, res=res, threshold=thr, coords="index")
        assert v.is_cuda and t.is_cuda
        np.testing.assert_array_equal(t.cpu().numpy(), ref[1])
        np.testing.assert_array_equal(v.cpu().numpy(), ref[0])


def test_render_mesh_writes_one_ply_per_pose(tmp_path):
    g = Golden("dm_fine_d8w256")
    res, radius = g.meta["res"], g.meta["radius"]
    rc = anerf.RayCaster(g.cfg, g.ckpt)
    kps, skts, bones = _pose(g)
    data = {"kp": torch.cat([kps, kps + 0.04]), "skts": torch.cat([skts, skts]), "bones": torch.cat([bones, bones])}
    out = anerf.render_mesh(str(tmp_path), {"ray_caster": rc, "preproc_kwargs": {}}, data, radius=radius, res=res,
                            threshold=THR)
    assert len(out) == 2 and sorted(p.name for p in (tmp_path / "meshes").iterdir()) == ["000.ply", "001.ply"]
    for i, (v, t) in enumerate(out):
        ev, et = rc.extract_mesh(data["kp"][i:i + 1], data["skts"][i:i + 1], data["bones"][i:i + 1], radius=radius,
                                 res=res, threshold=THR)
        assert torch.equal(v, ev) and torch.equal(t, et) and len(t) > 0
        pv, pt = iso.read_ply(str(tmp_path / "meshes" / f"{i:03d}.ply"))
        np.testing.assert_array_equal(pv, ev.cpu().numpy())
        np.testing.assert_array_equal(pt, et.cpu().numpy())

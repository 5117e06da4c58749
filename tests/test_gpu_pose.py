"""Pose scoring on the GPU (csrc/anerf_posescore.hip, a-nerf_amd/posescore.py) against the float64 checker.

Bounds, for a pose of extent |X0| (the centred Frobenius norm of gt).  The scores, d, b, the singular values and c:
1e-12 x extent: both sides are double, the sums run over at most 128 joints (128 x 1.1e-16 = 1.4e-14).  T, err, pa_err:
1e-9 x extent, and Z, which the kernel rounds once to fp32, half an fp32 ulp of the checker's value plus 1e-9 x extent,
on the well-conditioned frames (sigma3 / sigma1 >= 1e-3, asserted for every frame of the generic cases): the singular
vectors carry eps sigma1 / sigma3 <= 1.1e-13 over a few dozen operations.  On the rank-deficient frames (J = 2, J = 3,
flat poses) T, Z and c hang on the completion and only the scores are compared.  Counts are compared exactly.

J in {1, 2, 3, 17, 24, 64, 65, 128}: a frame without a fit, rank 1, rank 2, a partial wave, a full wave, a second pass
and the limit; F in {1, 3, 5, 257}: fewer frames than the four waves of a workgroup, a count that is no multiple of it,
and nine slots of the total kernel (32 frames each), the last one ragged."""
import importlib
import os

import numpy as np
import pytest
import torch

import _pose_cases as cases

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
ps = importlib.import_module("a-nerf_amd.posescore")
kin = importlib.import_module("a-nerf_amd.kinematics")
syn = importlib.import_module("a-nerf_amd.synthetic")

HERE = os.path.dirname(os.path.abspath(__file__))
TOL, TOL_Z = 1e-12, 1e-9
ALL = dict(per_frame=True, return_aligned=True, return_errors=True)
SCORES = slice(0, 10)  # n, the four scores, d, b, the singular values
MAXIMA = {}            # the largest error seen per quantity, over extent (DESIGN 9j quotes them)


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    print("\nlargest error over its bound, per quantity:", {k: float(f"{v:.3g}") for k, v in sorted(MAXIMA.items())})


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "pose_scores.npz")))


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def extent(gt, on=None):
    """Per frame the centred Frobenius norm of the scored gt joints; where that is zero by the kernel's rule (one
    joint, all joints equal: only mpjpe is left to compare) the uncentred norm."""
    gt = np.asarray(gt, np.float64)
    on = np.ones(gt.shape[:2], bool) if on is None else on
    n = np.maximum(on.sum(1), 1)[:, None, None]
    mu = np.where(on[..., None], gt, 0).sum(1, keepdims=True) / n
    ss = (np.where(on[..., None], gt - mu, 0) ** 2).sum((1, 2))
    raw = (np.where(on[..., None], gt, 0) ** 2).sum((1, 2))
    return np.sqrt(np.where(ss > ps.ZERO_SS * raw, ss, raw))


def same(got, want, tol, what, extra=0.0):
    """|got - want| <= tol (per frame along axis 0, + extra per element) with the same NaNs on both sides."""
    got, want = _np(got).astype(np.float64), _np(want).astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: the NaNs differ"
    if got.size == 0:
        return
    tol = np.asarray(tol, np.float64)
    if tol.ndim:
        tol = tol.reshape((-1,) + (1,) * (got.ndim - 1))
    bound = tol + extra
    err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
    scale = np.broadcast_to(np.where(bound > 0, bound, 1.0), err.shape)
    key = what.split(":")[-1].strip()
    MAXIMA[key] = max(MAXIMA.get(key, 0.0), float((err / scale).max()))
    assert np.all(err <= bound), f"{what}: {float((err / scale).max()):.3g} x the bound ({err.max():.3g})"


def compare(got, want, gt, where, on=None, generic=None):
    """A device result against the checker's: the scores everywhere, T / Z / c on the frames `generic`."""
    ext = extent(gt, on)
    rec, wrec = _np(got.per_frame), want.per_frame
    same(rec[:, SCORES], wrec[:, SCORES], TOL * ext, f"{where}: scores")
    same(rec[:, 22:25], wrec[:, 22:25], TOL * np.maximum(ext, 1.0), f"{where}: norms")
    same(got.err, want.err, TOL_Z * ext, f"{where}: err")
    same(got.pa_err, want.pa_err, TOL_Z * ext, f"{where}: pa_err")
    fit = ~np.isnan(wrec[:, ps.COL["pa_mpjpe"]])
    assert np.array_equal(np.isnan(rec[:, 10:22]), np.isnan(wrec[:, 10:22])), f"{where}: the NaNs of T and c differ"
    assert np.array_equal(np.isnan(_np(got.aligned)), np.isnan(want.aligned)), f"{where}: the NaNs of Z differ"
    if fit.any():
        T = rec[fit, 10:19].reshape(-1, 3, 3)
        assert np.abs(T @ T.transpose(0, 2, 1) - np.eye(3)).max() < 1e-13, f"{where}: T is not orthogonal"
    g = fit if generic is None else generic
    if generic is not None and g.any():
        s = wrec[g, 7:10]
        assert np.all(np.abs(s[:, 2]) / s[:, 0] >= 1e-3), f"{where}: not every generic frame is well conditioned"
        same(rec[g, 19:22], wrec[g, 19:22], TOL * ext[g], f"{where}: c")
        same(rec[g, 10:19], wrec[g, 10:19], TOL_Z, f"{where}: T")
        same(_np(got.aligned)[g], want.aligned[g], TOL_Z * ext[g], f"{where}: Z",
             extra=np.abs(want.aligned[g]) * 2.0 ** -24)
    # the totals
    assert (got.n_frames, got.n_scored, got.n_pairs) == (want.n_frames, want.n_scored, want.n_pairs), where
    assert np.array_equal(got.pck_counts, want.pck_counts), f"{where}: threshold counts"
    big = float(ext.max()) if len(ext) else 1.0
    for k in ("mpjpe", "mpjpe_root", "n_mpjpe", "pa_mpjpe"):
        same(np.float64(getattr(got, k)), np.float64(getattr(want, k)), TOL * big, f"{where}: mean {k}")
    same(got.per_joint_mpjpe, want.per_joint_mpjpe, TOL_Z * big, f"{where}: per-joint err")
    same(got.per_joint_pa_mpjpe, want.per_joint_pa_mpjpe, TOL_Z * big, f"{where}: per-joint pa_err")
    assert got.pck == pytest.approx(want.pck, abs=0, nan_ok=True), where  # (a ratio of equal integers)
    assert got.auc == pytest.approx(want.auc, rel=1e-14, nan_ok=True), where


@pytest.mark.parametrize("F", [1, 3, 5, 257])
@pytest.mark.parametrize("J", [1, 2, 3, 17, 24, 64, 65, 128])
def test_gpu_scores_against_the_checker(J, F):
    pred, gt = cases.make_pair("body", F, J, 1000 + 7 * J + F)
    kw = dict(root=J // 2, pck_threshold=60.0)
    want = ps.evaluate_poses_reference(pred, gt, **kw, **ALL)
    got = anerf.evaluate_poses(pred, gt, **kw, **ALL)
    compare(got, want, gt, f"J={J} F={F}", generic=np.ones(F, bool) if J >= 17 else None)
    assert got.per_frame.is_cuda and got.aligned.dtype == torch.float32 and tuple(got.aligned.shape) == (F, J, 3)
    if J == 1:
        assert got.n_scored == 0 and np.isnan(got.pa_mpjpe) and np.all(np.isfinite(_np(got.column("mpjpe"))))


def test_gpu_no_frames():
    r = anerf.evaluate_poses(np.zeros((0, 24, 3), np.float32), np.zeros((0, 24, 3), np.float32), **ALL)
    assert (r.n_frames, r.n_scored, r.n_pairs) == (0, 0, 0) and np.isnan(r.pa_mpjpe) and np.isnan(r.mpjpe)
    assert tuple(r.per_frame.shape) == (0, 25) and tuple(r.aligned.shape) == (0, 24, 3)
    assert tuple(r.err.shape) == tuple(r.pa_err.shape) == (0, 24) and len(r.pck_curve) == 31


@pytest.mark.parametrize("scaling", [True, False])
def test_gpu_exact_similarity_is_recovered(scaling):
    """pred with gt = b pred T + c exactly (float64 inputs): the fit returns b, T and c and leaves no error."""
    rs = np.random.default_rng(5)
    gt = cases.body(rs, 6, 24)
    pred, b, T, c = cases.transformed(rs, gt)
    if not scaling:
        pred, b = pred * b[:, None, None], np.ones(6)
    ext = extent(gt)
    r = anerf.evaluate_poses(pred, gt, scaling=scaling, reflection=False, **ALL)
    same(r.column("pa_mpjpe"), np.zeros(6), TOL * ext, "exact: pa_mpjpe")
    same(r.column("d"), np.zeros(6), TOL, "exact: d")
    same(r.column("b"), b, TOL * b, "exact: b")
    same(r.column("T"), T, TOL_Z, "exact: T")
    same(r.column("c"), c, TOL_Z * ext, "exact: c")
    assert r.pa_mpjpe <= TOL * ext.max() and np.all(_np(r.pa_err) <= TOL_Z * ext[:, None])


@pytest.mark.parametrize("kind", ["mirrored", "exact"])
def test_gpu_reflection_modes(kind):
    """A mirrored pred: under 'best' det T = -1 and the error is near zero; under False det T = +1 and the checker's
    larger error is matched; True forces det T = -1 on a pred that is not mirrored."""
    rs = np.random.default_rng(11)
    gt = cases.body(rs, 4, 24)
    pred = cases.transformed(rs, gt, mirror=kind == "mirrored")[0]
    ext = extent(gt)
    for reflection in ("best", False, True):
        got = anerf.evaluate_poses(pred, gt, reflection=reflection, **ALL)
        want = ps.evaluate_poses_reference(pred, gt, reflection=reflection, **ALL)
        compare(got, want, gt, f"{kind} reflection={reflection}", generic=np.ones(4, bool))
        det = np.linalg.det(_np(got.column("T")))
        natural = -1.0 if kind == "mirrored" else 1.0
        forced = natural if reflection == "best" else (-1.0 if reflection else 1.0)
        assert np.allclose(det, forced, atol=1e-12), (kind, reflection, det)
        if forced == natural:
            assert got.pa_mpjpe <= TOL * ext.max()
        else:
            assert got.pa_mpjpe > 1e-3 * ext.min()


@pytest.mark.parametrize("kind,J", [("planar_gt", 24), ("collinear_gt", 8), ("both_planar", 12), ("planar_exact", 9),
                                    ("equal", 5)])
def test_gpu_degenerate_poses(kind, J):
    pred, gt = cases.make_pair(kind, 5, J, 77)
    for scaling, reflection in cases.COMBOS:
        kw = dict(scaling=scaling, reflection=reflection)
        got = anerf.evaluate_poses(pred, gt, **kw, **ALL)
        want = ps.evaluate_poses_reference(pred, gt, **kw, **ALL)
        compare(got, want, gt, f"{kind} {kw}")
        if kind == "equal":
            assert got.n_scored == 0 and np.all(np.isnan(_np(got.aligned)))
        else:
            det = np.linalg.det(_np(got.column("T")))
            assert np.allclose(det, -1.0 if reflection is True else 1.0, atol=1e-12), (kind, kw, det)
    if kind == "planar_exact":  # a rotation, not a projection: Z keeps pred's shape up to the scale b
        got = anerf.evaluate_poses(pred, gt, **ALL)
        y0 = pred - pred.mean(1, keepdims=True)
        z = _np(got.aligned).astype(np.float64)
        z0 = z - z.mean(1, keepdims=True)
        np.testing.assert_allclose(np.linalg.norm(z0, axis=-1), _np(got.column("b"))[:, None] * np.linalg.norm(y0, axis=-1),
                                   atol=1e-4)


def test_gpu_valid_masks_and_joint_subsets():
    pred, gt = cases.make_pair("body", 7, 17, 31)
    valid = np.ones((7, 17), np.uint8)
    valid[1] = 0                 # no joint
    valid[2, :16] = 0            # one joint
    valid[3, 2:] = 0             # two joints
    valid[4, 14] = 0             # the root is missing
    valid[5, [0, 3, 9]] = 0
    for joints in (None, cases.SUBSET_14, [16, 2, 14, 7, 0]):
        sel = np.zeros(17, bool)
        sel[list(range(17)) if joints is None else joints] = True
        on = (valid != 0) & sel[None]
        kw = dict(joints=joints, valid=valid, root=14)
        got = anerf.evaluate_poses(pred, gt, **kw, **ALL)
        want = ps.evaluate_poses_reference(pred, gt, **kw, **ALL)
        generic = on.sum(1) >= 10
        compare(got, want, gt, f"joints={joints}", on=on, generic=generic)
        assert np.array_equal(_np(got.column("n")), on.sum(1))
        assert np.all(_np(got.err)[~on] == 0) and np.all(_np(got.pa_err)[~on] == 0)
    # the subset equals the sliced arrays (sums in another order: the scores' bound)
    sub = cases.SUBSET_14
    a = anerf.evaluate_poses(pred, gt, joints=sub, root=14, **ALL)
    b = anerf.evaluate_poses(pred[:, sub], gt[:, sub], root=sub.index(14), **ALL)
    same(a.per_frame[:, SCORES], b.per_frame[:, SCORES], TOL * extent(gt[:, sub]), "subset against slices: scores")
    same(a.per_joint_pa_mpjpe, b.per_joint_pa_mpjpe, TOL_Z * extent(gt).max(), "subset against slices: per-joint pa_err")
    assert np.array_equal(a.pck_counts, b.pck_counts)
    valid_t = torch.from_numpy(valid).cuda()
    c = anerf.evaluate_poses(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), valid=valid_t, root=14, **ALL)
    d = anerf.evaluate_poses(pred, gt, valid=valid, root=14, **ALL)
    assert torch.equal(c.per_frame.nan_to_num(7.0), d.per_frame.nan_to_num(7.0)), "device and host inputs"


@pytest.mark.parametrize("pred_dtype,gt_dtype", [(np.float32, np.float32), (np.float64, np.float32),
                                                 (np.float32, np.float64), (np.float64, np.float64)])
def test_gpu_input_precisions_and_units(pred_dtype, gt_dtype):
    """fp32 and fp64 inputs widen exactly; pred in metres x 1000 against gt in millimetres x 1."""
    rs = np.random.default_rng(3)
    gt = cases.body(rs, 5, 24).astype(gt_dtype)
    pred = cases.transformed(rs, gt.astype(np.float64), noise=30.0, unit=1000.0)[0].astype(pred_dtype)
    kw = dict(pred_scale=1000.0, gt_scale=1.0, root=0)
    got = anerf.evaluate_poses(pred, gt, **kw, **ALL)
    want = ps.evaluate_poses_reference(pred, gt, **kw, **ALL)
    compare(got, want, gt.astype(np.float64), f"{pred_dtype.__name__} {gt_dtype.__name__}", generic=np.ones(5, bool))
    assert 5.0 < got.pa_mpjpe < 200.0
    metres = anerf.evaluate_poses(pred, gt, pred_scale=1.0, gt_scale=0.001, root=0, thresholds=ps.AUC_THRESHOLDS / 1000,
                                  pck_threshold=0.15, **ALL)
    same(metres.column("pa_mpjpe") * 1000, got.column("pa_mpjpe"), TOL * extent(gt), "metres against millimetres")


def test_gpu_runs_are_bit_identical_and_frames_independent():
    pred, gt = cases.make_pair("body", 37, 65, 55)
    valid = (np.random.default_rng(1).uniform(size=(37, 65)) > 0.2).astype(np.uint8)
    kw = dict(valid=valid, root=3, joints=list(range(1, 65)))
    a = anerf.evaluate_poses(pred, gt, **kw, **ALL)
    b = anerf.evaluate_poses(pred, gt, **kw, **ALL)
    for name in ("per_frame", "aligned", "err", "pa_err"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.view(torch.int64 if x.dtype == torch.float64 else torch.int32),
                           y.view(torch.int64 if y.dtype == torch.float64 else torch.int32)), name
    for name in ("mpjpe", "mpjpe_root", "n_mpjpe", "pa_mpjpe", "pck", "auc"):
        assert getattr(a, name) == getattr(b, name), name
    assert np.array_equal(a.per_joint_pa_mpjpe, b.per_joint_pa_mpjpe) and np.array_equal(a.pck_counts, b.pck_counts)
    # the records of frames scored together are those of the same frames scored one at a time
    for f in (0, 3, 4, 31, 32, 36):
        one = anerf.evaluate_poses(pred[f:f + 1], gt[f:f + 1], valid=valid[f:f + 1], root=3, joints=kw["joints"], **ALL)
        for name in ("per_frame", "aligned", "err", "pa_err"):
            x, y = getattr(one, name)[0], getattr(a, name)[f]
            assert torch.equal(x.nan_to_num(7.0), y.nan_to_num(7.0)) and torch.equal(x.isnan(), y.isnan()), (f, name)


def _layer(n=5, seed=4):
    rs = np.random.RandomState(seed)
    bones = (0.4 * rs.normal(size=(n, 24, 3))).astype(np.float32)
    kps = (rs.normal(scale=0.5, size=(n, 24, 3)) + np.array([0.3, -0.2, 0.1])).astype(np.float32)
    return kin.PoseOptLayer(kps, bones, syn.REST_POSE_24.astype(np.float32)[None]), rs


def test_gpu_evaluate_pose_layer_and_trainer_method():
    layer, rs = _layer()
    with torch.no_grad():
        kps = layer(np.arange(5))[0]
    gt = (_np(kps).astype(np.float64) * 1000 + rs.normal(scale=25.0, size=(5, 24, 3))).astype(np.float32)
    kw = dict(pred_scale=1000.0, root=0, joints=list(range(17)))
    got = anerf.evaluate_pose_layer(layer, gt, **kw, **ALL)
    want = anerf.evaluate_poses(_np(kps), gt, **kw, **ALL)
    assert torch.equal(got.per_frame, want.per_frame) and got.pa_mpjpe == want.pa_mpjpe and got.pck == want.pck
    assert 1.0 < got.pa_mpjpe < 100.0
    some = anerf.evaluate_pose_layer(layer, torch.from_numpy(gt).cuda(), idxs=[4, 1], **kw, **ALL)
    assert torch.equal(some.per_frame, want.per_frame[[4, 1]])
    stub = anerf.Trainer.__new__(anerf.Trainer)  # (the method reads popt_kwargs alone)
    stub.popt_kwargs = {"popt_layer": layer}
    assert anerf.Trainer.evaluate_poses(stub, gt, **kw).pa_mpjpe == got.pa_mpjpe
    stub.popt_kwargs = None
    with pytest.raises(ValueError):
        anerf.Trainer.evaluate_poses(stub, gt)


def test_gpu_evaluate_pose_ckpt_round_trip(tmp_path):
    layer, rs = _layer()
    with torch.no_grad():
        refined = _np(layer(np.arange(5))[0]).astype(np.float64)
    gt = (refined + rs.normal(scale=0.01, size=refined.shape)).astype(np.float32)
    init = (refined + rs.normal(scale=0.05, size=refined.shape)).astype(np.float32)
    path = str(tmp_path / "popt.tar")
    stub = anerf.Trainer.__new__(anerf.Trainer)  # (save_popt reads popt_kwargs alone)
    stub.popt_kwargs = {"popt_layer": layer, "popt_anchors": None}
    anerf.Trainer.save_popt(stub, path, 3)
    kw = dict(pred_scale=1000.0, gt_scale=1000.0)
    out = anerf.evaluate_pose_ckpt(path, gt_kps=gt, init_kps=init, **kw)
    want = anerf.evaluate_poses(refined.astype(np.float32), gt, **kw)
    assert out["refined"].pa_mpjpe == want.pa_mpjpe and out["refined"].mpjpe == want.mpjpe
    assert out["init"].pa_mpjpe == anerf.evaluate_poses(init, gt, **kw).pa_mpjpe
    assert out["delta_pa_mpjpe"] == out["refined"].pa_mpjpe - out["init"].pa_mpjpe < 0
    assert out["delta_mpjpe"] == out["refined"].mpjpe - out["init"].mpjpe < 0
    alone = anerf.evaluate_pose_ckpt(popt_sd={k: v.detach().cpu() for k, v in layer.state_dict().items()}, gt_kps=gt, **kw)
    assert alone["init"] is None and alone["delta_pa_mpjpe"] is None and alone["refined"].pa_mpjpe == want.pa_mpjpe


@pytest.mark.parametrize("name", ["body24", "mirrored", "j2", "planar_gt"])
def test_gpu_drop_in_modules(golden, name):
    """The reference's modules over the kernel: its return shapes for every reduction, and its float32 values (b)
    within 4 x its own recorded distance from float64."""
    pred, gt = cases.golden_pair(name)
    F, J = gt.shape[:2]
    tol = 4.0 * float(golden[f"fp32_gap_{name}"]) * extent(gt).max()
    p, g = torch.from_numpy(pred).float().cuda(), torch.from_numpy(gt).float().cuda()
    for red in ("mean", "sum", "none"):
        scale = F * J if red == "sum" else 1
        crit = anerf.Criterion_MPJPE(reduction=red)
        v = crit(p, g)
        assert v.dtype == torch.float32 and v.is_cuda and tuple(v.shape) == golden[f"b_{name}_mpjpe_{red}"].shape
        same(v, golden[f"b_{name}_mpjpe_{red}"], tol * scale, f"module: mpjpe {red}")
        v, aligned = anerf.Criterion3DPose_ProcrustesCorrected(crit)(p, g)
        assert tuple(v.shape) == golden[f"b_{name}_pa_{red}"].shape and tuple(aligned.shape) == (F, J, 3)
        assert aligned.dtype == torch.float32 and aligned.is_cuda
        same(v, golden[f"b_{name}_pa_{red}"], tol * scale, f"module: pa {red}")
        if name in cases.WELL_CONDITIONED:
            same(aligned, golden[f"b_{name}_pa_aligned"], tol, "module: aligned")
        v, scaled = anerf.Criterion3DPose_leastQuaresScaled(crit)(p, g)
        assert tuple(v.shape) == golden[f"b_{name}_lsq_{red}"].shape and tuple(scaled.shape) == (F, J, 3)
        same(v, golden[f"b_{name}_lsq_{red}"], tol * scale, f"module: lsq {red}")
        same(scaled, golden[f"b_{name}_lsq_scaled"], tol, "module: scaled")
    # a criterion that is not Criterion_MPJPE is called on the aligned tensor
    v, aligned = anerf.Criterion3DPose_ProcrustesCorrected(lambda a, b: (a - b).abs().amax())(p, g)
    assert v.dim() == 0 and float(v) == float((aligned - g).abs().amax())


def test_gpu_procrustes_and_align_drop_ins(golden):
    pred, gt = cases.golden_pair("body17")
    ext = extent(gt)
    for scaling, reflection in cases.COMBOS:
        key = cases.combo_key("body17", scaling, reflection)
        d, Z, tform = anerf.procrustes(gt[1], pred[1], scaling, reflection)
        same(np.float64(d), golden[key + "_d"][1], TOL, "procrustes: d")
        same(np.float64(tform["scale"]), golden[key + "_b"][1], TOL * ext[1], "procrustes: b")
        same(tform["translation"], golden[key + "_c"][1], TOL * ext[1], "procrustes: c")
        same(tform["rotation"], golden[key + "_T"][1], TOL_Z, "procrustes: T")
        same(Z, golden[key + "_Z"][1], TOL_Z * ext[1], "procrustes: Z")
        aligned, tf = anerf.procrustes_align(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), scaling,
                                             reflection)
        assert aligned.dtype == torch.float32 and tuple(aligned.shape) == (3, 17, 3) and tf["rotation"].is_cuda
        same(aligned, golden[key + "_Z"], TOL_Z * ext, "procrustes_align: Z",
             extra=np.abs(golden[key + "_Z"]) * 2.0 ** -24)
        same(tf["scale"], golden[key + "_b"], TOL * ext, "procrustes_align: b")
    one, tf1 = anerf.procrustes_align(pred[0], gt[0])
    assert tuple(one.shape) == (17, 3) and tuple(tf1["rotation"].shape) == (3, 3)


def test_gpu_evaluate_pampjpe(golden):
    """(c): the tuples of evaluate_pampjpe_from_smpl_params from its line 566 on."""
    pred_m, gt_mm = cases.pampjpe_pair()
    tol = 4.0 * float(golden["fp32_gap_c"]) * extent(gt_mm).max()
    pred_t = torch.from_numpy(pred_m).float().cuda()
    for norm in (0, 1):
        for red in ("mean", "none"):
            k = f"c_n{norm}_{red}_"
            out = anerf.evaluate_pampjpe(pred_t, gt_mm, reduction=red, use_normalize=bool(norm))
            assert len(out) == 2
            same(out[0], golden[k + "pampjpe"], tol, f"evaluate_pampjpe: pampjpe {red}")
            same(out[1], golden[k + "mpjpe"], tol, f"evaluate_pampjpe: mpjpe {red} normalize={norm}")
            pa, mp, al = anerf.evaluate_pampjpe(pred_t, gt_mm, ret_kp=True, align_kp=True, reduction=red,
                                                use_normalize=bool(norm))
            same(al, golden[k + "aligned"], tol, "evaluate_pampjpe: aligned_kps")
            pa, mp, pck, auc = anerf.evaluate_pampjpe(pred_t, gt_mm, ret_kp=True, ret_pck=True, reduction=red,
                                                      use_normalize=bool(norm))
            # the kernel's integer counts over the (frame, joint) pairs under every reduction: the reference's
            # numbers under 'none' (under 'mean' it takes the PCK of one scalar)
            assert float(pck) == pytest.approx(float(golden[f"c_n{norm}_none_pck"]), abs=1e-7)
            assert float(auc) == pytest.approx(float(golden[f"c_n{norm}_none_auc"]), abs=1e-7)
            assert anerf.evaluate_pampjpe(pred_t, gt_mm, ret_kp=True, reduction=red)[2] is pred_t
        pa_sum, mp_sum = anerf.evaluate_pampjpe(pred_t, gt_mm, reduction="sum", use_normalize=bool(norm))
        n_pairs = golden[f"c_n{norm}_none_pampjpe"].size
        same(pa_sum / n_pairs, golden[f"c_n{norm}_mean_pampjpe"], tol, "evaluate_pampjpe: pampjpe sum")
        same(mp_sum / n_pairs, golden[f"c_n{norm}_mean_mpjpe"], tol, f"evaluate_pampjpe: mpjpe sum normalize={norm}")
    r = anerf.evaluate_poses(pred_m, gt_mm, pred_scale=1000.0, root=14)
    same(np.float64(r.pa_mpjpe), golden["c_n0_mean_pampjpe"], tol, "evaluate_poses: pa_mpjpe")
    same(np.float64(r.mpjpe_root), golden["c_n0_mean_mpjpe"], tol, "evaluate_poses: mpjpe_root")
    same(np.float64(r.n_mpjpe), golden["c_n1_mean_mpjpe"], tol, "evaluate_poses: n_mpjpe")
    assert r.pck == pytest.approx(float(golden["c_n0_none_pck"]), abs=1e-7)
    assert r.auc == pytest.approx(float(golden["c_n0_none_auc"]), abs=1e-7)

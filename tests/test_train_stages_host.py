"""CPU: the float64 restatements of the training stages (tests/_stage_ref.py) pinned, so that
tests/test_gpu_train_stages.py compares the kernels with something that is itself checked.

  * Forward against the record: encode() against the reference's committed feature rows (stage_feat of the fixtures
    tests/test_oracle_golden.py and tests/test_gpu_parity.py compare) and against the C oracle on random points;
    composite() against the goldens' weights, maps and alphas and against the oracle's raw2outputs; samples() against
    the goldens' coarse z.  Tolerances: those of the existing tests for the same comparison (features 1e-6 on the
    fixtures' rows, weights 2e-7, maps 1e-4, alpha 2e-3, coarse weights 1e-5), with ONE reasoned exception, applied
    only where float64 cannot meet the existing figure: the rows of three fixtures (ARG_LIMITED: v4_nocutoff 1.4e-5,
    sg3 1.3e-6, sg4 querypts 2.3e-5, all in their top frequencies) and the oracle on random points (base 2e-6, the
    bound test_gpu_parity uses there; measured up to 4.4e-5).  There a column takes base + 4.8e-7 * (its gain - 1),
    the gain (_stage_cases.column_gain) being 2^k (* 2 / c under --cutoff_shift) + tau / 4 where windowed.  The
    existing 1e-6 holds between two float32 programs that round the distance identically (the oracle repeats
    torch's fma chains); a float64 restatement sees the exact distance, a float32 rounding or two (2.4e-7 each at
    lengths in [2, 4)) away, and sin(2^k x) moves by 2^k times that.  Every other fixture's rows, windowed or not,
    are held to the plain 1e-6 (measured 5e-8 to 8e-7).
  * The restatement's autograd against central differences in float64 (directional, one direction per joint), on the
    GPU tests' inputs: guards the detach placement and the kinks.
  * Power of the inputs: severing any one term of the backward (detach) changes the reference gradient by at least
    100 x the bound the GPU test applies to it.
  * The conditions on the inputs, and the bounds themselves (8 x the float32 restatement's own error, floor 1e-6).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import oracle  # noqa: E402
import _stage_cases as sc  # noqa: E402
import _stage_ref as ref  # noqa: E402
from _golden import Golden  # noqa: E402

F32 = torch.float32
ENC_GOLDENS = ["v1_mr10_w64_d4", "v2_softplus_nocutview", "v3_nocutinputs", "v4_nocutoff",
               "cd1_cuttodist_s32i16_d8w128", "cs1_cutoffshift_s32i16_d4w128", "cb1_cutoffbones_s32i16_d8w128",
               "mr3_mrv1_s32i16_d4w64", "mr5_mrv2_s32i16_d8w256", "mr9_mrv3_s32i16_d8w128", "t2000_512_s64i128",
               "vw1_viewworld_s32i16_d8w128", "c4_512_s64i128_j65"]
STAGED_GOLDENS = ["sg1_relpos_s32i16_d4w128", "sg2_rayangle_mrb2_cb_s32i16_d8w128", "sg3_all_fs_s32i16_d8w256",
                  "sg4_querypts_shift_s32i16_d8w128"]
TOL_FEAT = 1e-6
# fixtures whose rows a float64 restatement cannot meet at 1e-6 (unwindowed top frequencies; relpos and querypts, whose
# frequencies multiply a float32-rounded coordinate): measured 1.4e-5, 1.3e-6 and 2.3e-5
ARG_LIMITED = ("v4_nocutoff", "sg3_all_fs_s32i16_d8w256", "sg4_querypts_shift_s32i16_d8w128")


def _encode_points(g, pts, dirs):
    """encode() at points with their own directions: one ray per point, z = 0."""
    n = pts.shape[0]
    rb = np.concatenate([pts, dirs], -1).astype(np.float32)
    leaf, _, _ = ref.expand_skts(g["skts"][0:1], np.zeros(n, np.int32), n, 1)
    return ref.encode(g.cfg, ref.embed_state(g.cfg, g.ckpt), leaf, rb, np.zeros((n, 1), np.float32)).detach().numpy()[:, 0]


ARG_ROUNDING = 4.8e-7  # two float32 roundings of a length in [2, 4): the local coordinates', then the norm's


def _assert_features(got, want, g, what, base_tol=TOL_FEAT):
    tol = base_tol + ARG_ROUNDING * (sc.column_gain(g.cfg, ref.embed_state(g.cfg, g.ckpt)) - 1.0)
    d = np.abs(got - want.astype(np.float64))
    print(f"{what}: max |restatement - record| {d.max():.2e}, max d / tol {float((d / tol).max()):.3f} "
          f"(tol {tol.min():.1e} .. {tol.max():.1e})")
    assert (d <= tol).all(), what


# ----------------------------------------------------------------------------- forward against the record
@pytest.mark.parametrize("name", ENC_GOLDENS + STAGED_GOLDENS)
def test_encode_matches_reference_features(name):
    g = Golden(name)
    rb = g.ray_batch()[:4]
    z = g["stage_z"][:, :4]
    leaf, _, _ = ref.expand_skts(g["skts"][0:1], np.zeros(4, np.int32), 4, 4)
    got = ref.encode(g.cfg, ref.embed_state(g.cfg, g.ckpt), leaf, rb, z).detach().numpy().reshape(16, -1)
    want = g["stage_feat"].reshape(16, -1)
    assert got.shape[1] == sc.feat_dim(g.cfg, False) and want.shape[1] >= got.shape[1]
    if name in ARG_LIMITED:
        _assert_features(got, want[:, :got.shape[1]], g, name)
    else:
        d = float(np.abs(got - want[:, :got.shape[1]]).max())
        print(f"{name}: max |restatement - record| {d:.2e} (1e-6)")
        assert d <= TOL_FEAT, name


@pytest.mark.parametrize("name", ENC_GOLDENS)
def test_encode_matches_oracle(name):
    g = Golden(name)
    om = oracle.OracleModel(g.cfg, g.ckpt)
    rng = np.random.default_rng(3)
    kp = -np.einsum("jab,ja->jb", g["skts"][0][:, :3, :3], g["skts"][0][:, :3, 3])  # joint positions
    pts = (kp[rng.integers(0, len(kp), 256)] + rng.normal(0, 0.35, size=(256, 3))).astype(np.float32)
    dirs = rng.normal(size=(256, 3)).astype(np.float32)
    # (2e-6: test_gpu_parity.test_encode_points_matches_oracle's bound for the oracle on random points)
    _assert_features(_encode_points(g, pts, dirs), om.encode(g["skts"][0], pts, dirs), g, name, base_tol=2e-6)


@pytest.mark.parametrize("name", ENC_GOLDENS + STAGED_GOLDENS + ["s1_single_s96i48_mrv0", "l1_lindisp_s32i16_d4w128"])
def test_composite_matches_reference_and_oracle(name):
    g = Golden(name)
    rb = g.ray_batch()[:4]
    raw, z = g["stage_raw"], g["stage_z"]
    out = {k: v.numpy() for k, v in ref.composite(g.cfg, raw, z, rb[:, 3:6]).items()}
    np.testing.assert_allclose(out["weights"], g["stage_weights"], rtol=0, atol=2e-7)
    o = oracle.OracleModel(g.cfg, g.ckpt).raw2outputs(raw, z, rb[:, 3:6])
    np.testing.assert_allclose(out["weights"], o["weights"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(out["alpha"], o["alpha"], rtol=0, atol=2e-3)
    sfx = "0" if g.cfg.N_importance > 0 else "_map"
    for k, gk in (("rgb", "rgb" + sfx), ("disp", "disp" + sfx), ("acc", "acc" + sfx)):
        np.testing.assert_allclose(out[k], o[k + "_map"], rtol=0, atol=1e-4, err_msg=k)
        np.testing.assert_allclose(out[k], g["out_" + gk][:4], rtol=0, atol=1e-4, err_msg=k)
    ak = "out_alpha0" if g.cfg.N_importance > 0 else "out_alpha"
    np.testing.assert_allclose(out["alpha"], g[ak][:4], rtol=0, atol=2e-3)


@pytest.mark.parametrize("name", ["c2_256_s64_d8w256", "l1_lindisp_s32i16_d4w128", "s1_single_s96i48_mrv0"])
def test_samples_match_reference_coarse_z(name):
    g = Golden(name)
    z = ref.samples(g["stage_near"][:, 0], g["stage_far"][:, 0], g.cfg.N_samples, lindisp=g.cfg.lindisp).numpy()
    assert np.abs(z - g["stage_z"]).max() <= 1e-6 * np.abs(g["stage_z"]).max()
    assert (name[0] == "l") == g.cfg.lindisp


def test_samples_perturbed_intervals():
    """lower = z_0 in the first interval, upper = z_{S-1} in the last; t = 0 / 1 give the interval's ends."""
    near, far = np.float32([1.0]), np.float32([3.0])
    for lindisp in (False, True):
        z = ref.samples(near, far, 5, lindisp=lindisp)[0]
        mids = 0.5 * (z[1:] + z[:-1])
        lo = ref.samples(near, far, 5, np.zeros((1, 5)), lindisp)[0]
        hi = ref.samples(near, far, 5, np.ones((1, 5)), lindisp)[0]
        assert torch.equal(lo, torch.cat([z[:1], mids])) and torch.equal(hi, torch.cat([mids, z[-1:]]))


# ----------------------------------------------------------------------------- conditions on the inputs
def test_input_conditions():
    n_relu = n_cos = 0
    for model in sc.COMP_MODELS:
        for ns in sc.COMP_NS:
            for noise in (False, True):
                b = sc.comp_batch(model, ns, noise)
                x = ref.density_preact(b["cfg"], b["raw"], b["noise"], dtype=F32).double()
                if b["cfg"].density_type == "relu":
                    assert float(x.abs().min()) >= 1e-3, (model, ns, noise)
                    assert bool((x[sc.EMPTY] < 0).all())
                    n_relu += x.numel()
                out = ref.composite(b["cfg"], b["raw"], b["z"], b["rb"][:, 3:6], b["noise"])
                wsum = out["weights"].sum(-1)
                for i in range(5):
                    assert b["g"]["acc"][i] == 0 or float(wsum[i]) <= 0.999, (model, ns, noise, i)
                assert b["g"]["acc"][sc.OPAQUE] == 0 and float(wsum[sc.OPAQUE]) > 0.999
                if ns >= 8:
                    # the opaque ray's transmittance underflows float32 (< 1.4e-45), not float64
                    T = out["weights"][sc.OPAQUE] / out["alpha"][sc.OPAQUE]
                    assert 0 < float(T[7]) < 1e-45
                w = out["weights"][sc.LAST]
                assert float(w[-1]) > 0.999 and float(w[:-1].abs().sum()) == 0
    for kw in sc.encode_cases():
        b = sc.enc_batch(**kw)
        if not b["cfg"].view_angle:
            continue
        N, S = b["z"].shape
        leaf, _, ok = ref.expand_skts(b["skts"], b["ray_pose"], N, S)
        cs = ref.ray_angle_cosines(leaf.detach(), b["rb"], b["z"], b["pts_noise"]).abs()
        if kw.get("on_ray_joint"):
            c0 = cs[:, :, 0]
            assert bool((c0 > 1 - 5e-7).all()) and bool((c0 < 1 - 1e-9).all()), "joint 0 is the clamp's own case"
            cs = cs[:, :, 1:]
        assert float(cs.max()) <= 1 - 1e-6 - 1e-3, kw
        n_cos += cs.numel()
    assert n_relu > 0 and n_cos > 0


# ----------------------------------------------------------------------------- autograd against central differences
FD_H = 1e-6  # (the encoder: 2e-7, its top frequency is 2^9 * 2 / c = 2300)
FD_TOL = 2e-5  # of sum |g_k V_k|: truncation h^2 f(3) / (6 f(1)) = 4e-14 2300^2 / 6 = 4e-8, and conditioning
FD_ABS = 1e-8  # rounding of the difference itself, eps |L| / h


def _fd_encode(b):
    N, S = b["z"].shape
    cfg = b["cfg"]
    dtype = ref.F64
    g = torch.as_tensor(b["g_feat"], dtype=dtype)
    base, pose, ok = ref.expand_skts(b["skts"], b["ray_pose"], N, S)
    okf = ok[:, None, None].to(dtype)
    wd = None
    if cfg.kp_relpos or cfg.kp_query:  # the windows' distance does not move with skts
        sk = base.detach()
        p = torch.as_tensor(b["rb"][:, None, 0:3], dtype=dtype) + torch.as_tensor(b["rb"][:, None, 3:6], dtype=dtype) * \
            torch.as_tensor(b["z"], dtype=dtype)[..., None]
        if b["pts_noise"] is not None:
            p = p + torch.as_tensor(b["pts_noise"], dtype=dtype)
        wd = ((sk[..., :3, :3] * p[:, :, None, None, :]).sum(-1) + sk[..., :3, 3]).norm(dim=-1)

    def loss(sk):
        f = ref.encode(cfg, b["st"], sk, b["rb"], b["z"], b["ray_pose"], b["n_poses"], b["pts_noise"], b["vw"],
                       window_dist=wd)
        return (torch.nan_to_num(f) * g * okf).sum()

    loss(base).backward()
    grad = base.grad
    rng = np.random.default_rng(11)
    worst = 0.0
    for j in range(cfg.n_joints):  # one direction per joint: a pose perturbation shared by the samples of a ray
        V = torch.zeros_like(base)
        V[:, :, j, :3, :] = torch.as_tensor(rng.normal(size=(N, 1, 3, 4))).expand(-1, S, -1, -1)
        with torch.no_grad():
            fd = (loss(base.detach() + 2e-7 * V) - loss(base.detach() - 2e-7 * V)) / 4e-7
        an = (grad * V).sum()
        scale = float((grad * V).abs().sum())
        if scale == 0.0:
            assert float(fd) == 0.0
            continue
        worst = max(worst, abs(float(fd - an)) / scale)
    return worst


FD_ENC = [dict(name=n, N=2, S=4) for n in sc.ENC] + [
    dict(name="i7_4", N=5, S=12, pose_form="mixed"), dict(name="s_relpos_mrb2", N=4, S=5, pose_form="shared", noise=True),
    dict(name="s_angle", N=2, S=6, on_ray_joint=True)]


@pytest.mark.parametrize("kw", FD_ENC, ids=sc.case_id)
def test_encode_autograd_matches_central_differences(kw):
    err = _fd_encode(sc.enc_batch(**kw))
    print(f"{sc.case_id(kw)}: |fd - <g, V>| / sum |g V| = {err:.2e} (bound {FD_TOL:.0e})")
    assert err <= FD_TOL


@pytest.mark.parametrize("model", list(sc.COMP_MODELS))
@pytest.mark.parametrize("ns", [1, 2, 65])
def test_composite_autograd_matches_central_differences(model, ns):
    b = sc.comp_batch(model, ns, noise=True)
    rng = np.random.default_rng(12)
    for which in sc.WHICH:
        _, grad, _ = sc.comp_reference(b, which, with_scale=False)

        def loss(raw):
            out = ref.composite(b["cfg"], raw, b["z"], b["rb"][:, 3:6], b["noise"])
            return sum((out[k] * torch.as_tensor(b["g"][k], dtype=ref.F64)).sum() for k in which)

        raw = torch.as_tensor(b["raw"], dtype=ref.F64)
        for _ in range(4):
            V = torch.as_tensor(rng.normal(size=raw.shape))
            V[sc.OPAQUE] = 0  # (its saturated alphas are flat; its own gradient is checked below)
            fd = (loss(raw + FD_H * V) - loss(raw - FD_H * V)) / (2 * FD_H)
            scale = float((grad * V).abs().sum())
            assert abs(float(fd - (grad * V).sum())) <= FD_TOL * scale + FD_ABS, (which, float(fd), scale)
        assert bool(torch.isfinite(grad).all())
        if b["cfg"].density_type == "relu":
            assert bool((grad[sc.EMPTY, :, 3] == 0).all())


# ----------------------------------------------------------------------------- power of the inputs
POWER = 100.0
POWER_ENC = [
    ("kp_slope", dict(name="g5_2_tau200", N=3, S=6)),
    ("bone_slope", dict(name="g5_2_tau200", N=3, S=6)),
    ("view_slope", dict(name="g5_2_tau200", N=3, S=6)),
    ("bone_proj", dict(name="g1_0_nocutoff", N=3, S=6)),
    ("view_proj", dict(name="g1_0_nocutoff", N=3, S=6)),
    ("shift_factor", dict(name="w5_shift", N=3, S=6)),
    ("cut_to_sign", dict(name="i7_0_tau200_cutto", N=3, S=6)),
    ("angle_clamp", dict(name="s_angle", N=2, S=6, on_ray_joint=True)),
]


@pytest.mark.parametrize("term,kw", POWER_ENC, ids=[t + "-" + k["name"] for t, k in POWER_ENC])
def test_encoder_terms_are_visible_at_the_gpu_bound(term, kw):
    b = sc.enc_batch(**kw)
    assert kw in sc.encode_cases(), "the power is shown on a batch the GPU test runs"
    _, full, scale = sc.enc_reference(b)
    _, cut, _ = sc.enc_reference(b, cut=(term,), with_scale=False)
    change = sc.block_error(cut, full, scale)
    need = POWER * sc.BOUNDS["encode_backward"]
    print(f"{term}: severing it moves dL/dskts by {change:.2e} of a block's scale (need {need:.2e})")
    assert change >= need


@pytest.mark.parametrize("term,which", [("trans", ("rgb",)), ("disp", ("disp",)), ("g_weights", ("weights",)),
                                        ("g_alpha", ("alpha",)), ("trans", ref.COMPOSITE_OUTPUTS),
                                        ("disp", ref.COMPOSITE_OUTPUTS), ("g_weights", ref.COMPOSITE_OUTPUTS),
                                        ("g_alpha", ref.COMPOSITE_OUTPUTS)])
def test_composite_terms_are_visible_at_the_gpu_bound(term, which):
    b = sc.comp_batch("relu", 63, noise=True)
    _, full, scale = sc.comp_reference(b, which)
    _, cut, _ = sc.comp_reference(b, which, cut=(term,), with_scale=False)
    live = [0, 1]  # (the ordinary rays)
    change = sc.ray_error(cut[live], full[live], scale[live])
    need = POWER * sc.BOUNDS["composite_backward"]
    print(f"{term} with g on {which}: severing it moves dL/draw by {change:.2e} of a ray's max (need {need:.2e})")
    assert change >= need


# ----------------------------------------------------------------------------- the bounds
def measure_float32_reference():
    """Per family, the largest normalised error of the float32 restatement against the float64 one over the GPU
    tests' cases: the formulas' own float32 rounding on these inputs."""
    worst = {k: (0.0, None) for k in list(sc.BOUNDS) + ["encode_backward_plain"]}

    def note(fam, err, what):
        if err > worst[fam][0]:
            worst[fam] = (err, what)

    for S in sc.SAMPLE_S:
        for lindisp in (False, True):
            for t in sc.SAMPLE_T:
                near, far, tr = sc.sample_case(S, t)
                note("samples", sc.rel_error(ref.samples(near, far, S, tr, lindisp, dtype=F32),
                                             ref.samples(near, far, S, tr, lindisp)), (S, lindisp, t))
    for kw in sc.encode_cases() + ["dist0"]:
        b = sc.enc_batch(**kw) if kw != "dist0" else sc.dist0_batch()
        f64, g64, (scale, plain) = sc.enc_reference(b, plain_scale=True)
        f32, g32, _ = sc.enc_reference(b, dtype=F32, with_scale=False)
        note("encode_forward", sc.feature_error(f32, f64, sc.column_gain(b["cfg"], b["st"], b["vw"])), kw)
        note("encode_backward", sc.block_error(g32, g64, scale), kw)
        note("encode_backward_plain", sc.block_error(g32, g64, plain), kw)
    for model in sc.COMP_MODELS:
        for ns in sc.COMP_NS:
            for noise in (False, True):
                b = sc.comp_batch(model, ns, noise)
                for which in sc.WHICH:
                    o64, g64, scale = sc.comp_reference(b, which)
                    o32, g32, _ = sc.comp_reference(b, which, dtype=F32, with_scale=False)
                    for k in o64:
                        note("composite_forward", sc.rel_error(o32[k], o64[k]), (model, ns, noise, k))
                    note("composite_backward", sc.ray_error(g32, g64, scale), (model, ns, noise, which))
    return worst


def test_bounds_come_from_the_float32_restatement():
    worst = measure_float32_reference()
    err, what = worst.pop("encode_backward_plain")
    print(f"for the record, the encoder backward under the plain per-sample absolute sum: float32 restatement error "
          f"{err:.3e} at {what} (why the scale carries the features' gains, _stage_cases.enc_reference)")
    for fam, (err, what) in worst.items():
        print(f"{fam}: float32 restatement error {err:.3e} at {what}; 8 x = {sc.MARGIN * err:.3e}; "
              f"bound {sc.BOUNDS[fam]:.3e}")
    for fam, (err, what) in worst.items():
        rule = max(sc.FLOOR, sc.MARGIN * err)
        assert 0.5 * sc.BOUNDS[fam] <= rule <= 1.05 * sc.BOUNDS[fam], fam
        assert 0.9 * err <= sc.F32_ERR[fam] <= 1.1 * err, fam

"""Inputs shared by tests/test_train_stages_host.py (CPU) and tests/test_gpu_train_stages.py (device): the encoder
configurations (one per kernel instance of the encoder backward and per staged form), seeded ray / pose / gradient
batches built so that the hand-derived terms of the backward are visible, the composite's named rays, and the
comparisons' normalisations and bounds.

Geometry of an encoder batch: rays from near the origin along roughly -z, samples z in [1, 3]; every pose is a set of
rigid transforms whose joint j sits at distance c_j (+- 0.3 / tau) from one sample of a ray that uses the pose, so that
sample lies on the steep part of joint j's windows (slope -tau w (1 - w)).  With tau = 200 the three embedders' cutoff
distances are set equal (`equal_cutoffs`), so the same sample is within 1 / tau of all three.
"""
import importlib

import numpy as np
import torch

import _stage_ref as ref

config = importlib.import_module("a-nerf_amd.config")
syn = importlib.import_module("a-nerf_amd.synthetic")

# ---- bounds (normalised errors; see test_gpu_train_stages.py's docstring for the measurements behind them).
# Each is 8 x the largest float32-restatement error of its family over the cases below, floor 1e-6;
# test_train_stages_host.test_bounds_come_from_the_float32_restatement re-measures and holds them to that rule.
BOUNDS = {
    "samples": 1.0e-6,             # float32 restatement 8.5e-8 (x 8 = 6.8e-7: the floor)
    "encode_forward": 1.3e-5,      # 1.55e-6 (i7_4_tau2, shared pose, noise), in units of column_gain
    "encode_backward": 3.0e-6,     # 3.75e-7 (i7_4, 65 joints, 2 samples), of the gain-weighted term sum
    "composite_forward": 3.0e-6,   # 3.70e-7 (relu, 192 samples, rgb), of max |output|
    "composite_backward": 1.3e-5,  # 1.62e-6 (softplus, 1 sample, g_weights), of the ray's term sum
}
# the float32 restatement's own error behind each bound (the GPU tests print it beside the device's)
F32_ERR = {
    "samples": 8.5e-8,
    "encode_forward": 1.55e-6,
    "encode_backward": 3.75e-7,
    "composite_forward": 3.70e-7,
    "composite_backward": 1.62e-6,
}
FLOOR = 1e-6
MARGIN = 8.0

# ---- encoder configurations: name -> (RenderConfig keywords, tau, view_windows)
ENC = {
    # the five-plus-three compiled instances of train_encode_backward_kernel<MR, MRV>
    "i7_4": (dict(), 20.0, False),
    "i7_0_tau200_cutto": (dict(multires_views=0, cut_to_dist=True), 200.0, False),
    "i10_4_noinputs_shift": (dict(multires=10, cutoff_inputs=False, cutoff_shift=True), 20.0, False),
    "i10_0_noviewcut_cb": (dict(multires=10, multires_views=0, cutoff_viewdir=False, cutoff_bones=True), 20.0, False),
    "g5_2_world_cutto_shift": (dict(multires=5, multires_views=2, cut_to_dist=True, cutoff_shift=True,
                                    extra={"view_type": "world"}), 20.0, False),
    "g5_2_tau200": (dict(multires=5, multires_views=2, cutoff_bones=True), 200.0, False),
    # (RenderConfig.validate refuses multires 0: the smallest generic count is 1)
    "g1_0_nocutoff": (dict(multires=1, multires_views=0, use_cutoff=False), 20.0, False),
    # tau = 2, the wide window: every sample of a ray is on the window's slope, not only the one at the cutoff
    "i7_4_tau2": (dict(), 2.0, False),
    "w7": (dict(), 20.0, True),
    "w10_world_tau200_cb": (dict(multires=10, cutoff_bones=True, extra={"view_type": "world"}), 200.0, True),
    "w5_shift": (dict(multires=5, multires_views=2, cutoff_shift=True), 20.0, True),
    # encode_row_grad_joint_staged
    "s_relpos_mrb2": (dict(multires_bones=2, extra={"kp_dist_type": "relpos"}), 20.0, False),
    "s_relpos_angle_mrb2_cb": (dict(multires_bones=2, cutoff_bones=True, cutoff_inputs=False,
                                    extra={"kp_dist_type": "relpos", "view_type": "rayangle"}), 20.0, False),
    "s_query_shift": (dict(cutoff_shift=True, extra={"kp_dist_type": "querypts"}), 20.0, False),
    "s_angle_mrb2_cb_tau200": (dict(multires_bones=2, cutoff_bones=True, extra={"view_type": "rayangle"}), 200.0,
                               False),
    "s_angle_mrb2_cb_tau2": (dict(multires_bones=2, cutoff_bones=True, extra={"view_type": "rayangle"}), 2.0, False),
    "s_relpos_tau2": (dict(multires=5, extra={"kp_dist_type": "relpos"}), 2.0, False),
    "s_angle": (dict(multires=3, multires_views=2, extra={"view_type": "rayangle"}), 20.0, False),
    "s_mrb2_cutto": (dict(multires=5, multires_views=1, multires_bones=2, cut_to_dist=True), 200.0, False),
}

_CFG = {}


def enc_config(name, n_joints=24):
    """(cfg, ckpt, embed state, view_windows) of an encoder configuration at the smallest network the packer takes
    (the encoder and the composite read no weights)."""
    key = (name, n_joints)
    if key not in _CFG:
        kw, tau, vw = ENC[name]
        kw = dict(kw)
        extra = dict(kw.pop("extra", {}))
        cfg = config.RenderConfig(n_joints=n_joints, netdepth=4, netwidth=64, N_samples=8, N_importance=0,
                                  precision="fp32", extra=extra, **kw).validate()
        ckpt = syn.make_checkpoint(700 + n_joints, n_joints=n_joints, D=4, W=64, fine=False, tau=tau,
                                   multires=cfg.multires, multires_views=cfg.multires_views,
                                   cutoff_bones=cfg.cutoff_bones, tau_bones=1.5 * tau if cfg.cutoff_bones else None,
                                   multires_bones=cfg.multires_bones, kp_dims=3 if cfg.kp_relpos else 1,
                                   view_dims=1 if cfg.view_angle else 3, kp_query=cfg.kp_query)
        if tau >= 100.0 and not cfg.kp_query:  # equal_cutoffs: one sample within 1 / tau of every window
            cd = ckpt["embed_state_dict"]["cutoff_dist"]
            ckpt["embeddirs_state_dict"]["cutoff_dist"] = cd.copy()
            if cfg.cutoff_bones:
                ckpt["embedbones_state_dict"]["cutoff_dist"] = cd.copy()
                ckpt["embedbones_state_dict"]["tau"] = np.array(tau, np.float32)
        _CFG[key] = (cfg, ckpt, ref.embed_state(cfg, ckpt), vw)
    return _CFG[key]


def feat_dim(cfg, view_windows):
    return cfg.input_ch + cfg.input_ch_bones + (cfg.n_joints if view_windows else cfg.input_ch_views)


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)


def enc_batch(name, N, S, pose_form="per_ray", noise=False, n_joints=24, seed=0, on_ray_joint=False, dist0=False):
    """One encoder batch (float32 numpy): rb [N, 8], z [N, S], skts [n_poses, NJ, 4, 4], ray_pose (None: one
    skeleton per ray), pts_noise, g_feat [N, S, F].  pose_form: 'per_ray', 'shared' (every ray on pose 0 of 1) or
    'mixed' (3 poses; ray 1 has index -1 and ray 3 index n_poses).  on_ray_joint (one skeleton per ray, no noise): joint 0
    of every pose lies 1.5e-4 |d| beside its ray's line, 0.3 |d| behind the last sample: inside the windows, the
    ray-angle cosine of every sample within 2e-7 of -1, outside the clamp (1e-6), and not AT -1, where the cosine's
    own gradient would vanish and hide the clamp."""
    cfg, ckpt, st, vw = enc_config(name, n_joints)
    rng = np.random.default_rng([seed, N, S, n_joints, sum(map(ord, name + pose_form)), int(noise)])
    NJ = n_joints
    o = rng.normal(0, 0.05, size=(N, 3))
    d = np.array([0.0, 0.0, -1.0]) + rng.normal(0, 0.15, size=(N, 3))
    d *= rng.uniform(0.7, 1.3, size=(N, 1))  # un-normalised directions
    z = np.sort(rng.uniform(1.0, 3.0, size=(N, S)), -1)
    rb = np.concatenate([o, d, np.zeros((N, 1)), np.ones((N, 1))], -1).astype(np.float32)
    z = z.astype(np.float32)
    if dist0:  # (dyadic coordinates: o + d z is exact in float32, fused or not)
        rb[0, :6] = [0.25, 0.5, -0.75, 0.0, 0.0, 1.0]
        z[0] = np.linspace(0.5, 1.5, S)
    pn = rng.normal(0, 0.02, size=(N, S, 3)).astype(np.float32) if noise else None
    if pose_form == "per_ray":
        n_poses, ray_pose, owner = N, None, np.arange(N)
    elif pose_form == "shared":
        n_poses, ray_pose, owner = 1, np.zeros(N, np.int32), np.zeros(1, np.int64)
    else:
        assert pose_form == "mixed" and N == 5
        n_poses = 3
        ray_pose = np.array([0, -1, 2, n_poses, 0], np.int32)
        owner = np.array([0, 0, 2])  # (pose 1 has no ray at all)
    p = rb[:, None, 0:3].astype(np.float64) + rb[:, None, 3:6].astype(np.float64) * z[..., None].astype(np.float64)
    if noise:
        p = p + pn
    tau = st["tau"]
    cj = np.resize(st["cutoff"].astype(np.float64), NJ)  # (querypts: 3 cutoffs; any radius near 0.5 will do)
    skts = np.zeros((n_poses, NJ, 4, 4))
    for k in range(n_poses):
        ps = p[owner[k]]
        sj = rng.integers(0, S, size=NJ)
        users = [k] if ray_pose is None else [i for i in range(N) if ray_pose[i] == k] or [owner[k]]
        pu = p[users].reshape(-1, 3)
        du = np.repeat(rb[users, 3:6].astype(np.float64), S, axis=0)
        kp = np.zeros((NJ, 3))
        for j in range(NJ):
            # no sample of the pose's rays closer than 0.1 (the bone direction q / |q| is ill-conditioned there), no
            # ray-angle cosine within 0.01 of +-1 (acos' slope; the clamp has its own case)
            for _ in range(200):
                u = rng.normal(size=3)
                kp[j] = ps[sj[j]] + u / np.linalg.norm(u) * (cj[j] + rng.uniform(-0.3, 0.3) / tau)
                v = pu - kp[j]
                dist = np.linalg.norm(v, axis=-1)
                cs = (v * du).sum(-1) / (dist * np.linalg.norm(du, axis=-1))
                if dist.min() >= 0.1 and np.abs(cs).max() <= 0.99:
                    break
            else:
                raise AssertionError("no admissible joint position")
        if on_ray_joint:
            r = rb[owner[k]].astype(np.float64)
            perp = np.cross(r[3:6], [1.0, 0.0, 0.0])
            kp[0] = r[0:3] + r[3:6] * (float(z[owner[k]].max()) + 0.3) + perp / np.linalg.norm(perp) * 1.5e-4 * np.linalg.norm(r[3:6])
        R = _rotations(rng, NJ)
        skts[k, :, :3, :3] = R
        skts[k, :, :3, 3] = -np.einsum("jab,jb->ja", R, kp)
        skts[k, :, 3, 3] = 1.0
    if dist0:  # joint 0 of ray 0's pose: the identity rotation about the first sample, q = p - p = 0 exactly
        skts[0, 0] = np.eye(4)
        skts[0, 0, :3, 3] = [-0.25, -0.5, 0.25]
    g = rng.normal(size=(N, S, feat_dim(cfg, vw))).astype(np.float32)
    return dict(name=name, cfg=cfg, st=st, vw=vw, rb=rb, z=z, skts=skts.astype(np.float32), ray_pose=ray_pose,
                n_poses=n_poses, pts_noise=pn, g_feat=g)


def dist0_batch():
    """A sample exactly on a joint: dist = 0 in float32 and float64 alike."""
    return enc_batch("i7_4", 2, 3, seed=5, dist0=True)


def feature_kinds(cfg, view_windows):
    """The feature columns grouped into kinds (part, frequency slot, component): the NJ columns of a kind belong to
    NJ different joints, so one backward of a kind's sum holds every (sample, joint)'s own derivative of that one
    feature.  The querypts kp part is no function of the poses and is left out."""
    nj = cfg.n_joints
    parts = []
    if not cfg.kp_query:
        parts.append((0, 1 + 2 * cfg.multires, 3 if cfg.kp_relpos else 1))
    parts.append((cfg.input_ch, 1 + 2 * cfg.multires_bones, 3))
    o = cfg.input_ch + cfg.input_ch_bones
    parts.append((o, 1, 1) if view_windows else (o, 1 + 2 * cfg.multires_views, 1 if cfg.view_angle else 3))
    kinds = []
    for off, slots, dims in parts:
        for f in range(slots):
            for c in range(dims):
                kinds.append(off + (f * nj + np.arange(nj)) * dims + c)
    return kinds


def enc_reference(b, dtype=ref.F64, cut=(), with_scale=True, plain_scale=False):
    """The restatement on a batch: features, dL/dskts [n_poses, NJ, 4, 4] for g_feat, and the per-(pose, joint) scale
    of a comparison: the absolute sum, over the samples of the rays on the pose AND over the features, of
    |g_feat dfeature / dskts| times the feature's gain (column_gain), its largest value over the block's 12 entries.
    The plain per-sample sum is unusable in float32: under it the float32 restatement itself is 2.3e-3 off on these
    cases (i10_4_noinputs_shift; test_bounds_come_from_the_float32_restatement prints the figure).  It hides the
    cancellation inside a sample (a joint's gradient from one sample is the small difference of twenty terms of size
    2^k |g|) and the argument's rounding, which a term of frequency 2^k (2 / c) amplifies by that frequency (multires
    10 with --cutoff_shift: 2300 x 5e-7 = 1e-3 of the term, whatever computes it in float32).  With the gain in the
    scale a normalised error is in units of the ARGUMENT's error (a few 1e-7) for every configuration, so the
    top-frequency configuration does not set the bound of the others."""
    N, S = b["z"].shape
    leaf, pose, ok = ref.expand_skts(b["skts"], b["ray_pose"], N, S, dtype)
    feat = ref.encode(b["cfg"], b["st"], leaf, b["rb"], b["z"], b["ray_pose"], b["n_poses"], b["pts_noise"], b["vw"],
                      cut=cut, dtype=dtype)
    g = torch.as_tensor(b["g_feat"], dtype=dtype)
    terms = torch.nan_to_num(feat) * g * ok[:, None, None].to(dtype)
    if not with_scale:
        terms.sum().backward()
        grad, _ = ref.gather_pose_grad(leaf.grad, pose, ok, b["n_poses"])
        return feat.detach(), grad, None
    total, asum = torch.zeros_like(leaf), torch.zeros_like(leaf)
    gain = column_gain(b["cfg"], b["st"], b["vw"])
    for cols in feature_kinds(b["cfg"], b["vw"]):
        gk, = torch.autograd.grad(terms[:, :, cols].sum(), leaf, retain_graph=True)
        total += gk
        asum += gk.abs() * float(gain[cols[0]])
    grad, plain = ref.gather_pose_grad(total, pose, ok, b["n_poses"])
    _, a = ref.gather_pose_grad(asum, pose, ok, b["n_poses"])
    block = lambda x: x[:, :, :3, :].reshape(b["n_poses"], b["cfg"].n_joints, 12).max(-1).values  # noqa: E731
    if plain_scale:  # (the plain absolute sum of the per-sample contributions, for the record)
        return feat.detach(), grad, (block(a), block(plain))
    return feat.detach(), grad, block(a)


def block_error(got, want, scale):
    """max over the (pose, joint) blocks of max |got - want| over the block's 3 x 4 entries / the block's scale;
    blocks with no contribution at all (scale 0) must be exactly zero."""
    got, want, scale = (torch.as_tensor(np.asarray(x), dtype=torch.float64) for x in (got, want, scale))
    d = (got - want)[:, :, :3, :].abs().reshape(*scale.shape, 12).max(-1).values
    live = scale > 0
    assert bool((d[~live] == 0).all()), "a (pose, joint) block without contributions is not zero"
    return float((d[live] / scale[live]).max()) if bool(live.any()) else 0.0


def rel_error(got, want):
    """max |got - want| / max |want| (1 when the reference is all zero), NaNs in the same places."""
    got, want = (torch.as_tensor(np.asarray(x), dtype=torch.float64) for x in (got, want))
    assert got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaNs differ"
    m = float(torch.nan_to_num(want).abs().max())
    return float(torch.nan_to_num(got - want).abs().max()) / (m if m > 0 else 1.0)


def column_gain(cfg, st, view_windows=False):
    """Per feature column, |d feature / d argument| at most: 2^k for the sin / cos of frequency k (times 2 / c under
    --cutoff_shift in the kp part), 1 for a raw slot, plus tau / 4 (the window's steepest slope) where the column is
    windowed.  The argument (distance, local coordinate, world point) carries a float32 rounding that a float64
    restatement does not repeat, and the feature moves by this much times that rounding."""
    nj = cfg.n_joints

    def part(width, n_freq, a, tau_raw, tau_freq):
        g = [np.full(width, 1.0 + tau_raw / 4)]
        for k in range(n_freq):
            g += [np.full(width, a * 2.0 ** k + tau_freq / 4)] * 2
        return np.concatenate(g)

    use = bool(cfg.use_cutoff)
    shift = (2.0 / float(np.min(st["cutoff"]))) if (use and cfg.cutoff_shift) else 1.0
    kpw = 3 if cfg.kp_query else nj * (3 if cfg.kp_relpos else 1)
    t = st["tau"] if use else 0.0
    tb = st["tau_b"] if cfg.bone_window else 0.0
    tv = st["tau_v"] if cfg.view_window else 0.0
    cols = [part(kpw, cfg.multires, 1.0 if cfg.kp_relpos else shift, t if cfg.cutoff_inputs else 0.0, t),
            part(3 * nj, cfg.multires_bones, 1.0, tb if cfg.cutoff_inputs else 0.0, tb)]
    if view_windows:
        cols.append(np.full(nj, tv / 4))
    else:
        cols.append(part(nj * (1 if cfg.view_angle else 3), cfg.multires_views, 1.0, tv if cfg.cutoff_inputs else 0.0, tv))
    return np.concatenate(cols)


def feature_error(got, want, gain):
    """max over columns of max |got - want| / the column's gain (column_gain); NaN rows in the same places."""
    got, want = (torch.as_tensor(np.asarray(x), dtype=torch.float64) for x in (got, want))
    assert got.shape == want.shape and got.shape[-1] == len(gain)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaNs differ"
    d = torch.nan_to_num(got - want).abs().reshape(-1, len(gain)).max(0).values
    return float((d / torch.as_tensor(gain)).max())


# ----------------------------------------------------------------------------- layout edges of the encoder backward
def layout_cases():
    """(nj, ns, N) over nj in {2, 17, 24, 65} (spb = 256 // nj sample slots: 128, 15, 10, 3), ns in
    {1, spb - 1, spb, spb + 1, 67} (ns >= 1) and N in {1, 5}."""
    out = []
    for nj in (2, 17, 24, 65):
        spb = 256 // nj
        for ns in sorted({1, spb - 1, spb, spb + 1, 64 + 3} - {0}):
            for n in (1, 5):
                out.append((nj, ns, n))
    return out


def encode_cases():
    """Every encoder batch of the GPU tests, as enc_batch keywords (the host tests measure the float32 restatement
    on the same list): each configuration with one skeleton per ray and with all rays on one shared pose (with
    pts_noise), the layout edges, the pose forms with out-of-range indices, the ray angle's clamp."""
    out = []
    for name in ENC:
        out.append(dict(name=name, N=3, S=6))
        out.append(dict(name=name, N=4, S=5, pose_form="shared", noise=True))
    for i, (nj, ns, n) in enumerate(layout_cases()):
        out.append(dict(name="i7_4", N=n, S=ns, n_joints=nj, noise=bool(i % 2)))
    for name in ("i7_4", "s_relpos_angle_mrb2_cb", "w7", "s_query_shift", "i7_4_tau2"):
        out.append(dict(name=name, N=5, S=12, pose_form="mixed"))
        out.append(dict(name=name, N=5, S=67, pose_form="shared"))
    out.append(dict(name="s_angle", N=2, S=6, on_ray_joint=True))
    out.append(dict(name="s_angle_mrb2_cb_tau200", N=2, S=6, on_ray_joint=True))
    return out


def case_id(kw):
    return "-".join(f"{k[0]}{v}" if k != "name" else str(v) for k, v in kw.items())


# ----------------------------------------------------------------------------- samples
SAMPLE_S = (2, 3, 64)
SAMPLE_T = ("none", "zeros", "ones", "random")


def sample_case(S, t_kind, seed=0):
    rng = np.random.default_rng([seed, S])
    N = 5
    near = rng.uniform(0.5, 1.5, N).astype(np.float32)
    far = (near + rng.uniform(1.0, 3.0, N)).astype(np.float32)
    t = {"none": None, "zeros": np.zeros((N, S), np.float32),
         "ones": np.full((N, S), np.nextafter(np.float32(1), np.float32(0)), np.float32),
         "random": rng.random((N, S)).astype(np.float32)}[t_kind]
    return near, far, t


# ----------------------------------------------------------------------------- composite
COMP_NS = (1, 2, 63, 64, 65, 192)
EMPTY, OPAQUE, LAST = 2, 3, 4  # (the named rays of comp_batch)
COMP_MODELS = {
    "relu": dict(),
    "relu_scale": dict(density_scale=0.37),
    "softplus": dict(density_type="softplus", softplus_shift=1.0, density_scale=2.5),
}
_COMP = {}


def comp_config(model):
    if model not in _COMP:
        cfg = config.RenderConfig(n_joints=24, netdepth=4, netwidth=64, N_samples=8, N_importance=0, precision="fp32",
                                  **COMP_MODELS[model]).validate()
        _COMP[model] = (cfg, syn.make_checkpoint(701, n_joints=24, D=4, W=64, fine=False))
    return _COMP[model]


def comp_batch(model, ns, noise=False, seed=0):
    """Five rays (float32 numpy): raw [5, ns, 4], z, rb [5, 8] with un-normalised directions, noise, and upstream
    gradients for the five outputs.  Rays 0 and 1 are ordinary semi-transparent rays; ray 2 is EMPTY (every density
    pre-activation below 0); ray 3 is OPAQUE (every sample saturates alpha = 1, so the transmittance is 1e-10^s: it
    underflows float32 after 5 samples, not double; g_acc = 0 there); ray 4 has ONE occupied sample, the last (where
    the 1e10 distance applies).  The ordinary rays keep sum w <= 0.999, and no relu pre-activation lies within 1e-3
    of 0 (test_train_stages_host checks both)."""
    cfg, _ = comp_config(model)
    rng = np.random.default_rng([seed, ns, sum(map(ord, model)), int(noise)])
    N = 5
    B = cfg.density_scale
    z = np.sort(rng.uniform(1.0, 3.0, size=(N, ns)), -1).astype(np.float32)
    d = rng.normal(size=(N, 3))
    d *= (rng.uniform(0.6, 1.6, size=(N, 1)) / np.linalg.norm(d, axis=-1, keepdims=True))
    rb = np.concatenate([rng.normal(0, 0.1, size=(N, 3)), d, np.zeros((N, 1)), np.ones((N, 1))], -1).astype(np.float32)
    raw = rng.normal(0, 1.5, size=(N, ns, 4))
    nz = rng.normal(0, 0.3, size=(N, ns)) if noise else np.zeros((N, ns))
    # optical depths tau_s = sigma_s delta_s per sample: the ordinary rays total at most 4.1 (sum w <= 0.984), about
    # half of their samples occupied; sigma_s = tau_s / delta_s from the distances the kernel will see
    dn = np.linalg.norm(rb[:, 3:6].astype(np.float64), axis=-1, keepdims=True)
    delta = np.concatenate([np.diff(z.astype(np.float64), axis=-1), np.full((N, 1), 1e10)], -1) * dn
    occ = rng.random((N, ns)) < 0.5
    tau_s = rng.uniform(0.3, 1.7, (N, ns)) * 1.2 / max(0.5 * (ns - 1), 1.0)
    soft = cfg.density_type == "softplus"
    if soft:  # (softplus is never 0: the other samples are thin, not empty, and ray 2 is an ordinary ray)
        tau_s = np.where(occ, tau_s, 0.01 * tau_s)
        occ[:] = True
    occ[:, -1] = False
    occ[EMPTY] = soft
    occ[OPAQUE] = True
    tau_s[OPAQUE] = rng.uniform(200.0, 400.0, ns)
    tau_s[OPAQUE, -1] = 1e10 * dn[OPAQUE, 0]  # (sigma 1 at the 1e10 distance)
    occ[LAST] = False
    occ[LAST, -1] = True
    tau_s[LAST, -1] = 0.7e10 * dn[LAST, 0]  # (sigma 0.7 at the 1e10 distance)
    sigma = tau_s / delta
    if soft:
        x = cfg.softplus_shift + np.where(sigma > 30.0, sigma, np.log(np.expm1(np.minimum(sigma, 30.0))))
        x = np.where(occ, x, -80.0)  # (softplus(-81) 1e10 = 7e-26: alpha 0 in float32 and in float64)
    else:
        x = np.where(occ, sigma, -rng.uniform(0.05, 2.0, (N, ns)))
    raw[..., 3] = (x - nz) * B
    raw = raw.astype(np.float32)
    nz32 = nz.astype(np.float32) if noise else None
    g = dict(rgb=rng.normal(size=(N, 3)), disp=rng.normal(size=N), acc=rng.normal(size=N),
             weights=rng.normal(size=(N, ns)), alpha=rng.normal(size=(N, ns)))
    g["acc"][[OPAQUE, LAST]] = 0.0  # (sum w = 1 there: torch.minimum's tie)
    g = {k: v.astype(np.float32) for k, v in g.items()}
    return dict(model=model, cfg=cfg, raw=raw, z=z, rb=rb, noise=nz32, g=g)


def comp_reference(b, which, dtype=ref.F64, cut=(), with_scale=True):
    """Outputs, dL/draw [N, S, 4] for the upstream gradients named in `which`, and the per-ray scale of a comparison:
    the largest, over the ray's samples, of sum_k |G|_k |dw_k / dx_s| + |g_alpha_s dalpha_s / dx_s| (x the density
    channel), |G|_k the absolute sum of the terms of dL/dw_k (rgb, acc, the disparity's z_k and r parts, g_weights)
    -- the gradient's own terms before they cancel (G P against P R; z_k against r in the disparity) -- and of the
    ray's colour-channel gradients (one term each)."""
    raw = torch.as_tensor(b["raw"], dtype=dtype).requires_grad_(True)
    out = ref.composite(b["cfg"], raw, b["z"], b["rb"][:, 3:6], b["noise"], cut=cut, dtype=dtype)
    g = {k: torch.as_tensor(b["g"][k], dtype=dtype) if k in which else torch.zeros_like(out[k]) for k in out}
    loss = sum((out[k] * g[k]).sum() for k in which)
    grad = torch.zeros_like(raw)
    if loss.requires_grad:  # (not when `cut` severs the only output with a gradient)
        grad, = torch.autograd.grad(loss, raw, retain_graph=True)
    outs = {k: v.detach() for k, v in out.items()}
    if not with_scale:
        return outs, grad, None
    N, S = b["z"].shape
    z = torch.as_tensor(b["z"], dtype=dtype)
    w, rgb = outs["weights"], torch.sigmoid(raw.detach()[..., :3]) * 1.002 - 0.001
    wsum, depth = w.sum(-1), (w * z).sum(-1)
    den = wsum + 1e-10
    r = depth / den
    live = ((r > 1e-10) & (wsum.abs() > 1e-8)).to(dtype)
    gd_r = (g["disp"].abs() * live / torch.where(r > 0, r * r, torch.ones_like(r)))[:, None]
    Gabs = (g["rgb"][:, None, :] * rgb).abs().sum(-1) + (g["acc"].abs() * (wsum < 1).to(dtype))[:, None] + \
        gd_r * (z.abs() + r[:, None].abs()) / den[:, None] + g["weights"].abs()
    sig = torch.zeros(N, S, dtype=dtype)
    for k in range(S):  # d w_k / d x_s of every ray at once (the rays are independent)
        jk, = torch.autograd.grad(out["weights"][:, k].sum(), raw, retain_graph=True)
        sig += Gabs[:, k:k + 1] * jk[..., 3].abs()
    ja, = torch.autograd.grad(out["alpha"].sum(), raw, retain_graph=True)
    sig += g["alpha"].abs() * ja[..., 3].abs()
    scale = torch.maximum(sig.max(-1).values, grad[..., :3].abs().reshape(N, -1).max(-1).values)
    return outs, grad, scale


def ray_error(got, want, scale):
    """max over rays of max |got - want| over the ray / the ray's scale (comp_reference); a ray without any term
    (scale 0: the empty ray under relu) must be exactly zero."""
    got, want, scale = (torch.as_tensor(np.asarray(x), dtype=torch.float64) for x in (got, want, scale))
    d = (got - want).abs().reshape(want.shape[0], -1).max(-1).values
    d = (d - 1e-37).clamp_min(0.0)  # (below float32's normal range, e.g. exp(-300) on the opaque ray: not an error)
    live = scale > 1e-30
    assert bool((d[~live] == 0).all()), "a ray without gradient terms is not zero"
    return float((d[live] / scale[live]).max()) if bool(live.any()) else 0.0


WHICH = [("rgb",), ("disp",), ("acc",), ("weights",), ("alpha",), ref.COMPOSITE_OUTPUTS]

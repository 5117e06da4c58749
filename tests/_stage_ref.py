"""Plain, differentiable torch restatements of the training stages (csrc/anerf_train.hpp), written from the reference's
formulas: sample_from_lineseg (core/utils/ray_utils.py:204-251), sample_pts + encode_inputs + the embedders
(core/raycasters.py:476-555, 650-663; core/encoders.py:8-37, 101-212; core/cutoff_embedder.py:125-166) and
NeRF.raw2outputs (core/networks/nerf.py:150-205).  No device code; float64 by default, and the same code in float32
measures the formulas' own float32 rounding (tests/test_train_stages_host.py pins all of it: the forward against the
C oracle and the committed reference features, the autograd against central differences).

`cut` names a term whose gradient path is severed (detach) while every value stays the same: the host tests use it
to show that each term of the kernels' hand-derived chain rule is visible at the GPU tests' tolerances.
"""
import math

import numpy as np
import torch

F64 = torch.float64

# terms of the encoder's / the composite's backward that `cut` can sever
ENCODE_TERMS = ("kp_slope", "bone_slope", "view_slope", "bone_proj", "view_proj", "shift_factor", "cut_to_sign",
                "angle_clamp")
COMPOSITE_TERMS = ("trans", "disp", "g_weights", "g_alpha")

# torch.clamp(x, -1 + 1e-6, 1 - 1e-6) on a float32 tensor: the bounds are float32 values
_CLAMP_HI = float(np.float32(1.0) - np.float32(1e-6))
# F.normalize's eps on a float32 tensor is the float32 nearest 1e-12 (it sets the gradient g / eps at |x| = 0)
_EPS12 = float(np.float32(1e-12))


def _t(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.to(dtype)
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def embed_state(cfg, ckpt):
    """The embedders' window constants of a checkpoint: tau / cutoff_dist of the kp, view and bone embedders."""
    e, ev, eb = ckpt["embed_state_dict"], ckpt["embeddirs_state_dict"], ckpt.get("embedbones_state_dict") or {}
    f = lambda v: float(np.asarray(v, np.float32).reshape(-1)[0])  # noqa: E731
    st = dict(tau=f(e["tau"]), cutoff=np.asarray(e["cutoff_dist"], np.float32), tau_v=f(ev["tau"]),
              cutoff_v=np.asarray(ev["cutoff_dist"], np.float32))
    if cfg.bone_window:
        st.update(tau_b=f(eb["tau"]), cutoff_b=np.asarray(eb["cutoff_dist"], np.float32))
    return st


# ----------------------------------------------------------------------------- samples
def samples(near, far, S, t_rand=None, lindisp=False, dtype=F64):
    """sample_from_lineseg: z [N, S]; t_rand None: perturb = 0."""
    near, far = _t(near, dtype).reshape(-1, 1), _t(far, dtype).reshape(-1, 1)
    t = torch.linspace(0.0, 1.0, S, dtype=dtype)
    z = 1.0 / (1.0 / near * (1.0 - t) + 1.0 / far * t) if lindisp else near * (1.0 - t) + far * t
    if t_rand is not None:
        mids = 0.5 * (z[..., 1:] + z[..., :-1])
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * _t(t_rand, dtype)
    return z


# ----------------------------------------------------------------------------- encoder
def expand_skts(skts, ray_pose, n_rays, n_samples, dtype=F64):
    """The skeleton transforms as a leaf expanded per sample, [N, S, NJ, 4, 4] (requires_grad), and the rays whose
    pose index is in range.  One backward then holds every sample's own contribution to dL/dskts[pose]."""
    skts = _t(skts, dtype)
    n_poses = skts.shape[0]
    if ray_pose is None:
        pose = torch.arange(n_rays)
    else:
        pose = torch.as_tensor(np.asarray(ray_pose), dtype=torch.int64)
    ok = (pose >= 0) & (pose < n_poses)
    leaf = skts[pose.clamp(0, n_poses - 1)][:, None].expand(-1, n_samples, -1, -1, -1).clone().requires_grad_(True)
    return leaf, pose, ok


def gather_pose_grad(per_sample, pose, ok, n_poses):
    """Per-sample contributions [N, S, NJ, 4, 4] -> (dL/dskts [n_poses, NJ, 4, 4], its absolute sum); rays with an
    out-of-range pose contribute nothing."""
    c = per_sample * ok[:, None, None, None, None].to(per_sample.dtype)
    g = torch.zeros(n_poses, *per_sample.shape[2:], dtype=per_sample.dtype)
    a = torch.zeros_like(g)
    idx = pose.clamp(0, n_poses - 1)
    g.index_add_(0, idx, c.sum(1))
    a.index_add_(0, idx, c.abs().sum(1))
    return g, a


def _window(tau, dist, c, slope):
    """CutoffEmbedder's window 1 - sigmoid(tau (dist - c)); slope False: its value without the gradient path."""
    return 1.0 - torch.sigmoid(tau * ((dist if slope else dist.detach()) - c))


def _freqs(x, n, w):
    """[sin(2^k x) w, cos(2^k x) w] for k < n, stacked on a new leading slot axis (2n slots)."""
    out = []
    for k in range(n):
        out += [torch.sin(x * float(2 ** k)) * w, torch.cos(x * float(2 ** k)) * w]
    return out


def encode(cfg, st, skts, rb, z, ray_pose=None, n_poses=None, pts_noise=None, view_windows=False, cut=(),
           dtype=F64, window_dist=None):
    """Feature rows [N, S, F] in the layout of feat_layout() (kp part | bone part | view part, a part's column of
    frequency slot f, joint j, component c: (f NJ + j) dims + c).  skts [N, S, NJ, 4, 4] (expand_skts).  Rays whose
    ray_pose is outside [0, n_poses) get NaN rows.  window_dist [N, S, NJ]: the windows' distance as a constant (what
    relpos / querypts mean by "no function of the poses", for a finite difference that moves skts)."""
    cut = set(cut)
    assert cut <= set(ENCODE_TERMS), cut
    rb, z = _t(rb, dtype), _t(z, dtype)
    N, S = z.shape
    NJ = cfg.n_joints
    o, d = rb[:, 0:3], rb[:, 3:6]
    p = o[:, None, :] + d[:, None, :] * z[..., None]  # sample_pts
    if pts_noise is not None:
        p = p + _t(pts_noise, dtype).reshape(N, S, 3)
    A, t = skts[..., :3, :3], skts[..., :3, 3]
    q = (A * p[:, :, None, None, :]).sum(-1) + t  # [N, S, NJ, 3]: world -> joint-local
    er = (A * d[:, None, None, None, :]).sum(-1)  # rotated ray directions R_j d
    dist = q.norm(dim=-1)
    # relpos / querypts: the windows' distance is |p - kp_j|, no function of the poses (raycasters.py:530-533)
    dw = dist if not (cfg.kp_relpos or cfg.kp_query) else dist.detach()
    if window_dist is not None:
        assert cfg.kp_relpos or cfg.kp_query
        dw = _t(window_dist, dtype)
    cutoff = use = bool(cfg.use_cutoff)
    cut_in = use and bool(cfg.cutoff_inputs)
    cut_to, shift = use and bool(cfg.cut_to_dist), use and bool(cfg.cutoff_shift)
    one = torch.ones((), dtype=dtype)

    def kp_in(x, c):  # CutoffEmbedder's input transforms (cutoff_embedder.py:125-134)
        u = c - x if cut_to else x
        if cut_to and "cut_to_sign" in cut:
            u = x + (u - x).detach()
        uf = u * (2.0 / c) - 1.0 if shift else u
        if shift and "shift_factor" in cut:
            uf = u + (uf - u).detach()
        return u, uf

    def slots(parts):  # list of [N, S, NJ(, dims)] -> [N, S, slots * NJ * dims]
        return torch.stack([x.reshape(N, S, -1) for x in parts], 2).reshape(N, S, -1)

    # ---- kp part
    if cfg.kp_query:  # the world point, windowed by itself against its 3 cutoffs
        c3 = _t(st["cutoff"], dtype)[:3]
        wq = 1.0 - torch.sigmoid(st["tau"] * (p - c3)) if cutoff else one
        u, uf = kp_in(p, c3)
        kp = slots([u * wq if cut_in else u] + _freqs(uf, cfg.multires, wq))
    else:
        c = _t(st["cutoff"], dtype)
        w = _window(st["tau"], dw, c, "kp_slope" not in cut) if cutoff else one
        if cfg.kp_relpos:
            w3 = w[..., None] if cutoff else one
            kp = slots([q * w3 if cut_in else q] + _freqs(q, cfg.multires, w3))
        else:
            u, uf = kp_in(dist, c)
            kp = slots([u * w if cut_in else u] + _freqs(uf, cfg.multires, w))
    # ---- bone part: F.normalize(q) (x / max(|x|, 1e-12)), the bone embedder's window
    dn = dist.clamp_min(_EPS12)
    ub = q / (dn.detach() if "bone_proj" in cut else dn)[..., None]
    bone_win = bool(cfg.bone_window)
    bone_cut = bone_win and bool(cfg.cutoff_inputs)
    wb = one
    if bone_cut or (bone_win and cfg.multires_bones > 0):
        wb = _window(st["tau_b"], dw, _t(st["cutoff_b"], dtype), "bone_slope" not in cut)[..., None]
    bones = slots([ub * wb if bone_cut else ub] + _freqs(ub, cfg.multires_bones, wb if bone_win else one))
    # ---- view part
    cutv = bool(cfg.view_window)
    wv = _window(st["tau_v"], dw, _t(st["cutoff_v"], dtype), "view_slope" not in cut) if cutv else one
    if view_windows:
        assert cutv
        view = wv
    elif cfg.view_angle:  # RayAngEncoder (encoders.py:195-212)
        cs = (q * er).sum(-1) / (dist * er.norm(dim=-1))
        cl = cs.clamp(-_CLAMP_HI, _CLAMP_HI)
        if "angle_clamp" in cut:
            cl = cs + (cl - cs).detach()
        a = torch.acos(cl) - math.pi / 2
        view = slots([a * wv if (cutv and cfg.cutoff_inputs) else a] + _freqs(a, cfg.multires_views, wv))
    else:
        if cfg.extra.get("view_type", "relray") == "world":
            e = er
        else:
            en = er.norm(dim=-1).clamp_min(_EPS12)
            e = er / (en.detach() if "view_proj" in cut else en)[..., None]
        wv3 = wv[..., None] if cutv else one
        view = slots([e * wv3 if (cutv and cfg.cutoff_inputs) else e] + _freqs(e, cfg.multires_views, wv3))
    feat = torch.cat([kp, bones, view.reshape(N, S, -1)], -1)
    if ray_pose is not None:
        pose = torch.as_tensor(np.asarray(ray_pose), dtype=torch.int64)
        bad = (pose < 0) | (pose >= n_poses)
        feat = torch.where(bad[:, None, None], torch.full_like(feat, float("nan")), feat)
    return feat


def ray_angle_cosines(skts, rb, z, pts_noise=None):
    """The ray angle's cosine of every (sample, joint), float64: the clamp's distance is a condition on the inputs."""
    rb, z = _t(rb, F64), _t(z, F64)
    p = rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]
    if pts_noise is not None:
        p = p + _t(pts_noise, F64).reshape(*z.shape, 3)
    sk = _t(skts, F64)
    q = (sk[..., :3, :3] * p[:, :, None, None, :]).sum(-1) + sk[..., :3, 3]
    er = (sk[..., :3, :3] * rb[:, None, None, None, 3:6]).sum(-1)
    return (q * er).sum(-1) / (q.norm(dim=-1) * er.norm(dim=-1))


# ----------------------------------------------------------------------------- composite
def density_preact(cfg, raw, noise=None, dtype=F64):
    x = _t(raw, dtype)[..., 3] / cfg.density_scale
    return x if noise is None else x + _t(noise, dtype)


def composite(cfg, raw, z, dirs, noise=None, cut=(), dtype=F64):
    """raw2outputs with the training noise (given, already scaled): rgb [N, 3], disp [N], acc [N], weights and alpha
    [N, S]."""
    cut = set(cut)
    assert cut <= set(COMPOSITE_TERMS), cut
    raw, z, dirs = _t(raw, dtype), _t(z, dtype), _t(dirs, dtype)
    dists = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], 1e10)], -1)
    dists = dists * dirs.norm(dim=-1, keepdim=True)
    rgb = torch.sigmoid(raw[..., :3]) * 1.002 - 0.001
    x = density_preact(cfg, raw, noise, dtype)
    if cfg.density_type == "softplus":
        sigma = torch.nn.functional.softplus(x - cfg.softplus_shift)
    else:
        sigma = torch.relu(x)
    alpha = 1.0 - torch.exp(-sigma * dists)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    if "trans" in cut:
        T = T.detach()
    weights = alpha * T
    rgb_map = (weights[..., None] * rgb).sum(-2)
    depth = (weights * z).sum(-1)
    wsum = weights.sum(-1)
    disp = 1.0 / torch.maximum(torch.full_like(depth, 1e-10), depth / (wsum + 1e-10))
    disp = disp * (wsum.detach().abs() > 1e-8).to(dtype)  # isclose(sum w, 0): atol 1e-8
    if "disp" in cut:
        disp = disp.detach()
    acc = torch.minimum(wsum, torch.ones((), dtype=dtype))
    return dict(rgb=rgb_map, disp=disp, acc=acc, weights=weights.detach() if "g_weights" in cut else weights,
                alpha=alpha.detach() if "g_alpha" in cut else alpha)


COMPOSITE_OUTPUTS = ("rgb", "disp", "acc", "weights", "alpha")

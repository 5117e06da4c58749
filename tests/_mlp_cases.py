"""Checkpoints, points and rays at which the render kernels' MLP is held to float64 (tests/test_render_mlp_host.py,
tests/test_gpu_render_mlp.py), and the per-case references, computed once and shared.

Checkpoints come from synthetic.make_checkpoint (alpha_gain = rgb_gain = 1, embedder tau 20 / view tau 2: small, so
that the windows' sensitivity to one ulp of distance does not swamp the MLP's rounding) and are rewritten in the dict:
  he          every pts_linears, feature_linear and views_linears.0 weight x sqrt(6): torch's default init has a
              per-layer gain of ~1/sqrt(3), eight such layers are a contraction and an early layer's error has shrunk
              to nothing at the heads; x sqrt(6) is the variance-preserving (He) gain
  he_tails    he, magnitudes x exp(N(0, 1)), rows renormalised to the same gain, eight entries per layer x 16
  he_negbias  he with every hidden bias -|b|
  he_dead     he_negbias with the bone-direction columns of layer 0 and of the skip layer zeroed.  The bone directions
              are not windowed, so in he_negbias a point beyond every cutoff still has live inputs and no hidden row
              is all zero (measured: 40-50 % of such a row is positive).  Here such a point has no live input: every
              hidden row of it is exactly zero from layer 0 on -- the fp16 modes' per-sample scale of a zero maximum
              -- and the network's output there is its biases' alone (sigma = the alpha bias exactly)
  init        the unscaled checkpoint (report only: it hides the early layers)

Points: 515 per case = 16 whole 32-point blocks and a ragged one of 3, over four waves and more than one workgroup;
one seeded scene per joint count.  172 near joints (N(0, 0.08) around a joint), 3 exactly on a joint, 172 at 1-2
cutoff radii from a joint, 82 spread over the body (N(0, 0.35)), 86 beyond every cutoff (~100 units away: every
window exactly zero); shuffled, so a block holds near and far samples whose activations differ by orders of
magnitude.  Each point has its own direction.  "Exactly on a joint" is the origin: the root joint's rest position
is 0, so its local coordinates are 0 in every arithmetic (any other joint's are a rounded inverse transform away from
0, and a bone direction q / |q| at |q| ~ 1e-8 is decided by rounding); three directions there.
Classes for the criterion are by the float64 geometry, r = min_j |q_j| / c_j: "near" r < 1, "mid" 1 <= r < 4, "far"
beyond (there every kp and view window is exactly zero in float64 too; asserted).
"""
import dataclasses
import importlib
import math

import numpy as np
import torch

import _mlp_ref as M

anerf = importlib.import_module("a-nerf_amd")
syn = importlib.import_module("a-nerf_amd.synthetic")

N_POINTS = 515
TAU, TAU_VIEWS = 20.0, 2.0

# name: (W, D, joints, checkpoint, multires, framecode)
INSTANCES = {
    "w256_he": (256, 8, 24, "he", 7, False),
    "w256_he_tails": (256, 8, 24, "he_tails", 7, False),
    "w256_he_negbias": (256, 8, 24, "he_negbias", 7, False),
    "w256_he_dead": (256, 8, 24, "he_dead", 7, False),
    "w128_d6_j17": (128, 6, 17, "he", 7, False),  # the skip layer is the last hidden layer
    "w64_d4": (64, 4, 24, "he", 7, False),  # no skip layer; the encoder-fed parts stay on f32 MFMAs
    "w256_j65": (256, 8, 65, "he", 7, False),
    "w128_mr10": (128, 8, 24, "he", 10, False),
    "w128_framecode": (128, 8, 24, "he", 7, True),
    "w256_single": (256, 8, 24, "he", 7, False),  # single_net: render_fused_kernel
    "w256_init": (256, 8, 24, "init", 7, False),
}
POINT_CASES = [n for n in INSTANCES if n != "w256_single"]  # (the point-wise entries; init: reported, not asserted)
RAY_CASES = ["w256_he", "w128_d6_j17", "w64_d4"]
MUTANT_CASES = ["w256_he", "w256_he_tails"]
CAM = 2  # the framecode model's index


def _rewrite(sd, kind, rng, n_kp=0, nx=0):
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    if kind == "init":
        return sd
    scaled = [k for k in sd if k.endswith(".weight") and k.split(".")[0] in ("pts_linears", "feature_linear",
                                                                             "views_linears")]
    for k in sorted(scaled):
        w = sd[k].astype(np.float64) * math.sqrt(6.0)
        if kind == "he_tails":
            norm = np.linalg.norm(w, axis=1, keepdims=True)
            w = w * np.exp(rng.normal(0.0, 1.0, w.shape))
            w *= norm / np.linalg.norm(w, axis=1, keepdims=True)
            w.reshape(-1)[rng.choice(w.size, 8, replace=False)] *= 16.0
        sd[k] = w.astype(np.float32)
    if kind == "he_dead":
        for k in sd:
            if k.startswith("pts_linears") and k.endswith(".weight") and sd[k].shape[1] >= nx:  # layer 0, skip layer
                sd[k][:, n_kp:nx] = 0.0
    if kind in ("he_negbias", "he_dead"):
        for k in sd:
            if k.endswith(".bias") and k.split(".")[0] in ("pts_linears", "views_linears"):
                sd[k] = -np.abs(sd[k])
    return sd


def _scene(nj):
    """One pose: the 24-joint scene, its first 17 joints (every parent of theirs is among them), or the 65-joint one."""
    sc = syn.make_scene(n_joints=65 if nj > 24 else 24, H=128, W=128, seed=41)
    return dict(sc, kps=np.ascontiguousarray(sc["kps"][:, :nj]), skts=np.ascontiguousarray(sc["skts"][:, :nj]))


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _points(kps, cutoff, seed):
    rng = np.random.default_rng(seed)
    nj = len(kps)
    j = lambda n: kps[rng.integers(0, nj, n)].astype(np.float64)  # noqa: E731
    near = j(172) + rng.normal(0, 0.08, (172, 3))
    on = np.zeros((3, 3))
    ring = j(172) + _unit(rng, 172) * (rng.uniform(1.0, 2.0, (172, 1)) * float(np.mean(cutoff)))
    body = j(82) + rng.normal(0, 0.35, (82, 3))
    far = kps[0] + rng.normal(0, 1.0, (86, 3)) + np.array([60.0, -45.0, 80.0])
    pts = np.concatenate([near, on, ring, body, far])
    assert len(pts) == N_POINTS
    order = rng.permutation(N_POINTS)
    return pts[order].astype(np.float32), _unit(rng, N_POINTS).astype(np.float32)


def classify(cfg, ckpt, skts, pts):
    """near / mid / far by r = min_j |q_j| / c_j in float64."""
    sk = np.asarray(skts, np.float64).reshape(-1, 4, 4)
    q = np.einsum("jab,nb->nja", sk[:, :3, :3], np.asarray(pts, np.float64)) + sk[None, :, :3, 3]
    c = np.asarray(ckpt["embed_state_dict"]["cutoff_dist"], np.float64)
    r = (np.linalg.norm(q, axis=-1) / c).min(1)
    return np.where(r < 1, "near", np.where(r < 4, "mid", "far"))


class Case:
    """One instance: configuration, checkpoint, scene, points, and the evaluations every test shares (lazily, once)."""

    def __init__(self, name):
        self.name = name
        W, D, nj, kind, mr, fc = INSTANCES[name]
        self.kind = kind
        self.cfg = anerf.RenderConfig(n_joints=nj, netdepth=D, netwidth=W, multires=mr, opt_framecode=fc,
                                      n_framecodes=5 if fc else 0, N_samples=33, N_importance=31,
                                      single_net=name.endswith("_single"), precision="fp32").validate()
        self.asserted = kind != "init"
        seed = 500 + W + D + nj + mr + (7 if self.cfg.single_net else 0)
        ck = syn.make_checkpoint(seed, n_joints=nj, D=D, W=W, fine=True, tau=TAU, tau_views=TAU_VIEWS, alpha_gain=1.0,
                                 rgb_gain=1.0, use_framecode=fc, n_framecodes=5, multires=mr)
        rng = np.random.default_rng(seed + 1)
        for net in ("network_fn_state_dict", "network_fine_state_dict"):
            ck[net] = _rewrite(ck[net], kind, rng, n_kp=nj * (1 + 2 * mr), nx=nj * (1 + 2 * mr) + 3 * nj)
        self.ckpt = ck
        self.scene = _scene(nj)
        self.skts, self.kps = self.scene["skts"][0], self.scene["kps"][0]
        self.pts, self.dirs = _points(self.kps, ck["embed_state_dict"]["cutoff_dist"], seed + 2)
        self.cam = CAM if fc else None
        self._ev = {}

    def with_precision(self, precision):
        return dataclasses.replace(self.cfg, precision=precision)

    def net(self, fine=False):
        # (single_net: network_fine IS network_fn, and the fine keys are the ones loaded last)
        return M.Net(self.cfg, self.ckpt, fine=fine or self.cfg.single_net, cam=self.cam)

    def evaluate(self, pts=None, dirs=None, fine=False, key="points"):
        """dict(ref, y32 [n, 4] float64 arrays, feat32, classes, net) at the case's points, or at `pts` / `dirs` under
        `key`; emu(mode) adds the emulations."""
        k = (key, fine)
        if k not in self._ev:
            pts = self.pts if pts is None else pts
            dirs = self.dirs if dirs is None else dirs
            net = self.net(fine)
            f64 = M.features(self.cfg, self.ckpt, self.skts, pts, dirs, M.F64)
            f32 = M.features(self.cfg, self.ckpt, self.skts, pts, dirs, M.F32)
            with torch.no_grad():
                ref = net.forward(f64, M.F64).numpy()
                y32 = net.forward(f32, M.F32).to(M.F64).numpy()
            classes = classify(self.cfg, self.ckpt, self.skts, pts)
            far = classes == "far"
            if far.any():  # beyond every cutoff: the kp and view windows are exactly zero, in float64 too
                assert (f64[far][:, :net.n_kp] == 0).all() and (f64[far][:, net.nx:] == 0).all()
            self._ev[k] = dict(ref=ref, y32=y32, feat32=f32, feat64=f64, classes=classes, net=net, emu={})
        return self._ev[k]

    def emu(self, ev, mode, drop=None):
        if drop is not None:
            with torch.no_grad():
                return ev["net"].emulate(ev["feat32"], mode, drop).numpy()
        if mode not in ev["emu"]:
            with torch.no_grad():
                ev["emu"][mode] = ev["net"].emulate(ev["feat32"], mode).numpy()
        return ev["emu"][mode]

    # -- 12 rays through the body (12: no multiple of the 4 rays a workgroup takes), near / far given
    def rays(self):
        rng = np.random.default_rng(77)
        o = self.scene["c2ws"][0][:3, 3].astype(np.float64)
        target = self.kps[rng.integers(0, len(self.kps), 12)] + rng.normal(0, 0.05, (12, 3))
        d = target - o
        dist = np.linalg.norm(d, axis=1)
        d = d / dist[:, None]
        rb = np.concatenate([np.broadcast_to(o, d.shape), d, (dist - 0.9)[:, None], (dist + 0.9)[:, None], d], 1)
        return np.ascontiguousarray(rb, np.float32)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def sample_points(rb, z):
    """pts = rays_o + rays_d * z, the multiply and the add separately rounded in float32 (raycasters.py:658), and the
    rays' directions per sample: [n S, 3] each."""
    o, d = rb[:, 0:3].astype(np.float32), rb[:, 3:6].astype(np.float32)
    prod = (d[:, None, :] * z[:, :, None].astype(np.float32)).astype(np.float32)
    p = (o[:, None, :] + prod).astype(np.float32)
    return p.reshape(-1, 3), np.broadcast_to(d[:, None, :], p.shape).reshape(-1, 3).copy()

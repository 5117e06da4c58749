"""The render kernels' MLP (csrc/anerf_mlp.hpp) restated on the host: no device code.

* features(): the feature rows of points with their own directions, from tests/_stage_ref.encode (a ray with origin p,
  direction d, z = 0, S = 1): float64 is the reference, float32 the formulas' own rounding.
* Net.forward(): NeRF.forward (core/networks/nerf.py:133-148) from the state-dict layout of synthetic.make_nerf_state:
  pts_linears with the [x | h] skip input, alpha_linear, feature_linear, views_linears.0 on [feature | view features
  (| framecode)], rgb_linear; raw (rgb, sigma) before any activation.  float64: the reference; float32: the yardstick.
* Net.emulate(mode, drop): the same forward in float64 with the operands of every product rounded as DESIGN §4
  documents the precision mode (restated from that text, not from the kernel); every layer's output is rounded to
  float32 once (the accumulators are float32), sums are exact.  So the emulation carries the operand formats' error
  and none of the summation's: the criterion takes max(E32, Eemu).

  What §4 says, part by part:
    hidden layers (h parts)   fp32: f32 | bf16x3: two bf16 planes (RNE), x0 w0 + x0 w1 + x1 w0 | bf16x6: three bf16
                              planes (activations by truncation, weights RNE of the running remainder), the six
                              products with i + j <= 2 | fp16x4: two fp16 planes after the layer's weight scale and the
                              sample's activation scale (powers of two, maximum into [2^10, 2^11)), four products |
                              fp16x3: fp16x4 without x1 w1
    view layer, h part        feature_linear fused in (W' = Wv_f Wf, b' = Wv_f bf + bv, formed in double and rounded
                              once); the hidden layers' format, except bf16x3: f32
    encoder-fed parts         layer 0 and the skip layer's x part (windowed kp features, bone directions): bf16x6 in
                              bf16x6; fp16 planes at fixed power-of-two scales in fp16x4 / fp16x3 (bounded features,
                              §9b); f32 in fp32 and bf16x3, and in every mode at width 64
    view-direction part, framecode, alpha head, rgb head: f32 in every mode

  drop = (layer, "w" | "x") removes every plane below the first of that operand in that layer (the one low plane of the
  two-plane modes; both of bf16x6's, whose third plane alone -- "w2" | "x2", reported only -- leaves the 16 bits that
  bf16x3 computes with and cannot show at the criterion's margin): the mutant set.  Layers: "L0" ..
  "L{D-1}" (the skip layer as "skip_x" and "skip_h"), "feature" (feature_linear evaluated as a layer of its own, then
  the view layer on its output), "view_h", "alpha".  A part that the mode runs in f32 has no plane to lose
  (mutants()); the alpha head is the exception the suite must still see: its mutant evaluates it in the mode's
  hidden-layer format with the low plane(s) lost.
"""
import numpy as np
import torch

import _stage_ref as R

F64, F32 = torch.float64, torch.float32
MODES = ("fp32", "bf16x3", "bf16x6", "fp16x3", "fp16x4")
ACCURATE = ("fp32", "bf16x6", "fp16x4", "fp16x3")  # "fp32-accurate"


def features(cfg, ckpt, skts, pts, dirs, dtype=F64):
    """Feature rows [n, F] of points (float32 values) with their own directions under one pose skts [NJ, 4, 4]."""
    pts, dirs = np.asarray(pts, np.float32), np.asarray(dirs, np.float32)
    n = pts.shape[0]
    rb = np.concatenate([pts, np.broadcast_to(dirs, pts.shape)], -1)
    with torch.no_grad():
        leaf, _, _ = R.expand_skts(np.asarray(skts, np.float32).reshape(1, cfg.n_joints, 4, 4), np.zeros(n, np.int32),
                                   n, 1, dtype=dtype)
        f = R.encode(cfg, R.embed_state(cfg, ckpt), leaf.detach(), rb, np.zeros((n, 1), np.float32), dtype=dtype)
    return f[:, 0].contiguous()


# ----------------------------------------------------------------------------- operand formats
def _pow2_into_top(m):
    """t = 2^k with m t in [2^10, 2^11) (k = 0 where m == 0), elementwise; exact."""
    _, e = torch.frexp(m)  # m = mant 2^e, mant in [0.5, 1)
    return torch.where(m > 0, torch.ldexp(torch.ones_like(m), 11 - e), torch.ones_like(m))


def _bf16_planes(x, n, trunc):
    """x (float64 holding float32 values) as n bf16 planes of the running remainder (each remainder exact)."""
    r, out = x.to(F32), []
    for _ in range(n):
        p = (r.view(torch.int32) & -65536).view(F32) if trunc else r.bfloat16().to(F32)
        out.append(p.to(F64))
        r = r - p
    return out


def _f16_planes(xs):
    """Scaled x as two fp16 planes, both rounded to nearest even."""
    p0 = xs.to(F32).half().to(F64)
    return [p0, (xs - p0).to(F32).half().to(F64)]


class _Fmt:
    """planes of both operands, the products kept, and which scaling."""
    def __init__(self, kind, nplanes, keep):
        self.kind, self.n, self.keep = kind, nplanes, keep


_F32 = _Fmt("f32", 1, lambda i, j: True)
_FMT = {"bf16x3": _Fmt("bf16", 2, lambda i, j: i + j <= 1), "bf16x6": _Fmt("bf16t", 3, lambda i, j: i + j <= 2),
        "fp16x3": _Fmt("f16", 2, lambda i, j: i + j <= 1), "fp16x4": _Fmt("f16", 2, lambda i, j: True)}


def _product(x, w, fmt, drop=None, xbound=None):
    """x [n, K] @ w [O, K]^T with the operands in fmt; drop "x" / "w" loses that operand's low plane(s).
    xbound: a fixed bound of |x| (the encoder-fed parts' fixed scale) instead of the per-sample maximum."""
    if fmt.kind == "f32":
        return x @ w.T
    if fmt.kind == "f16":
        sw = _pow2_into_top(w.abs().max())
        if xbound is None:
            t = _pow2_into_top(x.clamp_min(0).max(dim=1, keepdim=True).values)
        else:
            t = _pow2_into_top(torch.as_tensor(float(xbound), dtype=F64))
        xp, wp, unscale = _f16_planes(x * t), _f16_planes(w * sw), 1.0 / (t * sw)
    else:
        xp = _bf16_planes(x, fmt.n, fmt.kind == "bf16t")
        wp = _bf16_planes(w, fmt.n, False)
        unscale = 1.0
    if drop is not None:  # "x" / "w": every plane below the first; "x2" / "w2" (three planes): the third alone
        planes = xp if drop[0] == "x" else wp
        for i in range(fmt.n - 1 if len(drop) == 2 else 1, fmt.n):
            planes[i] = torch.zeros_like(planes[i])
    out = 0.0
    for i in range(fmt.n):
        js = [j for j in range(fmt.n) if fmt.keep(i, j)]
        out = out + xp[i] @ sum(wp[j] for j in js).T
    return out * unscale


def _r32(x):
    return x.to(F32).to(F64)


# ----------------------------------------------------------------------------- the network
class Net:
    def __init__(self, cfg, ckpt, fine=False, cam=None):
        """cam: a framecode index, or None for the eval-mode mean code (models with framecodes)."""
        self.cfg = cfg
        sd = ckpt["network_fine_state_dict" if fine else "network_fn_state_dict"]
        self.p = {k: torch.as_tensor(np.asarray(v, np.float32)).to(F64) for k, v in sd.items()}
        self.D, self.W = cfg.netdepth, cfg.netwidth
        self.skip = cfg.skips[0] if cfg.skips[0] < self.D - 1 else -1
        nj = cfg.n_joints
        self.n_kp = nj * (1 + 2 * cfg.multires)
        self.nx = self.n_kp + 3 * nj
        self.nv = 3 * nj * (1 + 2 * cfg.multires_views)
        self.code = None
        if cfg.opt_framecode:
            codes = self.p["framecodes.codes.weight"]
            self.code = _r32(codes.sum(0) / codes.shape[0]) if cam is None else codes[int(cam)]
        st = R.embed_state(cfg, ckpt)
        # |dist w_j| < max(|c_j|, c_j + 16.69 / tau); sin / cos times w and the bone directions: 1
        c = np.abs(st["cutoff"].astype(np.float64))
        self.kp_bound = max(1.0, float((c + 16.69 / st["tau"]).max()))
        p = self.p
        wv = p["views_linears.0.weight"]
        # feature_linear fused into the view layer's h part, formed in double and rounded once
        self.w_fused = _r32(wv[:, :self.W] @ p["feature_linear.weight"])
        self.b_fused = _r32(wv[:, :self.W] @ p["feature_linear.bias"] + p["views_linears.0.bias"])

    def _split(self, feat):
        x, v = feat[:, :self.nx], feat[:, self.nx:self.nx + self.nv]
        if self.code is not None:
            v = torch.cat([v, self.code.to(feat.dtype).expand(feat.shape[0], -1)], 1)
        return x, v

    def forward(self, feat, dtype=F64):
        """raw [n, 4] = (rgb, sigma), every operation in dtype."""
        p = {k: v.to(dtype) for k, v in self.p.items()}
        x, v = self._split(feat.to(dtype))
        h = x
        for i in range(self.D):
            h = torch.relu(torch.nn.functional.linear(h, p[f"pts_linears.{i}.weight"], p[f"pts_linears.{i}.bias"]))
            if i == self.skip:
                h = torch.cat([x, h], 1)
        lin = torch.nn.functional.linear
        sigma = lin(h, p["alpha_linear.weight"], p["alpha_linear.bias"])
        f = lin(h, p["feature_linear.weight"], p["feature_linear.bias"])
        hv = torch.relu(lin(torch.cat([f, v], 1), p["views_linears.0.weight"], p["views_linears.0.bias"]))
        return torch.cat([lin(hv, p["rgb_linear.weight"], p["rgb_linear.bias"]), sigma], 1)

    # -- the layers a mutant can name, and which of them a mode splits
    def layers(self):
        out = []
        for i in range(self.D):
            out += ["skip_x", "skip_h"] if i == self.skip + 1 and self.skip >= 0 else [f"L{i}"]
        return out + ["feature", "view_h", "alpha"]

    def trunk_layers(self):
        return [n for n in self.layers() if n not in ("feature", "view_h", "alpha")]

    def _fmt(self, mode, layer):
        if mode == "fp32":
            return _F32
        if layer in ("L0", "skip_x"):  # encoder-fed
            return _FMT[mode] if (mode != "bf16x3" and self.W >= 128) else _F32
        if layer in ("feature", "view_h"):
            return _F32 if mode == "bf16x3" else _FMT[mode]
        if layer == "alpha":
            return _F32
        return _FMT[mode]

    def mutants(self, mode):
        """(layer, operand) pairs that have a low plane in this mode, and the alpha head's."""
        if mode == "fp32":
            return []
        return [(n, o) for n in self.layers() for o in ("w", "x") if n == "alpha" or self._fmt(mode, n) is not _F32]

    def emulate(self, feat32, mode, drop=None):
        """raw [n, 4] in float64 from float32 feature rows, operands rounded as the mode documents."""
        assert mode in MODES and (drop is None or (drop[0], drop[1][0]) in self.mutants(mode)), (mode, drop)
        assert drop is None or len(drop[1]) == 1 or _FMT[mode].n == 3, drop
        p = self.p
        x, v = self._split(feat32.to(F64))
        dl, dop = drop if drop else (None, None)

        def prod(layer, a, w, xbound=None):
            fmt = self._fmt(mode, layer)
            if layer == "alpha" and dl == "alpha":
                fmt = _FMT[mode]
            return _product(a, w, fmt, dop if dl == layer else None, xbound if fmt.kind == "f16" else None)

        def enc(layer, w):  # the windowed kp part and the bone-direction part, each with its own scales
            return prod(layer, x[:, :self.n_kp], w[:, :self.n_kp], self.kp_bound) + \
                prod(layer, x[:, self.n_kp:], w[:, self.n_kp:self.nx], 1.0)

        h = None
        for i in range(self.D):
            w, b = p[f"pts_linears.{i}.weight"], p[f"pts_linears.{i}.bias"]
            if i == 0:
                a = enc("L0", w)
            elif self.skip >= 0 and i == self.skip + 1:
                a = prod("skip_h", h, w[:, self.nx:]) + enc("skip_x", w)
            else:
                a = prod(f"L{i}", h, w)
            h = torch.relu(_r32(a + b))
        sigma = _r32(prod("alpha", h, p["alpha_linear.weight"]) + p["alpha_linear.bias"])
        wv = p["views_linears.0.weight"]
        if dl == "feature":
            f = _r32(prod("feature", h, p["feature_linear.weight"]) + p["feature_linear.bias"])
            a = prod("view_h", f, wv[:, :self.W]) + p["views_linears.0.bias"]
        else:
            a = prod("view_h", h, self.w_fused) + self.b_fused
        hv = torch.relu(_r32(a + v @ wv[:, self.W:].T))
        rgb = _r32(hv @ p["rgb_linear.weight"].T + p["rgb_linear.bias"])
        return torch.cat([rgb, sigma], 1)


# ----------------------------------------------------------------------------- the criterion
COLS = ("r", "g", "b", "sigma")
FACTOR = 4.0  # summation order: MFMA k-blocks against torch's CPU sum, both ~ sqrt(k) 2^-24 (not tuned)
ELEMENT = 16.0  # a single element against the bound on its class's RMS
MIN_CLASS = 16  # a class with fewer points is judged only as part of "all"


def rms(err, sel):
    """RMS of err [n, 4] over the rows sel: one figure per column."""
    return np.sqrt((np.asarray(err, np.float64)[sel] ** 2).mean(0))


def class_masks(classes):
    """{"all": every point} plus one mask per class name of the array `classes` with at least MIN_CLASS members."""
    classes = np.asarray(classes)
    out = {"all": np.ones(classes.shape[0], bool)}
    for c in sorted(set(classes.tolist())):
        m = classes == c
        if m.sum() >= MIN_CLASS:
            out[c] = m
    return out


def bounds(mode, ref, y32, emu, classes):
    """{class: bound on E [4]}: FACTOR max(E32, Eemu(mode)) for the fp32-accurate modes, FACTOR Eemu for bf16x3."""
    out = {}
    for c, m in class_masks(classes).items():
        e32, eemu = rms(y32 - ref, m), rms(emu - ref, m)
        out[c] = FACTOR * (np.maximum(e32, eemu) if mode in ACCURATE else eemu)
    return out


def check(out, mode, ref, y32, emu, classes, what, assert_it=True, cols=(0, 1, 2, 3), skip=()):
    """The criterion on out [n, len(cols)] against those columns of ref (float64): per class and column E <= bound,
    every element within ELEMENT x its class's bound.  Prints E / E32 and E / bound per class; returns the worst
    E / bound.  skip: classes judged by the caller (they stay part of "all")."""
    cols = list(cols)
    out, ref, y32, emu = (np.asarray(a, np.float64) for a in (out, ref, y32, emu))
    ref, y32, emu = ref[:, cols], y32[:, cols], emu[:, cols]
    assert out.shape == ref.shape and np.isfinite(out).all(), what
    worst, msgs = 0.0, []
    b = bounds(mode, ref, y32, emu, classes)
    for c, m in class_masks(classes).items():
        if c in skip:
            continue
        e, e32 = rms(out - ref, m), rms(y32 - ref, m)
        el = np.abs(out - ref)[m].max(0)
        # (a bound of exactly 0 -- every evaluation equal to the reference -- admits only 0)
        re = np.where(b[c] > 0, e / np.where(b[c] > 0, b[c], 1), np.where(e > 0, np.inf, 0))
        rl = np.where(b[c] > 0, el / np.where(b[c] > 0, ELEMENT * b[c], 1), np.where(el > 0, np.inf, 0))
        r32 = np.where(e32 > 0, e / np.where(e32 > 0, e32, 1), 0)
        print(f"{what} [{c}, {int(m.sum())} pts] E/E32 " + " ".join(f"{x:.2f}" for x in r32) + " | E/bound "
              + " ".join(f"{x:.2f}" for x in re) + " | max elem/(16 bound) " + " ".join(f"{x:.2f}" for x in rl)
              + " | E32 " + " ".join(f"{x:.1e}" for x in e32))
        worst = max(worst, float(re.max()), float(rl.max()))
        if re.max() > 1 or rl.max() > 1:
            msgs.append(f"{c}: E/bound {re}, element/(16 bound) {rl}")
    if assert_it:
        assert not msgs, f"{what}: " + "; ".join(msgs)
    return worst


def mutant_ratio(mut, mode, ref, y32, emu, classes):
    """max over columns (and classes) of E(mutant) / bound, per column: [4]."""
    b = bounds(mode, ref, y32, emu, classes)
    best = np.zeros(4)
    for c, m in class_masks(classes).items():
        e = rms(mut - ref, m)
        best = np.maximum(best, np.where(b[c] > 0, e / np.where(b[c] > 0, b[c], 1), 0))
    return best

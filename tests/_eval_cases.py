"""Shared inputs and yardsticks of the frame-scoring tests (tests/test_eval_host.py, tests/test_gpu_eval.py).

* make_case: a synthetic frame pair -- a smooth ground truth quantised to uint8 with a flat white background, a
  prediction that is the ground truth plus sigma = 0.03 noise, and a block where both are flat and equal (there
  var = E[x^2] - mu^2 is pure cancellation).
* ssim_direct: the definition stated directly, a non-separable 121-tap float64 window per pixel.
* ssim_fp32_torch: the fp32 yardstick -- the published package's operation order (conv2d along H, then W, fp32 window,
  fp32 moments), with padding 5.  It is what the device kernel would compute in fp32, and why it does not.
"""
import functools
import importlib

import numpy as np
import torch
import torch.nn.functional as F

ev = importlib.import_module("a-nerf_amd.evaluation")

# map bound of the GPU test: the checker and the kernel agree to ~1e-12 before the kernel rounds its map to fp32, so
# one fp32 ulp at 1 (2^-23) with a factor of two
MAP_TOL = 2.0 ** -22
SCORE_TOL = 1e-9  # per-frame ssim (absolute) and psnr (dB) against the float64 checker


@functools.lru_cache(maxsize=None)
def make_case(h, w, seed, n_frames=1):
    """-> dict of gt_u8 [F][h][w][3] uint8, gt [F][h][w][3] float32 (= float32(gt_u8 / 255.)), pred float32, mask
    uint8 [F][h][w] (a partial disc).  Read-only: shared between tests."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    gts, preds, masks = [], [], []
    for f in range(n_frames):
        img = np.stack([0.5 + 0.4 * np.sin(0.31 * xx + 0.17 * yy + c + f) * np.cos(0.11 * xx - 0.23 * yy) for c in range(3)], -1)
        cy, cx, r = h * 0.55, w * 0.45, 0.33 * min(h, w)
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        img[~disc] = 1.0  # the flat white background
        u8 = np.clip(np.round(img * 255.0), 0, 255).astype(np.uint8)
        gt = (u8 / 255.).astype(np.float32)
        pred = (gt + 0.03 * rng.standard_normal(gt.shape)).astype(np.float32)
        pred[: h // 4, : w // 3] = gt[: h // 4, : w // 3]  # flat and equal
        gts.append(u8)
        preds.append(pred)
        masks.append(disc.astype(np.uint8))
    out = {"gt_u8": np.stack(gts), "pred": np.stack(preds), "mask": np.stack(masks)}
    out["gt"] = (out["gt_u8"] / 255.).astype(np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


def ssim_direct(x, y, data_range=1.0, border="same"):
    """The definition, directly: per pixel and channel the 121-tap float64 window over the zero-extended image
    (border "same") -> [H][W][C]; border "valid" -> the [H - 10][W - 10][C] interior."""
    g = ev.gaussian_window()
    w2 = np.outer(g, g)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    h, w, _ = x.shape

    def mean(v):
        p = np.pad(v, ((5, 5), (5, 5), (0, 0)))
        out = np.zeros_like(v)
        for dy in range(11):
            for dx in range(11):
                out += w2[dy, dx] * p[dy:dy + h, dx:dx + w]
        return out

    mx, my = mean(x), mean(y)
    vx, vy, vxy = mean(x * x) - mx * mx, mean(y * y) - my * my, mean(x * y) - mx * my
    m = ((2 * mx * my + c1) / (mx * mx + my * my + c1)) * ((2 * vxy + c2) / (vx + vy + c2))
    return m if border == "same" else m[5:h - 5, 5:w - 5]


def ssim_fp32_torch(x, y, data_range=1.0, device="cpu"):
    """The fp32 yardstick: torch conv2d (padding 5) in the published package's order, [F][H][W][3] -> the same."""
    X, Y = ((v if torch.is_tensor(v) else torch.tensor(np.array(v))).to(device, torch.float32).permute(0, 3, 1, 2)
            for v in (x, y))
    coords = torch.arange(11, dtype=torch.float32, device=device) - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).reshape(1, 1, 11).repeat(3, 1, 1)

    def blur(v):
        v = F.conv2d(v, g.reshape(3, 1, 11, 1), padding=(5, 0), groups=3)
        return F.conv2d(v, g.reshape(3, 1, 1, 11), padding=(0, 5), groups=3)

    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = blur(X), blur(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = blur(X * X) - mu1_sq, blur(Y * Y) - mu2_sq, blur(X * Y) - mu1_mu2
    cs = (2 * s12 + c2) / (s1 + s2 + c2)
    return (((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs).permute(0, 2, 3, 1)

"""Scoring of rendered frames: PSNR and SSIM on the device, and the reference's validation entry points over them.

  * `evaluate_frames` -- anerf_eval_frames (csrc/anerf_eval.hip): per-frame sums of the squared error and of the SSIM
    map over a rectangle, over rectangle x mask and over rectangle x box, one launch per frame size and one device
    read in all (the sums).
  * `evaluate_frames_reference` -- the same numbers in float64 NumPy on the host: the checker.
  * `evaluate_metric` -- core/utils/evaluation_helpers.py:257-385 (whole frames, the foreground mask, the box's pixels).
  * `evaluate_box_metric` -- run_render.py:883-968 (`--eval`: the same scores inside each frame's box).
  * `render_testset` -- run_nerf.py:148-180.

SSIM is defined here, not taken from a package (the reference imports pytorch_msssim): Wang et al.'s, per channel,
an 11-tap Gaussian window with sigma 1.5 normalised to sum 1 and applied separably, K1 = 0.01, K2 = 0.03,
C1 = (K1 L)^2, C2 = (K2 L)^2 for L = data_range, var = E[x^2] - mu^2, and
    map = ((2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1)) * ((2 cov_xy + C2) / (var_x + var_y + C2)).
border="same" (the default) takes zeros outside the scored rectangle without renormalising the weights (a conv2d with
padding 5): an image-sized map, what both call sites of the reference multiply by image-sized masks.  border="valid"
scores only the pixels whose window lies inside the rectangle: the rectangle, every mask and the squared error lose 5
pixels per side, and the mean is the published pytorch_msssim's number.  data_range defaults to 1.0, the range of the
images; 255.0 gives what the reference's `SSIM(size_average=False)` computes (the package's default range on [0, 1]
images).

Not covered: writing videos or images, MS-SSIM, LPIPS.  (The pose scores -- MPJPE, PA-MPJPE, PCK -- are posescore.py's.)
"""
import contextlib
import os
import warnings
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import rays as host_rays

WIN, RAD, SIGMA, K1, K2 = 11, 5, 1.5, 0.01, 0.03


@dataclass
class EvalScores:
    """Per-frame scores (float64 arrays of length F, in the order the frames were given).  psnr / ssim are over the
    scored rectangle, fg_* over its pixels with the mask set, valid_* over its pixels inside the frame's box (both
    equal the rectangle's without a mask / a box).  A mean over no pixel divides by 1 (denom = max(3 n, 1)) and an
    infinite PSNR is reported as 0, the reference's rules.  sums [F][9] = {n, sum se, sum ssim} x 3 as the kernel
    returned them; map: per-frame [H][W][3] SSIM maps when asked (device fp32 tensors from evaluate_frames, float64
    arrays from the checker), 0 outside the scored pixels."""
    psnr: np.ndarray
    ssim: np.ndarray
    fg_psnr: np.ndarray
    fg_ssim: np.ndarray
    valid_psnr: np.ndarray
    valid_ssim: np.ndarray
    n: np.ndarray
    n_fg: np.ndarray
    n_valid: np.ndarray
    sums: np.ndarray
    map: list = None


def gaussian_window():
    """The 11 float64 weights: exp(-d^2 / (2 sigma^2)), normalised to sum 1."""
    d = np.arange(WIN, dtype=np.float64) - RAD
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def _scores(sums, maps):
    sums = np.asarray(sums, np.float64).reshape(-1, 9)
    out = []
    for k in range(3):
        n, se, ss = sums[:, 3 * k], sums[:, 3 * k + 1], sums[:, 3 * k + 2]
        denom = np.maximum(3.0 * n, 1.0)
        with np.errstate(divide="ignore"):
            psnr = -10.0 * np.log10(se / denom)
        psnr[psnr == np.inf] = 0.0
        out += [psnr, ss / denom]
    return EvalScores(*out, sums[:, 0].copy(), sums[:, 3].copy(), sums[:, 6].copy(), sums, maps)


def _frames(x, image=True):
    """Stacked [F][H][W][C] (tensor or array; masks also [F][H][W] or [F][H*W]) or a per-frame list -> a list of
    per-frame tensors / arrays.  A lone [H][W][3] image is one frame; a lone mask goes in a list."""
    if x is None:
        return None
    if isinstance(x, (list, tuple)):
        return list(x)
    if image and x.ndim == 3:
        return [x]
    return [x[i] for i in range(x.shape[0])]


def _box(b):
    (x0, y0), (x1, y1) = b
    return [int(x0), int(y0), int(x1), int(y1)]


def _rect_tables(n, shapes, bboxes, crop):
    """Per frame: the scored rectangle (the box under `crop`, else the whole frame) and the box weight (None under
    `crop` or without boxes).  Boxes are (tl, br) = ((x0, y0), (x1, y1)) as render_path returns them."""
    if crop and bboxes is None:
        raise ValueError("crop=True needs bboxes")
    rects, boxes = [], None if (crop or bboxes is None) else []
    for i in range(n):
        h, w = shapes[i]
        if crop:
            rects.append(_box(bboxes[i]))
        else:
            rects.append([0, 0, w, h])
            if boxes is not None:
                boxes.append(_box(bboxes[i]))
    return rects, boxes


def _binary_mask_t(m, h, w, frames=1):
    """`frames` masks (bool, uint8 or float; [H][W], [H][W][C] or flat each) as uint8 0 / 1 [frames][H][W] on their
    device, without a host read: a frame with a value above 1 is a 0..255 image, thresholded at 128
    (run_render.py:911-912); otherwise != 0."""
    m = m.reshape(frames, h, w, -1)[..., 0]
    if m.dtype == torch.bool:
        return m.to(torch.uint8)
    hi = (m > 1).reshape(frames, -1).any(1)[:, None, None]
    return torch.where(hi, m >= 128, m != 0).to(torch.uint8)


def _tensor(x):
    """A tensor as it is; an array as a tensor (a read-only one copied: torch does not take those)."""
    if torch.is_tensor(x):
        return x
    x = np.asarray(x)
    return torch.from_numpy(x if x.flags.writeable else x.copy())


def _device_of(*groups):
    for g in groups:
        for x in g or []:
            if torch.is_tensor(x) and x.is_cuda:
                return x.device
    return torch.device("cuda", torch.cuda.current_device())


@torch.no_grad()
def evaluate_frames(rgbs, gts, masks=None, bboxes=None, crop=False, data_range=1.0, border="same", return_map=False):
    """Score frames on the device.  rgbs: fp32 [F][H][W][3] or a per-frame list (device tensors stay where they are,
    arrays are uploaded); gts the same, float in [0, 1] or uint8 (a byte v counts as float32(v / 255.)); masks per
    frame [H][W] / [H][W][1], bool, uint8 or float; bboxes per frame (tl, br).  crop=False scores whole frames and the
    boxes weigh the valid_* scores (evaluation_helpers' variant); crop=True takes each frame's box as the image
    (run_render's crop-then-score).  Frames of different sizes go to one launch per size.  -> EvalScores."""
    if border not in _lib.ANERF_EVAL_BORDERS:
        raise ValueError(f"border must be 'same' or 'valid', got {border!r}")
    rgbs_in, gts_in, masks_in = (_tensor(x) if isinstance(x, np.ndarray) else x for x in (rgbs, gts, masks))
    rgbs, gts, masks = _frames(rgbs), _frames(gts), _frames(masks, image=False)
    n = len(rgbs)
    if len(gts) != n or (masks is not None and len(masks) != n) or (bboxes is not None and len(bboxes) != n):
        raise ValueError("rgbs, gts, masks and bboxes must have one entry per frame")
    dev = _device_of(rgbs, gts, masks)
    shapes = [tuple(int(v) for v in r.shape[:2]) for r in rgbs]
    rects, boxes = _rect_tables(n, shapes, bboxes, crop)
    lib = _lib.load()
    st = _lib.stream_handle(dev)
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)
    all_sums, order, maps = [], [], [None] * n
    for (h, w), idx in groups.items():
        if torch.is_tensor(rgbs_in) and rgbs_in.dim() == 4:  # (one stacked tensor: no copy when it is fp32 on `dev`)
            pred = rgbs_in.to(dev, torch.float32).contiguous()
        else:
            pred = torch.stack([_tensor(rgbs[i]).to(dev, torch.float32).reshape(h, w, 3) for i in idx]).contiguous()
        if torch.is_tensor(gts_in) and gts_in.dim() == 4:  # (the dataset's uint8 images are read where they lie)
            u8 = gts_in.dtype == torch.uint8
            gt = (gts_in if u8 else gts_in.to(torch.float32)).to(dev).contiguous()
        else:
            g = [_tensor(gts[i]).to(dev).reshape(h, w, 3) for i in idx]
            u8 = all(x.dtype == torch.uint8 for x in g)
            gt = torch.stack([x if u8 else (x.float() / 255.0 if x.dtype == torch.uint8 else x.to(torch.float32))
                              for x in g]).contiguous()
        if masks is None:
            mk = None
        elif torch.is_tensor(masks_in):
            mk = _binary_mask_t(masks_in.to(dev), h, w, n).contiguous()
        else:
            mk = torch.cat([_binary_mask_t(_tensor(masks[i]).to(dev), h, w) for i in idx]).contiguous()
        r = np.ascontiguousarray([rects[i] for i in idx], dtype=np.int32)
        b = None if boxes is None else np.ascontiguousarray([boxes[i] for i in idx], dtype=np.int32)
        need = _lib.workspace("anerf_eval_workspace", len(idx), h, w)
        ws = torch.empty(need // 8, device=dev, dtype=torch.float64)
        sums = torch.empty(len(idx), 9, device=dev, dtype=torch.float64)
        mp = torch.empty(len(idx), h, w, 3, device=dev, dtype=torch.float32) if return_map else None
        _lib.check(lib.anerf_eval_frames(_lib.ptr(pred), _lib.ptr(gt), int(u8), _lib.ptr(mk),
                                         r.ctypes.data_as(_lib.c_i32p),
                                         None if b is None else b.ctypes.data_as(_lib.c_i32p), len(idx), h, w,
                                         float(data_range), _lib.ANERF_EVAL_BORDERS[border], _lib.ptr(mp),
                                         _lib.ptr(sums), _lib.ptr(ws), need, st), "anerf_eval_frames")
        all_sums.append(sums)
        order += idx
        if return_map:
            for k, i in enumerate(idx):
                maps[i] = mp[k]
    host = np.zeros((n, 9), np.float64)
    if n:
        host[np.asarray(order)] = torch.cat(all_sums, 0).cpu().numpy()  # (the one device read)
    return _scores(host, maps if return_map else None)


def _filter_rows(x, g):
    """11-tap filter along the last axis with zeros outside (same size)."""
    p = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(RAD, RAD)])
    out = np.zeros_like(x)
    for k in range(WIN):
        out += g[k] * p[..., k:k + x.shape[-1]]
    return out


def ssim_map_reference(x, y, data_range=1.0):
    """The float64 SSIM map of two [H][W][C] images under border="same" (zeros outside, separable)."""
    g = gaussian_window()
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    x = np.moveaxis(np.asarray(x, np.float64), -1, 0)
    y = np.moveaxis(np.asarray(y, np.float64), -1, 0)

    def blur(v):  # horizontal, then vertical
        return _filter_rows(_filter_rows(v, g).swapaxes(-1, -2), g).swapaxes(-1, -2)

    mx, my = blur(x), blur(y)
    vx, vy, vxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    m = ((2.0 * mx * my + c1) / (mx * mx + my * my + c1)) * ((2.0 * vxy + c2) / (vx + vy + c2))
    return np.moveaxis(m, 0, -1)


def _host_gt(g):
    g = _lib.host_array(g)
    if g.dtype == np.uint8:
        return (g / 255.).astype(np.float32).astype(np.float64)
    return g.astype(np.float32).astype(np.float64)


def _host_mask(m, h, w):
    m = _lib.host_array(m).reshape(h, w, -1)[..., 0]
    if m.dtype == np.bool_:
        return m
    return m >= 128 if (m > 1).any() else m != 0


def evaluate_frames_reference(rgbs, gts, masks=None, bboxes=None, crop=False, data_range=1.0, border="same",
                              return_map=False):
    """evaluate_frames in float64 NumPy on the host (the checker; the maps are float64, not rounded)."""
    if border not in _lib.ANERF_EVAL_BORDERS:
        raise ValueError(f"border must be 'same' or 'valid', got {border!r}")
    rgbs, gts, masks = _frames(rgbs), _frames(gts), _frames(masks, image=False)
    n = len(rgbs)
    shapes = [tuple(int(v) for v in r.shape[:2]) for r in rgbs]
    rects, boxes = _rect_tables(n, shapes, bboxes, crop)
    sums, maps = np.zeros((n, 9), np.float64), []
    for i in range(n):
        h, w = shapes[i]
        p = _lib.host_array(rgbs[i]).astype(np.float32).astype(np.float64).reshape(h, w, 3)
        g = _host_gt(gts[i]).reshape(h, w, 3)
        x0, y0, x1, y1 = rects[i]
        if not (0 <= x0 <= x1 <= w and 0 <= y0 <= y1 <= h):
            raise ValueError(f"rectangle {i} = {rects[i]} outside the {w} x {h} frame")
        full = np.zeros((h, w, 3), np.float64)
        full[y0:y1, x0:x1] = ssim_map_reference(p[y0:y1, x0:x1], g[y0:y1, x0:x1], data_range)
        s = RAD if border == "valid" else 0
        wr = np.zeros((h, w), bool)
        wr[min(y0 + s, h):max(y1 - s, 0), min(x0 + s, w):max(x1 - s, 0)] = True
        full *= wr[..., None]
        wm = wr if masks is None else wr & _host_mask(masks[i], h, w)
        wb = wr
        if boxes is not None:
            bx0, by0, bx1, by1 = boxes[i]
            wb = np.zeros((h, w), bool)
            wb[by0:by1, bx0:bx1] = True
            wb &= wr
        se = (g - p) ** 2
        for k, wt in enumerate((wr, wm, wb)):
            sums[i, 3 * k:3 * k + 3] = wt.sum(), se[wt].sum(), full[wt].sum()
        maps.append(full)
    return _scores(sums, maps if return_map else None)


def box_of_pixels(idx, W):
    """The box (tl, br) whose row-major enumeration is the pixel list `idx` (render_path's valid_idxs)."""
    idx = _lib.host_array(idx).reshape(-1).astype(np.int64)
    if idx.size == 0:
        return (0, 0), (0, 0)
    ys, xs = idx // W, idx % W
    tl, br = (int(xs.min()), int(ys.min())), (int(xs.max()) + 1, int(ys.max()) + 1)
    if not np.array_equal(idx, host_rays.box_pixels(tl, br, W)):
        raise ValueError("valid_idxs must enumerate a box's pixels in row-major order")
    return tl, br


def _append(path, value):
    with open(path, "a") as f:
        f.write(f"{value}\n")


@torch.no_grad()
def evaluate_metric(rgbs, gt_imgs, disps=None, gt_masks=None, valid_idxs=None, poses=None, kps=None, hwf=None,
                    centers=None, ext_scale=None, rgb_vid="rgb.mp4", disp_vid="disp.mp4", vid_base=None,
                    eval_postfix="", eval_both=False, white_bkgd=False, render_factor=0, bboxes=None,
                    data_range=1.0, border="same", backend=None):
    """core/utils/evaluation_helpers.py:257-385 over evaluate_frames (or `backend`, e.g. evaluate_frames_reference).
    Frames with an empty mask are dropped, a mean over no pixel divides by 1, an infinite PSNR counts as 0, the mean
    is over the frames; without masks the scores are over whole frames, with masks over the foreground, with
    eval_both over the box's pixels (psnr_fg / ssim_fg keep the foreground's).  The box comes from `bboxes`, else from
    valid_idxs, else (or when render_factor != 0) from the keypoints as render_path computes it.  render_factor > 0
    resizes the prediction to the ground truth's size on the device.  No video is written; with vid_base the
    psnr*.txt / ssim*.txt lines are appended.  psnr_fg / ssim_fg are None without masks."""
    backend = evaluate_frames if backend is None else backend
    rgbs, gts, masks = _frames(rgbs), _frames(gt_imgs), _frames(gt_masks, image=False)
    if eval_both and masks is None:
        raise ValueError("eval_both needs gt_masks")
    if render_factor > 0:
        sizes = [tuple(int(v) for v in g.shape[:2]) for g in gts]
        dev = _device_of(rgbs, gts)
        rgbs = [F.interpolate(_tensor(r).to(dev).float().permute(2, 0, 1)[None], size=s, mode="bilinear",
                              align_corners=False)[0].permute(1, 2, 0) for r, s in zip(rgbs, sizes)]
    if eval_both and bboxes is None:
        H, W, focal = hwf
        if valid_idxs is None or render_factor != 0:
            _, _, bboxes = host_rays.valid_pixels(_lib.host_array(poses).astype(np.float32), H, W, focal,
                                                  kps=_lib.host_array(kps), ext_scale=ext_scale,
                                                  centers=None if centers is None else _lib.host_array(centers))
        else:
            w = W if isinstance(W, int) else int(W[0])
            bboxes = [box_of_pixels(v, w) for v in valid_idxs]
    sc = backend(rgbs, gts, masks=masks, bboxes=bboxes if eval_both else None, crop=False, data_range=data_range,
                 border=border)
    keep = sc.n_fg > 0 if masks is not None else np.ones(len(rgbs), bool)

    def mean(v):
        with _quiet():
            return np.float64(np.mean(v[keep]))

    fg_psnr = fg_ssim = None
    if masks is not None:
        fg_psnr, fg_ssim = mean(sc.fg_psnr), mean(sc.fg_ssim)
    if masks is None:
        test_psnr, test_ssim = mean(sc.psnr), mean(sc.ssim)
    elif not eval_both:
        test_psnr, test_ssim = fg_psnr, fg_ssim
    else:
        test_psnr, test_ssim = mean(sc.valid_psnr), mean(sc.valid_ssim)
    if vid_base is not None:
        if os.path.dirname(vid_base):
            os.makedirs(os.path.dirname(vid_base), exist_ok=True)
        _append(vid_base + f"psnr{eval_postfix}.txt", test_psnr)
        _append(vid_base + f"ssim{eval_postfix}.txt", test_ssim)
        if eval_both:
            _append(vid_base + f"psnr{eval_postfix}_fg.txt", fg_psnr)
            _append(vid_base + f"ssim{eval_postfix}_fg.txt", fg_ssim)
    return {"psnr": test_psnr, "ssim": test_ssim, "psnr_fg": fg_psnr, "ssim_fg": fg_ssim}


@contextlib.contextmanager
def _quiet():
    """The mean of no frame is NaN, as the reference's: without NumPy's warning."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def _h36m_rows(x, h, w):
    """Pixels of an h x w frame as [h][w][C].  The h36m special case of run_render.py:919-925: images of 1002 rows
    against a 1000-row render lose their first and last row."""
    if h == 1000 and w > 0 and x.numel() % (h * w) != 0 and x.numel() % (1002 * w) == 0:
        return x.reshape(1002, w, -1)[1:-1]
    if h * w == 0 or x.numel() == 0 or x.numel() % (h * w) != 0:
        raise ValueError(f"{x.numel()} values are not the pixels of a {h} x {w} frame (nor of a 1002-row image "
                         "against a 1000-row one)")
    return x.reshape(h, w, -1)


@torch.no_grad()
def evaluate_box_metric(rgbs, accs, bboxes, gt_dict, basedir=None, data_range=1.0, border="same", backend=None):
    """run_render.py:883-968: PSNR / SSIM inside each frame's box, and over the box's foreground when masks are given.
    gt_dict: gt_paths (per frame uint8 pixels of the frame's size, any shape), gt_mask_paths (or None), is_gt_paths
    (must be False: reading image files is not covered), bg_imgs / bg_indices (or None).  A frame whose cropped mask
    is empty is skipped; gt * mask + (1 - mask) * bg is formed on the device; 1002-row (h36m) images and masks given
    against a 1000-row render lose their first and last row (where the render itself has 1002 rows nothing is trimmed
    and the rows are scored aligned: the reference then scores its trimmed image against the untrimmed render, one row
    off).  -> {'psnr', 'ssim', 'fg_psnr', 'fg_ssim'} lists; with basedir, scores.npy and score_final.txt."""
    backend = evaluate_frames if backend is None else backend
    if gt_dict.get("is_gt_paths"):
        raise NotImplementedError("is_gt_paths: reading image files is not covered, pass the pixels")
    gt_paths, mask_paths = gt_dict["gt_paths"], gt_dict.get("gt_mask_paths")
    bg_imgs, bg_indices = gt_dict.get("bg_imgs"), gt_dict.get("bg_indices")
    rgbs = _frames(rgbs)
    on_dev = backend is evaluate_frames
    dev = _device_of(rgbs) if on_dev else torch.device("cpu")
    gts, masks = [], None if mask_paths is None else []
    for i, rgb in enumerate(rgbs):
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        gt = _h36m_rows(_tensor(gt_paths[i]).to(dev), h, w)
        if gt.shape[-1] != 3:
            raise ValueError(f"gt_paths[{i}] has {gt.numel()} values, frame {i} is {h} x {w} x 3")
        if masks is not None:
            m = _binary_mask_t(_h36m_rows(_tensor(mask_paths[i]).to(dev), h, w), h, w)[0]
            if bg_imgs is not None:
                bg = _tensor(bg_imgs[int(bg_indices[i])]).to(dev).to(torch.float64)
                mf = m[..., None].to(torch.float64)
                gt = ((gt.to(torch.float64) / 255. if gt.dtype == torch.uint8 else gt.to(torch.float64)) * mf
                      + (1. - mf) * bg).float()
            masks.append(m)
        gts.append(gt)
    sc = backend(rgbs, gts, masks=masks, bboxes=bboxes, crop=True, data_range=data_range, border=border)
    s = sc.sums
    out = {"psnr": [], "ssim": [], "fg_psnr": [], "fg_ssim": []}
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(len(rgbs)):
            if masks is not None and s[i, 3] < 1:
                print(f"frame {i} is empty, skip")
                continue
            out["psnr"].append(-10. * np.log10(s[i, 1] / (3. * s[i, 0])))
            out["ssim"].append(s[i, 2] / (3. * s[i, 0]))
            if masks is not None:
                out["fg_psnr"].append(-10. * np.log10(s[i, 4] / (3. * s[i, 3])))
                out["fg_ssim"].append(s[i, 5] / (3. * s[i, 3]))
    if basedir is not None:
        os.makedirs(basedir, exist_ok=True)
        np.save(os.path.join(basedir, "scores.npy"), out, allow_pickle=True)
        with open(os.path.join(basedir, "score_final.txt"), "w") as f, _quiet():
            for k in out:
                f.write(f"{k}: {np.mean(out[k])}\n")
    return out


@torch.no_grad()
def render_testset(poses, hwf, args, render_kwargs, kps=None, skts=None, cyls=None, cams=None, bones=None,
                   subject_idxs=None, gt_imgs=None, gt_masks=None, bg_imgs=None, bg_indices=None, vid_base=None,
                   rgb_vid="rgb.mp4", disp_vid="disp.mp4", eval_metrics=False, render_factor=0, eval_postfix="",
                   save_npy=False, eval_both=False, centers=None, save_image=False):
    """run_nerf.py:148-180: render the test poses (render_frames at args.chunk // 8, the frames stay on the device),
    score them there when eval_metrics, download them once -> (metrics, rgbs, disps / disps.max()).  gt_imgs,
    gt_masks and bg_imgs may be device tensors ([F][H*W][C] as RayImageDataset holds them, or [F][H][W][C]).  No
    video or image is written (save_image raises)."""
    from .render import render_frames
    if save_image:
        raise NotImplementedError("save_image: writing images is not covered")
    rc = render_kwargs["ray_caster"]
    # (the render-only RayCaster has no train mode to go back to: only a caster that was training is switched)
    modes = hasattr(rc, "eval") and hasattr(rc, "train") and bool(getattr(rc, "training", False))
    if modes:
        rc.eval()
    try:
        frames, valid_idxs, bboxes = render_frames(
            poses, hwf, args.chunk // 8, render_kwargs, centers=centers, kp=kps, skts=skts, cyls=cyls, bones=bones,
            bg_imgs=bg_imgs, bg_indices=bg_indices, cams=cams, subject_idxs=subject_idxs,
            render_factor=args.render_factor, ext_scale=args.ext_scale, white_bkgd=args.white_bkgd, to_host=False)
    finally:
        if modes:
            rc.train()
    metrics = {"psnr": None, "ssim": None}
    if eval_metrics:
        H, W = hwf[0], hwf[1]
        n = len(frames)

        def shaped(x, c):
            if x is None:
                return None
            x = _frames(x, image=False)  # (stacked over the frames, never a lone image: [F][H*W][3] has 3 axes too)
            return [v.reshape(H if isinstance(H, int) else int(H[i]), W if isinstance(W, int) else int(W[i]), c)
                    for i, v in enumerate(x[:n])]

        metrics = evaluate_metric([f[0] for f in frames], shaped(gt_imgs, 3), None, shaped(gt_masks, -1), valid_idxs,
                                  poses=poses, kps=kps, hwf=hwf, ext_scale=args.ext_scale, rgb_vid=rgb_vid,
                                  disp_vid=disp_vid, vid_base=vid_base, eval_postfix=eval_postfix, centers=centers,
                                  eval_both=eval_both, white_bkgd=False, render_factor=args.render_factor,
                                  bboxes=bboxes if args.render_factor == 0 else None)
    both = torch.stack([torch.cat([f[0], f[1]], -1) for f in frames]).cpu().numpy()  # (the one download)
    rgbs, disps = np.ascontiguousarray(both[..., :3]), np.ascontiguousarray(both[..., 3:])
    disps[np.isnan(disps)] = 0.
    if save_npy:
        np.save(vid_base + rgb_vid + ".npy", rgbs)
        np.save(vid_base + disp_vid + ".npy", disps)
    disps = disps / disps.max()
    return metrics, rgbs, disps

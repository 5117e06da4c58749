"""Making a dataset on the device: sampling masks, keypoint masks, median backgrounds, the skeleton overlay.

Every loader of the reference runs the same pixel-level steps on the host (cv2, NumPy) before training can start.  Here
they are three entries of csrc/anerf_prep.hip over the byte images where the dataset keeps them:

  * `dilate_masks`, `erode_masks`, `sampling_masks` -- anerf_mask_morph: dilate_masks (core/load_surreal.py:50-59, used by
    load_h36m.py:187, load_3dhp.py:106-129, load_perfcap.py:36, load_mixamo.py:85-88) and get_mask's tail
    (core/load_zju.py:53-63).  `iterations` applications of a k x k all-ones element are one window of radius
    iterations (k - 1) / 2, so the kernel makes a single pass;
  * `draw_skeleton2d`, `draw_skeletons`, `draw_skeletons_3d`, `skeleton3d_to_2d`, `create_kp_mask(s)` --
    anerf_draw_segments under the reference's names and argument orders (core/utils/skeleton_utils.py:475-488, 774-816,
    1331-1398).  COVERAGE IS DEFINED HERE: a segment covers the pixels whose integer centre lies within width / 2 of it
    (an exact integer rule, include/anerf.h).  cv2.line fills a fixed-point polygon with round caps and its boundary
    pixels can differ; no comparison against cv2 has been run, so the difference is not measured.  Inside a
    keypoint mask the line is dilated by at least 2 pixels afterwards;
  * `median_backgrounds` -- anerf_background_median: np.median over a camera's frames (load_h36m.py:110,
    load_3dhp.py:76) and, with masks, over the frames whose mask is clear at the pixel (load_zju.py:266-281, :459-474);
  * `prepare_dataset` -- the mapping RayImageDataset takes, with `sampling_masks` and optionally `bkgds` / `bkgd_idxs`.

Each has a NumPy checker (`*_reference`) that the kernels are held bit-identical to (tests/test_gpu_prep.py), and the
checkers are held to scipy.ndimage, np.median and a brute force over Python integers (tests/test_prep_host.py).

Not covered: reading images or h5 files, cv2.resize / undistort, DeepLab masks (process_mask.py), anti-aliased lines,
structuring elements other than squares.
"""
import numpy as np
import torch

from . import _lib
from .kinematics import CanonicalSkeleton, SMPLSkeleton

MAX_RADIUS = _lib.ANERF_PREP_MAX_RADIUS
MAX_COORD = _lib.ANERF_PREP_MAX_COORD
MAX_CAMERA_FRAMES = _lib.ANERF_PREP_MAX_CAMERA_FRAMES
_OPS = {"dilate": _lib.ANERF_MORPH_DILATE, "erode": _lib.ANERF_MORPH_ERODE}
_DROPPED = 1 << 20  # an endpoint coordinate that anerf_draw_segments drops (outside [-8192, 8192])
# draw_skeleton2d's colours by joint name: (plain, flip)
_COLORS = {"left": ((100, 149, 237), (0, 128, 128)), "right": ((255, 0, 0), (128, 128, 0)),
           "": ((46, 204, 13), (128, 0, 128))}


def _dev(x, device=None):
    if device is not None:
        return torch.device(device)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    return torch.device("cuda", 0)


def _u8(x, device):
    """uint8 bytes on the device, contiguous: a tensor where it lies, a NumPy array uploaded once."""
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.bool:
            x = x.to(torch.uint8)
        if x.dtype != torch.uint8:
            raise ValueError(f"expected uint8, got {x.dtype}")
        return x.detach().to(device).contiguous()
    a = np.asarray(x)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype != np.uint8:
        raise ValueError(f"expected uint8, got {a.dtype}")
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _mask_planes(shape, H=None, W=None):
    """(N, H, W) of masks given as (N, H, W), (N, H, W, 1), (H, W) or, with H and W, (N, H*W[, 1])."""
    shape = tuple(int(s) for s in shape)
    if H is not None and W is not None:
        n = int(np.prod(shape)) // (int(H) * int(W)) if H * W else 0
        if n * int(H) * int(W) != int(np.prod(shape)):
            raise ValueError(f"masks of shape {shape} are not N x {H} x {W}")
        return n, int(H), int(W)
    if len(shape) == 4 and shape[3] == 1:
        return shape[:3]
    if len(shape) == 3:
        return shape
    if len(shape) == 2:
        return (1,) + shape
    raise ValueError(f"masks of shape {shape}: give (N, H, W), (N, H, W, 1), (H, W), or H and W with (N, H*W, 1)")


def fold_radius(kernel, iterations):
    """`iterations` applications of a kernel x kernel all-ones element as one window's half-width."""
    kernel, iterations = int(kernel), int(iterations)
    if kernel < 1 or kernel % 2 == 0:
        raise ValueError("kernel must be odd and >= 1 (a square all-ones element)")
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    radius = iterations * (kernel - 1) // 2
    if radius > MAX_RADIUS:
        raise ValueError(f"iterations * (kernel - 1) / 2 = {radius} is over the kernel's limit of {MAX_RADIUS}")
    return radius


def mask_morph(masks, op, radius, band=0, other=None, H=None, W=None, device=None):
    """anerf_mask_morph on masks of any byte values -> a device tensor of the input's shape.  op "dilate" / "erode";
    band > 0 clears the dilate-minus-erode == 1 border band (get_mask); other: ORed in as 0 / 1 bytes."""
    dev = _dev(masks, device)
    src = _u8(masks, dev)
    n, h, w = _mask_planes(src.shape, H, W)
    oth = None
    if other is not None:
        oth = _u8(other, dev)
        if oth.numel() != src.numel():
            raise ValueError("other must have as many bytes as masks")
    dst = torch.empty_like(src)
    with torch.cuda.device(dev):
        rc = _lib.load().anerf_mask_morph(_lib.ptr(src), _lib.ptr(dst), n, h, w, _OPS[op], int(radius), int(band),
                                          _lib.ptr(oth), _lib.stream_handle(dev))
    _lib.check(rc, "anerf_mask_morph")
    return dst


def dilate_masks(masks, extend_iter=1, kernel=5, H=None, W=None, device=None):
    """load_surreal.py's dilate_masks: cv2.dilate with a kernel x kernel element, extend_iter iterations."""
    return mask_morph(masks, "dilate", fold_radius(kernel, extend_iter), H=H, W=W, device=device)


def erode_masks(masks, extend_iter=1, kernel=5, H=None, W=None, device=None):
    """cv2.erode with a kernel x kernel element, extend_iter iterations."""
    return mask_morph(masks, "erode", fold_radius(kernel, extend_iter), H=H, W=W, device=device)


def sampling_masks(masks, extend_iter=3, kernel=5, erode_border=False, H=None, W=None, device=None):
    """get_mask's sampling mask (load_zju.py:53-63): the mask dilated extend_iter times and, with erode_border, cleared
    where one step's dilation minus one step's erosion is 1.  Without erode_border this is dilate_masks."""
    band = (int(kernel) - 1) // 2 if erode_border else 0
    if erode_border and band < 1:
        raise ValueError("erode_border needs kernel >= 3")
    return mask_morph(masks, "dilate", fold_radius(kernel, extend_iter), band=band, H=H, W=W, device=device)


# ---------------------------------------------------------------- skeleton segments
def skeleton_type_of(skel):
    nj = int(skel.shape[-2])
    if nj == 24:
        return SMPLSkeleton
    if nj == 17:
        return CanonicalSkeleton
    raise ValueError(f"no skeleton type with {nj} joints: pass skel_type")


def skeleton_colors(skel_type, flip=False):
    """(NJ, 3) uint8: draw_skeleton2d's colour of each joint's segment, by its name."""
    out = []
    for name in skel_type.joint_names:
        key = "left" if "left" in name else "right" if "right" in name else ""
        out.append(_COLORS[key][1 if flip else 0])
    return np.array(out, dtype=np.uint8)


def _float_dev(x, device, dtype=None):
    if isinstance(x, torch.Tensor):
        t = x.detach().to(device)
    else:
        t = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if dtype is not None:
        t = t.to(dtype)
    elif not t.is_floating_point():
        t = t.to(torch.float64)
    return t


def skeleton_segments(kp2ds, skel_type=SMPLSkeleton, device=None):
    """kp2ds (F, NJ, 2) -> (F, NJ, 4) int32 on the device: joint j's segment from round(j) to round(j + (parent - j)),
    half to even in the key points' own dtype, as draw_skeleton2d.  A coordinate that is not finite or lies outside
    [-8192, 8192] becomes one that makes anerf_draw_segments drop the segment."""
    dev = _dev(kp2ds, device)
    j = _float_dev(kp2ds, dev)
    parents = torch.as_tensor(np.asarray(skel_type.joint_trees, dtype=np.int64), device=dev)
    if j.ndim != 3 or j.shape[1] != len(parents) or j.shape[2] != 2:
        raise ValueError(f"kp2ds must be (F, {len(parents)}, 2), got {tuple(j.shape)}")
    e = torch.cat([torch.round(j), torch.round(j + (j[:, parents] - j))], dim=-1)
    ok = torch.isfinite(e) & (e.abs() <= MAX_COORD)
    return torch.where(ok, e, torch.full_like(e, _DROPPED)).to(torch.int32).contiguous()


def draw_segments(segs, H, W, width=3, colors=None, frames=None, device=None):
    """anerf_draw_segments.  segs (F, B, 4) int32.  With frames (F, H, W, 3) uint8 on the device: painted in place
    with colors (B, 3) and returned; without: the (F, H, W) coverage mask."""
    dev = _dev(frames if frames is not None else segs, device)
    segs = torch.as_tensor(segs).to(device=dev, dtype=torch.int32).contiguous()
    if segs.ndim != 3 or segs.shape[2] != 4:
        raise ValueError(f"segs must be (F, B, 4), got {tuple(segs.shape)}")
    F_, B = int(segs.shape[0]), int(segs.shape[1])
    mask = col = None
    if frames is None:
        mask = torch.empty(F_, int(H), int(W), dtype=torch.uint8, device=dev)
    else:
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8
                and frames.is_contiguous() and tuple(frames.shape) == (F_, int(H), int(W), 3)):
            raise ValueError("frames must be a contiguous uint8 device tensor (F, H, W, 3): they are painted in place")
        col = _u8(colors, dev)
        if tuple(col.shape) != (B, 3):
            raise ValueError(f"colors must be ({B}, 3)")
    with torch.cuda.device(dev):
        rc = _lib.load().anerf_draw_segments(_lib.ptr(segs), F_, B, int(H), int(W), int(width), _lib.ptr(col),
                                             _lib.ptr(mask), _lib.ptr(frames), _lib.stream_handle(dev))
    _lib.check(rc, "anerf_draw_segments")
    return mask if frames is None else frames


def _per_frame(v, n, what):
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        return np.full(n, float(a))
    a = a.reshape(-1)
    if len(a) != n:
        raise ValueError(f"{what} must be a number or one per frame")
    return a


def _focal_pairs(focals, n):
    """(n, 2) float64 of (fx, fy) rounded through float32, as focal_to_intrinsic_np's float32 matrix holds them."""
    f = np.asarray(host(focals), dtype=np.float64)
    if f.ndim == 0:
        f = np.full((n, 1), float(f))
    f = f.reshape(n, -1)
    if f.shape[1] == 1:
        f = np.repeat(f, 2, axis=1)
    if f.shape[1] != 2:
        raise ValueError("focals must be a number, (F,) or (F, 2)")
    return f.astype(np.float32).astype(np.float64)


def host(x):
    return _lib.host_array(x)


def skeleton3d_to_2d(kps, c2ws, H, W, focals, centers=None, device=None):
    """world_to_cam over nerf_c2w_to_extrinsic (skeleton_utils.py:442-445, 475-488, 1331-1349) in float64 on the
    device -> (F, NJ, 2).  H, W and focals may be per frame, focals as (fx, fy) pairs; the focal goes through float32 as
    the reference's intrinsic matrix does; a coordinate of +inf becomes 0 before the offset is added, as there.  c2ws'
    last row is taken as (0, 0, 0, 1): the extrinsic is the affine inverse of swap_mat(c2w)."""
    dev = _dev(kps, device)
    p = _float_dev(kps, dev, torch.float64)
    if p.ndim != 3 or p.shape[2] != 3:
        raise ValueError(f"kps must be (F, NJ, 3), got {tuple(p.shape)}")
    n = int(p.shape[0])
    c = _float_dev(c2ws, dev, torch.float64).reshape(n, 4, 4)
    sw = c[:, :3, :] * torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64, device=dev)
    c0, c1, c2, t = sw[:, :, 0], sw[:, :, 1], sw[:, :, 2], sw[:, :, 3]
    r0, r1, r2 = torch.linalg.cross(c1, c2), torch.linalg.cross(c2, c0), torch.linalg.cross(c0, c1)
    inv = torch.stack([r0, r1, r2], dim=1) / (c0 * r0).sum(-1)[:, None, None]
    cam = (inv[:, None, :, :] * (p - t[:, None, :])[:, :, None, :]).sum(-1)
    f = torch.from_numpy(_focal_pairs(focals, n)).to(dev)
    uv = cam[..., :2] * f[:, None, :] / cam[..., 2:3]
    uv = torch.where(uv == float("inf"), torch.zeros_like(uv), uv)
    if centers is None:
        off = np.stack([_per_frame(W, n, "W") * 0.5, _per_frame(H, n, "H") * 0.5], axis=1)
    else:
        off = np.asarray(host(centers), dtype=np.float64).reshape(n, 2)
    return uv + torch.from_numpy(off).to(dev)[:, None, :]


def draw_skeletons(imgs, skels, skel_type=SMPLSkeleton, width=3, flip=False, device=None):
    """draw_skeleton2d on every frame: imgs (F, H, W, 3) uint8 (device or NumPy), skels (F, NJ, 2) -> a painted copy
    on the device."""
    dev = _dev(imgs, device)
    src = _u8(imgs, dev)
    if src.ndim != 4 or src.shape[3] != 3:
        raise ValueError(f"imgs must be (F, H, W, 3), got {tuple(src.shape)}")
    out = src.clone() if (isinstance(imgs, torch.Tensor) and src.data_ptr() == imgs.data_ptr()) else src
    segs = skeleton_segments(skels, skel_type, dev)
    return draw_segments(segs, out.shape[1], out.shape[2], width, skeleton_colors(skel_type, flip), out, dev)


def draw_skeleton2d(img, skel, skel_type=None, width=3, flip=False, device=None):
    """One frame (H, W, 3) and its (NJ, 2) key points -> the painted copy (device)."""
    skel = skel if isinstance(skel, torch.Tensor) else np.asarray(skel)
    if skel_type is None:
        skel_type = skeleton_type_of(skel)
    return draw_skeletons(img[None], skel[None], skel_type, width, flip, device)[0]


def draw_skeletons_3d(imgs, skels, c2ws, H, W, focals, centers=None, width=3, flip=False, skel_type=SMPLSkeleton,
                      device=None):
    """The skeleton overlay of run_render.py:1032-1043: skels (F, NJ, 3) projected through c2ws and drawn."""
    dev = _dev(imgs, device)
    return draw_skeletons(imgs, skeleton3d_to_2d(skels, c2ws, H, W, focals, centers, dev), skel_type, width, flip, dev)


def create_kp_masks(masks, kp2ds=None, kp3ds=None, c2ws=None, hwf=None, extend_iter=3, skel_type=SMPLSkeleton,
                    device=None):
    """skeleton_utils.py's create_kp_masks: the projected skeleton drawn at width 3, dilated 5 x 5 extend_iter times
    and ORed into masks (N, H, W, 1) or (N, H, W) -> 0 / 1 bytes of the same shape on the device.  Two launches for
    all N masks."""
    dev = _dev(masks, device)
    m = _u8(masks, dev)
    n, h, w = _mask_planes(m.shape)
    if kp2ds is None:
        if kp3ds is None or c2ws is None or hwf is None:
            raise ValueError("give kp2ds, or kp3ds with c2ws and hwf")
        kp2ds = skeleton3d_to_2d(kp3ds, c2ws, hwf[0], hwf[1], hwf[2], device=dev)
    drawn = draw_segments(skeleton_segments(kp2ds, skel_type, dev), h, w, 3, device=dev)
    if int(drawn.shape[0]) != n:
        raise ValueError("one skeleton per mask")
    return mask_morph(drawn, "dilate", fold_radius(5, extend_iter), other=m, device=dev).reshape(m.shape)


def create_kp_mask(mask, kp, H=None, W=None, extend_iter=3, skel_type=SMPLSkeleton, device=None):
    """One mask (H, W, 1) or (H, W) and its (NJ, 2) key points."""
    kp = kp if isinstance(kp, torch.Tensor) else np.asarray(kp)
    return create_kp_masks(mask[None], kp2ds=kp[None], extend_iter=extend_iter, skel_type=skel_type, device=device)[0]


# ---------------------------------------------------------------- median backgrounds
def camera_lists(cam_idxs, n_cams=None):
    """cam_idxs (N,) -> order (N,) int32, cam_start (C + 1,) int32: camera c's frames are order[cam_start[c] :
    cam_start[c + 1]], in their own order (one stable argsort)."""
    cam = np.asarray(host(cam_idxs)).reshape(-1).astype(np.int64)
    C = (int(cam.max()) + 1 if cam.size else 0) if n_cams is None else int(n_cams)
    if cam.size and (cam.min() < 0 or cam.max() >= C):
        raise ValueError(f"cam_idxs must lie in [0, {C})")
    order = np.argsort(cam, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=C))]).astype(np.int32)
    return order, start


def _image_rows(shape, H, W):
    shape = tuple(int(s) for s in shape)
    if len(shape) == 4 and shape[3] == 3:
        return shape[0], shape[1], shape[2]
    if len(shape) == 3 and shape[2] == 3 and H is not None and W is not None and shape[1] == int(H) * int(W):
        return shape[0], int(H), int(W)
    raise ValueError(f"imgs of shape {shape}: give (N, H, W, 3), or (N, H*W, 3) with H and W")


def median_backgrounds(imgs, cam_idxs, masks=None, n_cams=None, H=None, W=None, return_counts=False, device=None):
    """Per-camera median backgrounds -> (C, H, W, 3) uint8 on the device (and, with return_counts, the (C, H, W) int32
    number of frames taken at each pixel).  imgs (N, H*W, 3) with H and W, or (N, H, W, 3); masks (N, H*W[, 1]) or
    (N, H, W[, 1]): only frames whose mask byte is 0 at the pixel are taken, a pixel no frame leaves clear gives 0."""
    dev = _dev(imgs, device)
    src = _u8(imgs, dev)
    n, h, w = _image_rows(src.shape, H, W)
    m = None
    if masks is not None:
        m = _u8(masks, dev)
        if m.numel() != n * h * w:
            raise ValueError("masks must have one byte per pixel of imgs")
    order, start = camera_lists(cam_idxs, n_cams)
    if len(order) != n:
        raise ValueError("one cam_idx per image")
    C = len(start) - 1
    order_d, start_d = torch.from_numpy(order).to(dev), torch.from_numpy(start).to(dev)
    out = torch.empty(C, h, w, 3, dtype=torch.uint8, device=dev)
    counts = torch.empty(C, h, w, dtype=torch.int32, device=dev) if return_counts else None
    with torch.cuda.device(dev):
        rc = _lib.load().anerf_background_median(_lib.ptr(src), _lib.ptr(m), n, h * w,
                                                 order.ctypes.data_as(_lib.c_i32p), start.ctypes.data_as(_lib.c_i32p),
                                                 _lib.ptr(order_d), _lib.ptr(start_d), C, _lib.ptr(out),
                                                 _lib.ptr(counts), _lib.stream_handle(dev))
    _lib.check(rc, "anerf_background_median")
    return (out, counts) if return_counts else out


# ---------------------------------------------------------------- the dataset end
def prepare_dataset(data, *, extend_iter=2, kernel=5, erode_border=False, kp_masks=False, kp2ds=None, bkgd=None,
                    cam_idxs=None, device=None):
    """A new mapping that RayImageDataset accepts: the keys of `data` (imgs (N, H*W, 3) uint8, masks (N, H*W, 1),
    img_shape, c2ws, focals, kp3d, ...) plus
      sampling_masks (N, H*W, 1): with kp_masks the key point masks first (create_kp_masks' defaults, from kp2ds or
        from kp3d projected through c2ws, focals and centers), then `sampling_masks(extend_iter, kernel, erode_border)`;
      bkgds (C, H, W, 3) and bkgd_idxs (N,) with bkgd = "median" (every frame of a camera) or "masked_median" (the
        frames whose `masks` byte is 0 at the pixel); cam_idxs (N,) names each image's camera (default: one camera).
    The masks (and, for bkgd, the images) are uploaded once and each result is read back once: the sampler draws its
    pixels on the host."""
    if bkgd not in (None, "median", "masked_median"):
        raise ValueError('bkgd must be None, "median" or "masked_median"')
    dev = _dev(None, device)
    out = {k: data[k] for k in data.keys()}
    shape = np.asarray(data["img_shape"][:])
    H, W = int(shape[1]), int(shape[2])
    masks = _u8(np.asarray(data["masks"][:]), dev).reshape(-1, H, W)
    n = int(masks.shape[0])
    m = masks
    if kp_masks:
        if kp2ds is None:
            centers = np.asarray(data["centers"][:]) if "centers" in data.keys() else None
            kp2ds = skeleton3d_to_2d(np.asarray(data["kp3d"][:]), np.asarray(data["c2ws"][:]), H, W,
                                     np.asarray(data["focals"][:]), centers, dev)
        m = create_kp_masks(m, kp2ds=kp2ds, device=dev)
    sm = sampling_masks(m, extend_iter, kernel, erode_border, device=dev)
    out["sampling_masks"] = sm.cpu().numpy().reshape(n, H * W, 1)
    if bkgd is not None:
        cam = np.zeros(n, np.int64) if cam_idxs is None else np.asarray(host(cam_idxs)).reshape(-1).astype(np.int64)
        imgs = _u8(np.asarray(data["imgs"][:]), dev).reshape(n, H * W, 3)
        bg = median_backgrounds(imgs, cam, masks if bkgd == "masked_median" else None, H=H, W=W, device=dev)
        out["bkgds"] = bg.cpu().numpy()
        out["bkgd_idxs"] = cam
    return out


# ---------------------------------------------------------------- NumPy checkers
def _window(a, radius, axis, fn):
    """fn (np.maximum / np.minimum) over [i - radius, i + radius] cut to the axis, along `axis` of a."""
    out = a.copy()
    n = a.shape[axis]
    for d in range(1, min(int(radius), n - 1) + 1):
        head, tail = [slice(None)] * a.ndim, [slice(None)] * a.ndim
        head[axis], tail[axis] = slice(0, n - d), slice(d, n)
        head, tail = tuple(head), tuple(tail)
        out[tail] = fn(out[tail], a[head])
        out[head] = fn(out[head], a[tail])
    return out


def mask_morph_reference(masks, op, radius, band=0, other=None, H=None, W=None):
    """anerf_mask_morph in NumPy: rows then columns, the window cut to the mask."""
    src = np.asarray(masks)
    src = src.astype(np.uint8) if src.dtype == np.bool_ else src
    planes = src.reshape(_mask_planes(src.shape, H, W))
    fn = {"dilate": np.maximum, "erode": np.minimum}[op]
    out = _window(_window(planes, radius, 2, fn), radius, 1, fn)
    if band > 0:
        hi = _window(_window(planes, band, 2, np.maximum), band, 1, np.maximum)
        lo = _window(_window(planes, band, 2, np.minimum), band, 1, np.minimum)
        out[(hi - lo).astype(np.uint8) == 1] = 0
    if other is not None:
        out = ((out != 0) | (np.asarray(other).reshape(planes.shape) != 0)).astype(np.uint8)
    return out.reshape(src.shape)


def morph_iterated_reference(masks, op, kernel, iterations, H=None, W=None):
    """`iterations` passes of the kernel x kernel window, one after the other (what cv2's `iterations` means)."""
    out = np.asarray(masks)
    for _ in range(int(iterations)):
        out = mask_morph_reference(out, op, (int(kernel) - 1) // 2, H=H, W=W)
    return out.copy() if iterations == 0 else out


def dilate_masks_reference(masks, extend_iter=1, kernel=5, H=None, W=None):
    return mask_morph_reference(masks, "dilate", fold_radius(kernel, extend_iter), H=H, W=W)


def erode_masks_reference(masks, extend_iter=1, kernel=5, H=None, W=None):
    return mask_morph_reference(masks, "erode", fold_radius(kernel, extend_iter), H=H, W=W)


def sampling_masks_reference(masks, extend_iter=3, kernel=5, erode_border=False, H=None, W=None):
    band = (int(kernel) - 1) // 2 if erode_border else 0
    return mask_morph_reference(masks, "dilate", fold_radius(kernel, extend_iter), band=band, H=H, W=W)


def draw_segments_reference(segs, H, W, width=3, colors=None, frames=None):
    """anerf_draw_segments in NumPy int64: the segments of a frame in index order, each over its own bounding box, a
    later one painting over an earlier one.  -> the (F, H, W) mask, or the painted copy of frames."""
    segs = np.asarray(segs, dtype=np.int64)
    F_ = segs.shape[0]
    mask = np.zeros((F_, H, W), np.uint8)
    out = None if frames is None else np.array(frames, dtype=np.uint8, copy=True)
    w2, half = int(width) ** 2, (int(width) + 1) // 2
    for f in range(F_):
        for b, (px, py, qx, qy) in enumerate(segs[f]):
            if max(abs(px), abs(py), abs(qx), abs(qy)) > MAX_COORD:
                continue
            x0, x1 = max(0, min(px, qx) - half), min(W - 1, max(px, qx) + half)
            y0, y1 = max(0, min(py, qy) - half), min(H - 1, max(py, qy) + half)
            if x0 > x1 or y0 > y1:
                continue
            cy, cx = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
            dx, dy, ex, ey = qx - px, qy - py, cx - px, cy - py
            t, dd = ex * dx + ey * dy, dx * dx + dy * dy
            cov = np.where(t <= 0, 4 * (ex * ex + ey * ey) <= w2,
                           np.where(t >= dd, 4 * ((cx - qx) ** 2 + (cy - qy) ** 2) <= w2,
                                    4 * (dx * ey - dy * ex) ** 2 <= w2 * dd))
            mask[f, y0:y1 + 1, x0:x1 + 1] |= cov.astype(np.uint8)
            if out is not None:
                out[f, y0:y1 + 1, x0:x1 + 1][cov] = np.asarray(colors, np.uint8)[b]
    return mask if frames is None else out


def skeleton_segments_reference(kp2ds, skel_type=SMPLSkeleton):
    j = np.asarray(host(kp2ds))
    j = j if j.dtype.kind == "f" else j.astype(np.float64)
    parents = np.asarray(skel_type.joint_trees, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        e = np.concatenate([np.round(j), np.round(j + (j[:, parents] - j))], axis=-1)
        ok = np.isfinite(e) & (np.abs(e) <= MAX_COORD)
    return np.where(ok, e, _DROPPED).astype(np.int32)


def skeleton3d_to_2d_reference(kps, c2ws, H, W, focals, centers=None):
    """skeleton3d_to_2d in NumPy float64, through the full 4 x 4 inverse."""
    p = np.asarray(host(kps), dtype=np.float64)
    n = p.shape[0]
    c = np.asarray(host(c2ws), dtype=np.float64).reshape(n, 4, 4)
    ext = np.linalg.inv(c * np.array([1.0, -1.0, -1.0, 1.0]))
    ph = np.concatenate([p, np.ones(p.shape[:2] + (1,))], axis=-1)
    f = _focal_pairs(focals, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        cam = np.einsum("fnj,fij->fni", ph, ext)
        uv = cam[..., :2] * f[:, None, :] / cam[..., 2:3]
    uv[uv == np.inf] = 0.0
    if centers is None:
        off = np.stack([_per_frame(W, n, "W") * 0.5, _per_frame(H, n, "H") * 0.5], axis=1)
    else:
        off = np.asarray(host(centers), dtype=np.float64).reshape(n, 2)
    return uv + off[:, None, :]


def draw_skeletons_reference(imgs, skels, skel_type=SMPLSkeleton, width=3, flip=False):
    imgs = np.asarray(host(imgs))
    return draw_segments_reference(skeleton_segments_reference(skels, skel_type), imgs.shape[1], imgs.shape[2], width,
                                   skeleton_colors(skel_type, flip), imgs)


def draw_skeletons_3d_reference(imgs, skels, c2ws, H, W, focals, centers=None, width=3, flip=False,
                                skel_type=SMPLSkeleton):
    return draw_skeletons_reference(imgs, skeleton3d_to_2d_reference(skels, c2ws, H, W, focals, centers), skel_type,
                                    width, flip)


def create_kp_masks_reference(masks, kp2ds=None, kp3ds=None, c2ws=None, hwf=None, extend_iter=3,
                              skel_type=SMPLSkeleton):
    m = np.asarray(host(masks))
    n, h, w = _mask_planes(m.shape)
    if kp2ds is None:
        kp2ds = skeleton3d_to_2d_reference(kp3ds, c2ws, hwf[0], hwf[1], hwf[2])
    drawn = draw_segments_reference(skeleton_segments_reference(kp2ds, skel_type), h, w, 3)
    return mask_morph_reference(drawn, "dilate", fold_radius(5, extend_iter), other=m).reshape(m.shape)


def median_backgrounds_reference(imgs, cam_idxs, masks=None, n_cams=None, H=None, W=None, return_counts=False,
                                 chunk=1 << 15):
    """anerf_background_median in NumPy, vectorised: per camera the frames' values sorted with the masked ones last,
    then floor((v[(n - 1) // 2] + v[n // 2]) / 2) of the n taken, `chunk` pixels at a time."""
    src = np.asarray(host(imgs))
    n, h, w = _image_rows(src.shape, H, W)
    src = src.reshape(n, h * w, 3)
    m = None if masks is None else np.asarray(host(masks)).reshape(n, h * w)
    order, start = camera_lists(cam_idxs, n_cams)
    C = len(start) - 1
    out = np.zeros((C, h * w, 3), np.uint8)
    counts = np.zeros((C, h * w), np.int32)
    for c in range(C):
        idx = order[start[c]:start[c + 1]]
        if len(idx) == 0:
            continue
        for p0 in range(0, h * w, chunk):
            vals = src[idx, p0:p0 + chunk].astype(np.int16)
            taken = np.ones(vals.shape[:2], bool) if m is None else m[idx, p0:p0 + chunk] == 0
            vals = np.sort(np.where(taken[..., None], vals, 256), axis=0)
            k = taken.sum(0)
            lo = np.take_along_axis(vals, np.maximum(k - 1, 0)[None, :, None] // 2, axis=0)[0]
            hi = np.take_along_axis(vals, np.minimum(k // 2, len(idx) - 1)[None, :, None], axis=0)[0]
            out[c, p0:p0 + chunk] = np.where(k[:, None] > 0, (lo + hi) // 2, 0).astype(np.uint8)
            counts[c, p0:p0 + chunk] = k
    out, counts = out.reshape(C, h, w, 3), counts.reshape(C, h, w)
    return (out, counts) if return_counts else out


__all__ = ["MAX_RADIUS", "MAX_COORD", "MAX_CAMERA_FRAMES", "fold_radius", "mask_morph", "dilate_masks", "erode_masks",
           "sampling_masks", "skeleton_type_of", "skeleton_colors", "skeleton_segments", "draw_segments",
           "skeleton3d_to_2d", "draw_skeleton2d", "draw_skeletons", "draw_skeletons_3d", "create_kp_masks",
           "create_kp_mask", "camera_lists", "median_backgrounds", "prepare_dataset", "mask_morph_reference",
           "morph_iterated_reference", "dilate_masks_reference", "erode_masks_reference", "sampling_masks_reference",
           "draw_segments_reference", "skeleton_segments_reference", "skeleton3d_to_2d_reference",
           "draw_skeletons_reference", "draw_skeletons_3d_reference", "create_kp_masks_reference",
           "median_backgrounds_reference"]

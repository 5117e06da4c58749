"""Shared cases and independent restatements for the dataset-preparation tests (tests/test_prep_host.py,
tests/test_gpu_prep.py) and tools/prep_bench.py: masks, segments, skeletons, camera frame lists, the raw dataset."""
import importlib
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
syn = importlib.import_module("a-nerf_amd.synthetic")


# ---------------------------------------------------------------- masks
def mask_stack(H, W, seed, binary):
    """N = 3 masks of H x W: blobs (or random bytes), the four corner pixels, and a stripe pattern."""
    rs = np.random.RandomState(seed)
    a = (rs.uniform(size=(H, W)) < 0.08).astype(np.uint8) if binary else rs.randint(0, 256, (H, W)).astype(np.uint8)
    b = np.zeros((H, W), np.uint8)
    b[0, 0] = b[0, W - 1] = b[H - 1, 0] = b[H - 1, W - 1] = 1 if binary else 200
    c = np.zeros((H, W), np.uint8)
    c[H // 3:H // 3 + max(1, H // 4), W // 4:W // 4 + max(1, W // 2)] = 1 if binary else 77
    c[:, W // 2] = 1 if binary else 255
    return np.stack([a, b, c])


def morph_scipy(masks, op, kernel, iterations):
    """cv2.dilate / cv2.erode with a kernel x kernel all-ones element, `iterations` times, border ignored:
    scipy.ndimage's grey morphology with constant borders of 0 (dilate) / 255 (erode), iterated."""
    from scipy import ndimage
    fn, cval = (ndimage.grey_dilation, 0) if op == "dilate" else (ndimage.grey_erosion, 255)
    out = []
    for m in np.asarray(masks):
        for _ in range(iterations):
            m = fn(m, size=(kernel, kernel), mode="constant", cval=cval)
        out.append(m)
    return np.stack(out)


def get_mask_scipy(mask, erode_border):
    """The tail of load_zju.py's get_mask on one mask, its three lines restated with scipy."""
    sampling = morph_scipy(mask[None], "dilate", 5, 3)[0].copy()
    if erode_border:
        dilated = morph_scipy(mask[None], "dilate", 5, 1)[0]
        eroded = morph_scipy(mask[None], "erode", 5, 1)[0]
        sampling[(dilated - eroded) == 1] = 0
    return sampling


# ---------------------------------------------------------------- segments
def segment_frames(H, W):
    """(3, 12, 4) int32: horizontal, vertical, 45 degrees, shallow, zero-length, crossing each edge, wholly outside,
    an overlapping pair; frame 2 repeats frame 0 with one endpoint at +-8193 (that segment is dropped)."""
    f0 = [[5, 4, 40, 4], [9, 2, 9, 30], [12, 8, 32, 28], [3, 20, 66, 25], [50, 10, 50, 10], [-6, 12, 8, 18],
          [60, 30, 80, 44], [30, -5, 34, 6], [-40, -40, -20, -30], [200, 10, 300, 10], [20, 14, 45, 14],
          [30, 6, 30, 24]]
    f1 = [[W - 1 - a, H - 1 - b, W - 1 - c, H - 1 - d] for a, b, c, d in f0]
    f2 = [list(s) for s in f0]
    f2[3] = [3, 20, 8193, 25]
    f2[1] = [9, -8193, 9, 30]
    return np.array([f0, f1, f2], np.int32)


def coverage_brute(seg, H, W, width):
    """(H, W) bool: is the pixel centre within width / 2 of the closed segment?  The closest point by a clamped
    projection in exact fractions -- no case split, no cross product."""
    px, py, qx, qy = (int(v) for v in seg)
    dx, dy = qx - px, qy - py
    out = np.zeros((H, W), bool)
    lim = Fraction(width * width, 4)
    for y in range(H):
        for x in range(W):
            t = Fraction(0)
            if dx or dy:
                t = min(Fraction(1), max(Fraction(0), Fraction((x - px) * dx + (y - py) * dy, dx * dx + dy * dy)))
            ex, ey = x - (px + t * dx), y - (py + t * dy)
            out[y, x] = ex * ex + ey * ey <= lim
    return out


def skeleton_scene(n_joints, F_, H, W, seed):
    """kps (F, NJ, 3), c2ws (F, 4, 4), per-frame (fx, fy) focals (F, 2), centers (F, 2): a synthetic skeleton seen by
    orbiting cameras, zoomed so that it fills the frame and some joints leave it.  kps and c2ws are float64 (float32
    values widened): the frame loop below computes in the precision of what it is given."""
    sc = syn.make_scene(n_joints=24, H=H, W=W, seed=seed, n_frames=F_, yaw_step=0.7)
    rs = np.random.RandomState(seed)
    # a 17-joint skeleton: the first 17 points, joined by its own tree; moved off the optical axis, where the pelvis
    # would project onto the half-pixel (W / 2, H / 2) exactly
    sc["kps"] = sc["kps"][:, :n_joints] + rs.uniform(-0.05, 0.05, 3).astype(np.float32)
    focals = np.stack([rs.uniform(3.0, 4.5, F_) * H, rs.uniform(3.0, 4.5, F_) * H], axis=1).astype(np.float32)
    centers = (np.array([W / 2, H / 2]) + rs.uniform(-3, 3, (F_, 2))).astype(np.float32)
    return sc["kps"].astype(np.float64), sc["c2ws"].astype(np.float64), focals, centers


def project_loop(kps, c2ws, H, W, focals, centers=None):
    """skeleton3d_to_2d frame by frame as the reference composes it: the inverse of the camera with its y and z
    columns negated, the float32 pinhole matrix, the division, +inf to 0, the offset."""
    out = []
    for i, (kp, c2w) in enumerate(zip(np.asarray(kps), np.asarray(c2ws))):
        flip = np.concatenate([c2w[..., 0:1], -c2w[..., 1:2], -c2w[..., 2:3], c2w[..., 3:]], axis=-1)
        ext = np.linalg.inv(flip)
        f = focals if isinstance(focals, float) else focals[i]
        fx, fy = (f, f) if np.size(f) < 2 else f
        K = np.array([[fx, 0, 0, 0], [0, fy, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
        pts = np.concatenate([kp, np.ones_like(kp[..., :1])], axis=-1)
        cam = pts @ ext.T @ K.T
        cam = cam[..., :2] / cam[..., 2:3]
        cam[cam == np.inf] = 0.
        ox, oy = ((W if isinstance(W, int) else W[i]) * .5, (H if isinstance(H, int) else H[i]) * .5) \
            if centers is None else centers[i]
        cam[..., 0] += ox
        cam[..., 1] += oy
        out.append(cam)
    return np.array(out)


# ---------------------------------------------------------------- medians
def median_frames(n, H, W, seed, extremes=True):
    """imgs (n, H*W, 3) bytes with 0 and 255 present and neighbouring values of odd sum, masks (n, H*W) that leave
    pixels with 0, 1 and an even number of clear frames."""
    rs = np.random.RandomState(seed)
    imgs = rs.randint(0, 256, (n, H * W, 3)).astype(np.uint8)
    if extremes:
        imgs[:, 0] = 0
        imgs[:, 1] = 255
        imgs[::2, 2] = 10   # pairs (10, 11): an odd sum, the floor of 10.5
        imgs[1::2, 2] = 11
        imgs[::2, 3] = 0    # (0, 255) -> 127
        imgs[1::2, 3] = 255
    masks = (rs.uniform(size=(n, H * W)) < 0.4).astype(np.uint8)
    masks[:, 4] = 1                 # no clear frame
    masks[:, 5] = 1
    masks[n - 1, 5] = 0             # one clear frame
    masks[:, 6] = 0                 # every frame
    if n >= 2:
        masks[:, 7] = 1
        masks[:2, 7] = 0            # two clear frames
    return imgs, masks


def median_loop(imgs, masks, cam_idxs, n_cams, H, W):
    """load_zju.py's backgrounds, pixel by pixel: np.median over the frames whose mask is below 1, zeros where none."""
    imgs, masks, cam_idxs = np.asarray(imgs), np.asarray(masks), np.asarray(cam_idxs)
    bk = np.zeros((n_cams, H, W, 3), dtype=np.uint8)
    for c in np.unique(cam_idxs):
        ci = imgs[cam_idxs == c].reshape(-1, H, W, 3)
        cm = masks[cam_idxs == c].reshape(-1, H, W, 1)
        for h in range(H):
            for w in range(W):
                clear = np.where(cm[:, h, w] < 1)[0]
                med = np.zeros(3) if len(clear) == 0 else np.median(ci[clear, h, w], axis=0)
                bk[c, h, w] = med.astype(np.uint8)
    return bk


# ---------------------------------------------------------------- the raw dataset
def raw_dataset():
    """The `plain` case of tests/golden/raybatch.npz (5 images of 24 x 32, what tests/test_gpu_dataset.py feeds
    RayImageDataset) without its sampling masks, with blob masks so that dilation has work to do, plus cam_idxs."""
    G = np.load(os.path.join(HERE, "golden", "raybatch.npz"))
    data = {k.split("/", 2)[2]: np.array(G[k]) for k in G.files if k.startswith("plain/in/")}
    del data["sampling_masks"]
    H, W = int(data["img_shape"][1]), int(data["img_shape"][2])
    n = len(data["imgs"])
    masks = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        masks[i, 6 + i:14 + i, 10 + 2 * i:17 + 2 * i] = 1
    data["masks"] = masks.reshape(n, H * W, 1)
    return data, np.array([0, 1, 0, 1, 0]), H, W

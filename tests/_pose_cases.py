"""Seeded pose pairs for the pose-score tests, the golden generator (tests/golden/make_pose_golden.py) and
tools/pose_bench.py.

Every array is float64 holding float32-representable values, so that the float32 reference modules and the float64
checker read the same numbers.  gt is in millimetres around a centroid a few metres from the origin, pred an (inexact)
similarity transform of it; `unit` = 1000 gives pred in metres, the reference's pairing."""
import numpy as np

SPREAD = np.array([220.0, 450.0, 160.0])  # a standing body's extent per axis, millimetres
CENTRE = np.array([350.0, -900.0, 2600.0])


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def rotation(rs, mirror=False):
    q, r = np.linalg.qr(rs.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if (np.linalg.det(q) < 0) != mirror:
        q[:, 2] *= -1
    return q


def body(rs, F, J):
    """Generic 3-D joints: no plane, no line."""
    return rs.normal(size=(F, J, 3)) * SPREAD + CENTRE + rs.normal(size=(F, 1, 3)) * 300.0


def transformed(rs, gt, noise=0.0, mirror=False, unit=1.0):
    """pred with gt = b pred T + c up to `noise` (millimetres) -> (pred, b [F], T [F][3][3], c [F][3])."""
    F = gt.shape[0]
    T = np.stack([rotation(rs, mirror) for _ in range(F)])
    b = rs.uniform(0.6, 1.6, size=F)
    c = rs.normal(size=(F, 3)) * 400.0
    pred = np.einsum("fjk,flk->fjl", (gt - c[:, None]) / b[:, None, None], T)  # (gt - c) / b @ T^T
    pred = pred + rs.normal(size=gt.shape) * noise / b[:, None, None]
    return pred / unit, b * unit, T, c


def make_pair(kind, F, J, seed, noise=35.0, unit=1.0):
    """-> (pred, gt) float64 [F][J][3].  kind: 'body' (generic, well conditioned), 'exact' (noise 0), 'mirrored'
    (pred a reflected copy), 'planar_gt', 'collinear_gt', 'both_planar' (flat exactly), 'planar_exact'
    (small integers with z = 7: rank 2 exactly), 'equal' (all joints of gt equal)."""
    rs = np.random.default_rng(seed)
    gt = body(rs, F, J)
    # the flat cases are flat exactly, in float32 too: a plane z = const, a line along x
    if kind in ("planar_gt", "both_planar"):
        gt = rs.normal(size=(F, J, 3)) * SPREAD * np.array([1.0, 1.0, 0.0]) + CENTRE
    if kind == "collinear_gt":
        gt = rs.normal(size=(F, J, 3)) * np.array([300.0, 0.0, 0.0]) + CENTRE
    if kind == "both_planar":  # pred a turn about z of gt, with noise inside its own plane z = 0.5
        th = rs.uniform(0, 2 * np.pi, size=F)
        R = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], 1)
        xy = np.einsum("fjk,flk->fjl", gt[..., :2] - CENTRE[:2], R) / 1.3 + rs.normal(size=(F, J, 2)) * noise
        return _f32(np.concatenate([xy, np.full((F, J, 1), 0.5)], -1) / unit), _f32(gt)
    if kind == "planar_exact":
        gt = np.concatenate([rs.integers(-40, 40, size=(F, J, 2)), np.full((F, J, 1), 7)], axis=-1).astype(np.float64)
        pred = gt[..., [1, 0, 2]] * np.array([1.0, -1.0, 1.0]) * 0.5 + 3.0  # a quarter turn about z, half size
        pred[..., :2] += rs.integers(-2, 3, size=(F, J, 2))
        return _f32(pred / unit), _f32(gt)
    if kind == "equal":
        gt = np.repeat(gt[:, :1], J, axis=1)
    pred = transformed(rs, gt, 0.0 if kind == "exact" else noise, kind == "mirrored", unit)[0]
    return _f32(pred), _f32(gt)


# the golden fixture's cases: name -> (kind, F, J, seed)
GOLDEN_CASES = {
    "body24": ("body", 4, 24, 101),
    "body17": ("body", 3, 17, 102),
    "mirrored": ("mirrored", 2, 24, 103),
    "j2": ("body", 2, 2, 104),
    "j3": ("body", 2, 3, 105),
    "planar_gt": ("planar_gt", 2, 24, 106),
    "collinear_gt": ("collinear_gt", 2, 8, 107),
    "both_planar": ("both_planar", 2, 12, 108),
}
WELL_CONDITIONED = ("body24", "body17", "mirrored")  # Z and T are compared on these alone
RANK_DEFICIENT = ("j2", "j3", "planar_gt", "collinear_gt", "both_planar")
PAMPJPE_CASE = ("body", 3, 17, 131)  # evaluate_pampjpe's: 17 joints, root 14, pred in metres
SUBSET_14 = [16, 2, 14, 5, 11, 1, 8, 3, 13, 6, 10, 4, 15, 12]  # 14 of 17 joints, not in order, joint 14 among them
COMBOS = [(s, r) for s in (True, False) for r in ("best", False, True)]


def golden_pair(name):
    kind, F, J, seed = GOLDEN_CASES[name]
    return make_pair(kind, F, J, seed)


def pampjpe_pair():
    kind, F, J, seed = PAMPJPE_CASE
    return make_pair(kind, F, J, seed, noise=45.0, unit=1000.0)


def combo_key(name, scaling, reflection):
    return f"a_{name}_s{int(scaling)}_r{reflection}"

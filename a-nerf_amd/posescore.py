"""Scoring of refined skeleton poses: MPJPE, PA-MPJPE, PCK and AUC on the device, and the reference's entry points.

  * `evaluate_poses` -- anerf_pose_scores (csrc/anerf_posescore.hip): every frame's MPJPE, root-centred MPJPE,
    least-squares-scaled MPJPE and Procrustes-aligned PA-MPJPE in double, their means over the frames, per-joint means
    and the PCK curve, from one call and one device read of 520 numbers whatever the frame count.
  * `evaluate_poses_reference` -- the same in float64 NumPy on the host (np.linalg.svd): the checker.
  * `procrustes_align`, `procrustes`, `Criterion_MPJPE`, `Criterion3DPose_ProcrustesCorrected`,
    `Criterion3DPose_leastQuaresScaled`, `evaluate_pampjpe` -- core/utils/evaluation_helpers.py:387-603 over the kernel.
  * `evaluate_pose_layer`, `evaluate_pose_ckpt`, `Trainer.evaluate_poses` -- score a PoseOptLayer's joints where its
    kinematic chain left them, and a `Trainer.save_popt` checkpoint before and after the refinement.

The fit is the reference's procrustes(X = gt, Y = pred): Z = b Y T + c with T = V U^T from A = X0^T Y0 = U S V^T.
`reflection` is 'best' (the reference's default: det T = -1 is allowed), False (Kabsch / Umeyama, what most published
PA-MPJPE numbers use) or True.  Rules the reference does not have, the same in the kernel and in the checker:

  * T is always orthogonal.  Where A has rank 2 or 1 (three joints, planar or collinear poses: singular values
    <= 1e-12 of the largest) the missing left singular vectors are completed by cross products to det T = +1 (-1 under
    reflection=True).  The scores do not depend on the completion; Z and T do.
  * A frame without a scored joint, or whose centred sum of squares on either side is <= 1e-26 of the uncentred one
    (one joint, all joints equal), has no fit: NaN in its fitted fields, and the means leave it out (the reference
    divides by zero there).  mpjpe_root and n_mpjpe are NaN where the root joint is not valid, and their means are over
    the frames where they are not.

Not covered: the SMPL-vertex joint regressor of evaluate_pampjpe_from_smpl_params (it needs smpl/SMPL_NEUTRAL.pkl and
J_regressor_h36m.npy: pass the joints to `evaluate_pampjpe`), 2-D reprojection error, gradients through the alignment.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

FRAME_COLUMNS = ("n", "mpjpe", "mpjpe_root", "n_mpjpe", "pa_mpjpe", "d", "b", "s0", "s1", "s2",
                 "T00", "T01", "T02", "T10", "T11", "T12", "T20", "T21", "T22", "c0", "c1", "c2",
                 "norm_gt", "norm_pred", "s_opt")
COL = {name: i for i, name in enumerate(FRAME_COLUMNS)}
RANK_TOL, ZERO_SS = 1e-12, 1e-26
MAXJ, MAXT = _lib.ANERF_POSE_MAX_JOINTS, _lib.ANERF_POSE_MAX_THRESHOLDS
_T_JOINT, _T_COUNT = 8, 8 + 3 * MAXJ
AUC_THRESHOLDS = np.linspace(0.0, 150.0, 31)  # evaluation_helpers.py:597


@dataclass
class PoseScores:
    """Means over the frames with a fit (n_scored of n_frames), in the unit pred_scale / gt_scale bring the joints to.
    pck: the share of scored (frame, joint) pairs with pa_err < pck_threshold; pck_curve the same at `thresholds` and
    auc its mean (the reference's numbers when thresholds is its linspace(0, 150, 31)); pck_counts [2][T + 1] the
    integer counts for pa_err and for err (last column: pck_threshold) of n_pairs.  per_joint_*: means per scored
    joint, in the order of `joints`.  per_frame [F][25] float64 (columns FRAME_COLUMNS, `column(name)`), aligned
    [F][J][3] fp32, err / pa_err [F][J] float64: when asked, device tensors from evaluate_poses and arrays from the
    checker."""
    mpjpe: float
    mpjpe_root: float
    n_mpjpe: float
    pa_mpjpe: float
    pck: float
    auc: float
    thresholds: np.ndarray
    pck_curve: np.ndarray
    per_joint_mpjpe: np.ndarray
    per_joint_pa_mpjpe: np.ndarray
    n_frames: int
    n_scored: int
    n_pairs: int = 0
    pck_counts: np.ndarray = None
    joints: np.ndarray = None
    per_frame: object = None
    aligned: object = None
    err: object = None
    pa_err: object = None

    def column(self, name):
        """A named column of per_frame; 'T' the [F][3][3] rotations, 'c' the [F][3] translations, 's' the singular
        values."""
        if self.per_frame is None:
            raise ValueError("per_frame was not asked for")
        if name == "T":
            return self.per_frame[:, COL["T00"]:COL["T00"] + 9].reshape(-1, 3, 3)
        if name == "c":
            return self.per_frame[:, COL["c0"]:COL["c0"] + 3]
        if name == "s":
            return self.per_frame[:, COL["s0"]:COL["s0"] + 3]
        return self.per_frame[:, COL[name]]


def _reflection_flag(reflection):
    if isinstance(reflection, str):
        if reflection != "best":
            raise ValueError(f"reflection must be 'best', False or True, got {reflection!r}")
        return 0
    return _lib.ANERF_POSE_REFLECT_TRUE if reflection else _lib.ANERF_POSE_REFLECT_FALSE


def _thresholds(thresholds, pck_threshold):
    th = AUC_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64).reshape(-1)
    if len(th) + 1 > MAXT:
        raise ValueError(f"at most {MAXT - 1} thresholds (pck_threshold takes the last slot), got {len(th)}")
    return th, np.ascontiguousarray(np.concatenate([th, [float(pck_threshold)]]))


def _joints(joints, J):
    if joints is None:
        return np.arange(J, dtype=np.int32)
    j = np.ascontiguousarray(np.asarray(joints).reshape(-1), dtype=np.int32)
    if j.size and (j.min() < 0 or j.max() >= J):
        raise ValueError(f"joints must lie in [0, {J})")
    if len(np.unique(j)) != len(j):
        raise ValueError("joints must not repeat")
    return j


def _from_totals(tot_f, tot_i, jidx, th, F):
    """PoseScores from the totals' layout (include/anerf.h ANERF_POSE_TOTALS): tot_f the words as float64, tot_i the
    same words as int64."""
    with np.errstate(divide="ignore", invalid="ignore"):
        n_scored, n_root, n_nm = tot_f[0], tot_f[1], tot_f[2]
        jc = tot_f[_T_JOINT + 2 * MAXJ + jidx]
        pairs = tot_f[_T_JOINT + 2 * MAXJ:_T_COUNT].sum()
        counts = np.stack([tot_i[_T_COUNT:_T_COUNT + len(th) + 1], tot_i[_T_COUNT + MAXT:_T_COUNT + MAXT + len(th) + 1]])
        curve = counts[0, :-1] / pairs
        return PoseScores(
            mpjpe=float(tot_f[3] / n_scored), mpjpe_root=float(tot_f[4] / n_root), n_mpjpe=float(tot_f[5] / n_nm),
            pa_mpjpe=float(tot_f[6] / n_scored), pck=float(counts[0, -1] / pairs),
            auc=float(np.mean(curve)) if len(th) else float("nan"), thresholds=th.copy(), pck_curve=curve,
            per_joint_mpjpe=tot_f[_T_JOINT + jidx] / jc, per_joint_pa_mpjpe=tot_f[_T_JOINT + MAXJ + jidx] / jc,
            n_frames=int(F), n_scored=int(n_scored), n_pairs=int(pairs), pck_counts=counts.astype(np.int64),
            joints=jidx.copy())


def _empty(jidx, th):
    z = np.zeros(_lib.ANERF_POSE_TOTALS)
    return _from_totals(z, z.astype(np.int64), jidx, th, 0)


def _device_input(x, dev):
    """pred / gt as a contiguous fp32 or fp64 [F][J][3] tensor on `dev` (arrays are uploaded once; other dtypes become
    fp32, as the reference's FloatTensor)."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float32)
    return t.detach().to(dev).contiguous()


def _pick_device(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


@torch.no_grad()
def evaluate_poses(pred_kps, gt_kps, joints=None, valid=None, root=0, pred_scale=1.0, gt_scale=1.0, scaling=True,
                   reflection="best", thresholds=None, pck_threshold=150.0, per_frame=False, return_aligned=False,
                   return_errors=False):
    """Score pred_kps against gt_kps, both [F][J][3] (fp32 or fp64; device tensors stay where they are, arrays are
    uploaded once), on the device: one anerf_pose_scores call, one device read.  joints: the scored subset (a list of
    joint indices, each once); valid [F][J]: nonzero where a joint exists; root: the joint mpjpe_root and n_mpjpe subtract (None:
    none).  pred_scale / gt_scale bring both to one unit (the reference's pairing is pred in metres, 1000, against gt
    in millimetres, 1), which is the unit of the scores and of `thresholds` (default linspace(0, 150, 31)) and
    pck_threshold.  At most 63 thresholds: the kernel takes 64 and pck_threshold has the last slot.  At most 128
    joints.  -> PoseScores; per_frame / return_aligned / return_errors add device tensors."""
    dev = _pick_device(pred_kps, gt_kps, valid)
    pred, gt = _device_input(pred_kps, dev), _device_input(gt_kps, dev)
    if pred.dim() != 3 or pred.shape[-1] != 3 or tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"pred_kps and gt_kps must both be [F][J][3], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    F, J = int(pred.shape[0]), int(pred.shape[1])
    jidx = _joints(joints, J)
    th, th_all = _thresholds(thresholds, pck_threshold)
    vd = None
    if valid is not None:
        v = valid if torch.is_tensor(valid) else torch.from_numpy(np.ascontiguousarray(np.asarray(valid)))
        vd = (v.to(dev) != 0).to(torch.uint8).reshape(F, J).contiguous()
    flags = (_lib.ANERF_POSE_PRED_F64 if pred.dtype == torch.float64 else 0) \
        | (_lib.ANERF_POSE_GT_F64 if gt.dtype == torch.float64 else 0) \
        | (0 if scaling else _lib.ANERF_POSE_NO_SCALING) | _reflection_flag(reflection)
    need = _lib.workspace("anerf_pose_scores_workspace", F, J, len(th_all))
    if F == 0:
        out = _empty(jidx, th)
        if per_frame:
            out.per_frame = torch.zeros(0, len(FRAME_COLUMNS), device=dev, dtype=torch.float64)
        if return_aligned:
            out.aligned = torch.zeros(0, J, 3, device=dev, dtype=torch.float32)
        if return_errors:
            out.err = torch.zeros(0, J, device=dev, dtype=torch.float64)
            out.pa_err = torch.zeros(0, J, device=dev, dtype=torch.float64)
        return out
    ws = torch.empty(need // 8, device=dev, dtype=torch.float64)
    totals = torch.empty(_lib.ANERF_POSE_TOTALS, device=dev, dtype=torch.float64)
    rec = torch.empty(F, len(FRAME_COLUMNS), device=dev, dtype=torch.float64) if per_frame else None
    al = torch.empty(F, J, 3, device=dev, dtype=torch.float32) if return_aligned else None
    er = torch.empty(F, J, device=dev, dtype=torch.float64) if return_errors else None
    pe = torch.empty(F, J, device=dev, dtype=torch.float64) if return_errors else None
    with torch.cuda.device(dev):
        rc = _lib.load().anerf_pose_scores(
            _lib.ptr(pred), _lib.ptr(gt), F, J, None if joints is None else jidx.ctypes.data_as(_lib.c_i32p),
            len(jidx), _lib.ptr(vd), -1 if root is None else int(root), float(pred_scale), float(gt_scale), flags,
            th_all.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(th_all), _lib.ptr(totals), _lib.ptr(rec),
            _lib.ptr(er), _lib.ptr(pe), _lib.ptr(al), _lib.ptr(ws), need, _lib.stream_handle(dev))
    _lib.check(rc, "anerf_pose_scores")
    tot = totals.cpu().numpy()  # (the one device read)
    out = _from_totals(tot, tot.view(np.int64), jidx, th, F)
    out.per_frame, out.aligned, out.err, out.pa_err = rec, al, er, pe
    return out


def _perp(u):
    """Per row a unit vector orthogonal to the unit vector u: the axis of u's smallest component, less its part
    along u (the kernel's rule)."""
    a = np.abs(u)
    k = np.where((a[:, 0] <= a[:, 1]) & (a[:, 0] <= a[:, 2]), 0, np.where(a[:, 1] <= a[:, 2], 1, 2))
    e = np.eye(3)[k]
    w = e - u[np.arange(len(u)), k][:, None] * u
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def evaluate_poses_reference(pred_kps, gt_kps, joints=None, valid=None, root=0, pred_scale=1.0, gt_scale=1.0,
                             scaling=True, reflection="best", thresholds=None, pck_threshold=150.0, per_frame=False,
                             return_aligned=False, return_errors=False):
    """evaluate_poses in float64 NumPy on the host (the checker): np.linalg.svd per frame, the same rank-completion and
    NaN rules.  per_frame, aligned (float64, not rounded), err and pa_err are arrays."""
    refl = _reflection_flag(reflection)
    p = np.asarray(_lib.host_array(pred_kps))
    g = np.asarray(_lib.host_array(gt_kps))
    p = p.astype(np.float64 if p.dtype == np.float64 else np.float32).astype(np.float64) * float(pred_scale)
    g = g.astype(np.float64 if g.dtype == np.float64 else np.float32).astype(np.float64) * float(gt_scale)
    if p.ndim != 3 or p.shape[-1] != 3 or p.shape != g.shape:
        raise ValueError(f"pred_kps and gt_kps must both be [F][J][3], got {p.shape} and {g.shape}")
    F, J = p.shape[:2]
    jidx = _joints(joints, J)
    th, th_all = _thresholds(thresholds, pck_threshold)
    sel = np.zeros(J, bool)
    sel[jidx] = True
    vd = np.ones((F, J), bool) if valid is None else np.asarray(_lib.host_array(valid)).reshape(F, J) != 0
    on = vd & sel[None]
    m = on[..., None].astype(np.float64)
    nan = np.float64("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        n = on.sum(1).astype(np.float64)
        pz, gz = np.where(on[..., None], p, 0.0), np.where(on[..., None], g, 0.0)
        err = np.where(on, np.linalg.norm(p - g, axis=-1), 0.0)
        mpjpe = err.sum(1) / n
        if root is None:
            pr, gr, root_ok = np.zeros((F, 1, 3)), np.zeros((F, 1, 3)), np.ones(F, bool)
        else:
            pr, gr, root_ok = p[:, root:root + 1], g[:, root:root + 1], vd[:, root]
        yr, xr = np.where(on[..., None], p - pr, 0.0), np.where(on[..., None], g - gr, 0.0)
        mpjpe_root = np.where(root_ok, np.linalg.norm(yr - xr, axis=-1).sum(1) / n, nan)
        s_opt = np.where(root_ok, (yr * xr).sum((1, 2)) / (yr * yr).sum((1, 2)), nan)
        n_mpjpe = np.linalg.norm(s_opt[:, None, None] * yr - xr, axis=-1).sum(1) / n
        muY, muX = pz.sum(1) / n[:, None], gz.sum(1) / n[:, None]
        Y0, X0 = (p - muY[:, None]) * m, (g - muX[:, None]) * m
        Y0, X0 = np.where(on[..., None], Y0, 0.0), np.where(on[..., None], X0, 0.0)
        ssY, ssX = (Y0 ** 2).sum((1, 2)), (X0 ** 2).sum((1, 2))
        fit = (n > 0) & (ssY > ZERO_SS * (pz ** 2).sum((1, 2))) & (ssX > ZERO_SS * (gz ** 2).sum((1, 2)))
        normY, normX = np.sqrt(ssY), np.sqrt(ssX)
        A = np.einsum("fji,fjk->fik", X0 / np.where(fit, normX, 1.0)[:, None, None],
                      Y0 / np.where(fit, normY, 1.0)[:, None, None])
        A = np.where(fit[:, None, None], A, np.eye(3)[None])
        U, s, Vt = np.linalg.svd(A)
        V = Vt.transpose(0, 2, 1).copy()
        # rank completion: the missing columns of U by cross products to det U = det V; rank 0: U = V
        has0 = s[:, 0] > 0
        has1 = has0 & (s[:, 1] > RANK_TOL * s[:, 0])
        has2 = has1 & (s[:, 2] > RANK_TOL * s[:, 0])
        dv = np.where(np.linalg.det(V) < 0, -1.0, 1.0)
        u0 = U[:, :, 0]
        u1 = np.where(has1[:, None], U[:, :, 1], _perp(u0))
        x = np.cross(u0, u1)
        u2 = np.where(has2[:, None], U[:, :, 2], dv[:, None] * x / np.linalg.norm(x, axis=1, keepdims=True))
        U = np.where(has0[:, None, None], np.stack([u0, u1, u2], axis=2), V)
        T = V @ U.transpose(0, 2, 1)
        if refl:
            flip = (np.linalg.det(T) < 0) != (refl == _lib.ANERF_POSE_REFLECT_TRUE)
            V[flip, :, 2] *= -1
            s[flip, 2] *= -1
            T = V @ U.transpose(0, 2, 1)
        trace = s.sum(1)
        if scaling:
            b = trace * normX / normY
            d = 1 - trace ** 2
        else:
            b = np.ones(F)
            d = 1 + ssY / ssX - 2 * trace * normY / normX
        Z = b[:, None, None] * ((p - muY[:, None]) @ T) + muX[:, None]
        c = muX - b[:, None] * np.einsum("fi,fik->fk", muY, T)
        pa_err = np.where(on, np.linalg.norm(Z - g, axis=-1), 0.0)
        pa_mpjpe = pa_err.sum(1) / n
        bad = ~fit
        for v in (pa_mpjpe, d, b):
            v[bad] = nan
        s[bad], T[bad], c[bad], Z[bad] = nan, nan, nan, nan
        pa_err[bad[:, None] & on] = nan
        rec = np.concatenate([np.stack([n, mpjpe, mpjpe_root, n_mpjpe, pa_mpjpe, d, b], 1), s, T.reshape(F, 9), c,
                              np.stack([normX, normY, s_opt], 1)], axis=1)
        # the totals, in the kernel's layout
        tf = np.zeros(_lib.ANERF_POSE_TOTALS)
        ti = np.zeros(_lib.ANERF_POSE_TOTALS, np.int64)
        rooted, scaled = fit & ~np.isnan(mpjpe_root), fit & ~np.isnan(n_mpjpe)
        tf[0:3] = fit.sum(), rooted.sum(), scaled.sum()
        tf[3:7] = mpjpe[fit].sum(), mpjpe_root[rooted].sum(), n_mpjpe[scaled].sum(), pa_mpjpe[fit].sum()
        pair = on & fit[:, None]
        tf[_T_JOINT:_T_JOINT + J] = np.where(pair, err, 0.0).sum(0)
        tf[_T_JOINT + MAXJ:_T_JOINT + MAXJ + J] = np.where(pair, pa_err, 0.0).sum(0)
        tf[_T_JOINT + 2 * MAXJ:_T_JOINT + 2 * MAXJ + J] = pair.sum(0)
        for k, t in enumerate(th_all):
            ti[_T_COUNT + k] = (pa_err[pair] < t).sum()
            ti[_T_COUNT + MAXT + k] = (err[pair] < t).sum()
        out = _from_totals(tf, ti, jidx, th, F)
    if per_frame:
        out.per_frame = rec
    if return_aligned:
        out.aligned = Z
    if return_errors:
        out.err, out.pa_err = err, pa_err
    return out


@torch.no_grad()
def procrustes_align(pred, gt, scaling=True, reflection="best"):
    """Align pred [F][J][3] (or one [J][3] pose) onto gt on the device -> (aligned fp32 tensor of pred's shape,
    tform = {'rotation' [F][3][3], 'scale' [F], 'translation' [F][3], 'd' [F]} float64 device tensors), with
    aligned = scale * pred @ rotation + translation as the reference's tform."""
    one = (pred.dim() if torch.is_tensor(pred) else np.ndim(pred)) == 2
    if one:
        pred, gt = pred[None], gt[None]
    sc = evaluate_poses(pred, gt, root=None, scaling=scaling, reflection=reflection, per_frame=True,
                        return_aligned=True)
    tform = {"rotation": sc.column("T"), "scale": sc.column("b"), "translation": sc.column("c"), "d": sc.column("d")}
    if one:
        return sc.aligned[0], {k: v[0] for k, v in tform.items()}
    return sc.aligned, tform


def procrustes(X, Y, scaling=True, reflection="best"):
    """evaluation_helpers.py:387-467 for one frame of 3-D points, over the kernel: X [n][3] the target, Y [n][3] the
    points to transform -> d, Z, tform = {'rotation', 'scale', 'translation'} with Z = scale * Y @ rotation +
    translation (float64 arrays; Z is formed on the host from the kernel's double transform, not from its fp32
    output)."""
    Xh, Yh = np.asarray(_lib.host_array(X)), np.asarray(_lib.host_array(Y))
    if Xh.ndim != 2 or Xh.shape[1] != 3 or Xh.shape != Yh.shape:
        raise ValueError("procrustes here takes two [n][3] point sets")
    sc = evaluate_poses(Yh[None], Xh[None], root=None, scaling=scaling, reflection=reflection, per_frame=True)
    rec = sc.per_frame.cpu().numpy()[0]
    T, b, c = rec[COL["T00"]:COL["T00"] + 9].reshape(3, 3).copy(), rec[COL["b"]], rec[COL["c0"]:COL["c0"] + 3].copy()
    Z = b * (Yh.astype(np.float64) @ T) + c
    return rec[COL["d"]], Z, {"rotation": T, "scale": b, "translation": c}


def _reduce(plane, reduction):
    if reduction == "mean":
        return plane.mean()
    if reduction == "sum":
        return plane.sum()
    return plane


def _batch(x):
    """[..., J, 3] -> ([B][J][3], the leading shape)."""
    return x.reshape(-1, x.shape[-2], 3), tuple(x.shape[:-1])


class Criterion_MPJPE(torch.nn.Module):
    """evaluation_helpers.py:469-483: |pred - label| per joint over the kernel's error plane, reduced by `reduction`
    ('mean', 'sum', anything else: none) -> a tensor of pred's dtype on the device.  It goes through
    anerf_pose_scores (which fits every frame on its way), so unlike the reference's module it takes [..., J, 3] with
    J <= 128 only: other last dimensions or more joints raise."""

    def __init__(self, reduction="mean"):
        super().__init__()
        self.reduction = reduction

    @torch.no_grad()
    def forward(self, pred_batch, label_batch):
        pred_batch, label_batch = torch.broadcast_tensors(pred_batch, label_batch.to(pred_batch.device))
        p, lead = _batch(pred_batch)
        l, _ = _batch(label_batch)
        sc = evaluate_poses(p, l, root=None, return_errors=True)
        return _reduce(sc.err.reshape(lead), self.reduction).to(pred_batch.device, pred_batch.dtype)


class Criterion3DPose_ProcrustesCorrected(torch.nn.Module):
    """evaluation_helpers.py:485-504: align every pose of pred_batch [B][J][3] onto label_batch with `procrustes`'
    defaults, then apply `criterion` -> (criterion(aligned, label), aligned).  With a Criterion_MPJPE the errors are
    the kernel's own double plane |Z - label| (the aligned joints are not rounded first); any other criterion is
    called on the aligned tensor."""

    def __init__(self, criterion):
        super().__init__()
        self.criterion = criterion

    @torch.no_grad()
    def forward(self, pred_batch, label_batch):
        assert pred_batch.shape[-1] == 3
        p, lead = _batch(pred_batch)
        l, _ = _batch(label_batch)
        sc = evaluate_poses(p, l, root=None, per_frame=True, return_aligned=True, return_errors=True)
        if pred_batch.dtype == torch.float64:  # (the kernel's aligned output is fp32: form Z from its transform)
            pd = p.to(sc.per_frame.device)
            aligned = sc.column("b")[:, None, None] * (pd @ sc.column("T")) + sc.column("c")[:, None, :]
        else:
            aligned = sc.aligned.to(pred_batch.dtype)
        aligned = aligned.reshape(pred_batch.shape).to(pred_batch.device)
        if isinstance(self.criterion, Criterion_MPJPE):
            score = _reduce(sc.pa_err.reshape(lead), self.criterion.reduction)
            return score.to(pred_batch.device, pred_batch.dtype), aligned
        return self.criterion(aligned, label_batch), aligned


class Criterion3DPose_leastQuaresScaled(torch.nn.Module):
    """evaluation_helpers.py:506-522: scale every pose of pred [B][J][3] by s_opt = <pred, label> / <pred, pred> (the
    kernel's, in double, over the vectors as they are given), then apply `criterion` -> (criterion(s_opt pred, label),
    s_opt pred).  Through anerf_pose_scores, as Criterion_MPJPE: [B][J][3] with J <= 128 only."""

    def __init__(self, criterion):
        super().__init__()
        self.criterion = criterion

    @torch.no_grad()
    def forward(self, pred, label):
        p, _ = _batch(pred)
        l, _ = _batch(label)
        sc = evaluate_poses(p, l, root=None, per_frame=True)
        s_opt = sc.column("s_opt").to(pred.device, pred.dtype).reshape(pred.shape[0], 1, 1)
        scaled = s_opt * pred
        return self.criterion.forward(scaled, label), scaled


@torch.no_grad()
def evaluate_pampjpe(pred_kps, gt_kps, ret_kp=False, ret_pck=False, align_kp=False, pck_threshold=150,
                     reduction="mean", use_normalize=False, root=14):
    """What evaluate_pampjpe_from_smpl_params returns (from its line 566 on), for given joints, from ONE
    evaluate_poses call: pred_kps [F][J][3] in metres (what the SMPL regressor gives), gt_kps in millimetres, both
    scored in millimetres.  -> (pampjpe, mpjpe): the aligned error and the error of both sides less their joint
    `root` (least-squares scaled under use_normalize), float64 device tensors reduced by `reduction`: 'mean' and 'sum'
    add up the kernel's pa_err plane and its per-frame scores, any other value gives the [F][J] planes (pampjpe the kernel's pa_err; the
    root-centred plane, which the kernel does not write out, is formed on the device from the inputs and the kernel's
    s_opt).  With ret_kp a third item follows: the kernel's aligned joints (fp32) under align_kp, else under ret_pck
    the pair (pck, auc) from the kernel's integer counts of pa_err < pck_threshold and < linspace(0, 150, 31) -- for
    every `reduction`, where the reference takes the PCK of a scalar under 'mean' -- else pred_kps as it came."""
    sc = evaluate_poses(pred_kps, gt_kps, root=root, pred_scale=1000.0, gt_scale=1.0, pck_threshold=pck_threshold,
                        per_frame=True, return_errors=True, return_aligned=bool(ret_kp and align_kp))
    n = sc.column("n")
    frame_mpjpe = sc.column("n_mpjpe" if use_normalize else "mpjpe_root")
    if reduction == "mean":
        scores = sc.pa_err.sum() / n.sum(), (frame_mpjpe * n).sum() / n.sum()
    elif reduction == "sum":
        scores = sc.pa_err.sum(), (frame_mpjpe * n).sum()
    else:
        dev = sc.pa_err.device
        p = _device_input(pred_kps, dev).double() * 1000.0
        g = _device_input(gt_kps, dev).double()
        p, g = p - p[:, root:root + 1], g - g[:, root:root + 1]
        if use_normalize:
            p = p * sc.column("s_opt")[:, None, None]
        scores = sc.pa_err, (p - g).norm(dim=-1)
    if not ret_kp:
        return scores
    if align_kp:
        return (*scores, sc.aligned)
    if ret_pck:
        return (*scores, sc.pck, sc.auc)
    return (*scores, pred_kps)


def evaluate_pampjpe_from_smpl_params(*args, **kwargs):
    raise NotImplementedError(
        "evaluate_pampjpe_from_smpl_params needs smpl/SMPL_NEUTRAL.pkl and the h36m joint regressor, which cannot be "
        "shipped: regress the joints yourself and pass them to evaluate_pampjpe(pred_kps, gt_kps, ...)")


@torch.no_grad()
def evaluate_pose_layer(layer, gt_kps, idxs=None, **kw):
    """Score a PoseOptLayer's joints against gt_kps [N_kps][J][3] (one row per pose of the layer): the kinematic chain
    runs on the device for the poses `idxs` (default: all) and its kps are scored without leaving it.  kw: as
    evaluate_poses (the layer's kps are in the dataset's unit, usually metres)."""
    idxs = np.arange(layer.N_kps) if idxs is None else np.atleast_1d(np.asarray(_lib.host_array(idxs))).astype(np.int64)
    kps = layer(idxs)[0]
    if torch.is_tensor(gt_kps):
        gt = gt_kps[torch.as_tensor(idxs, device=gt_kps.device)]
    else:
        gt = np.asarray(gt_kps)[idxs]
    return evaluate_poses(kps, gt, **kw)


@torch.no_grad()
def evaluate_pose_ckpt(path=None, popt_sd=None, gt_kps=None, init_kps=None, skel_type=None, device=None, **kw):
    """Score the refined poses of a `Trainer.save_popt` checkpoint (or of its poseopt_layer_state_dict) against
    gt_kps, and with init_kps, the poses the refinement started from, those as well ->
    {'refined': PoseScores, 'init': PoseScores | None, 'delta_pa_mpjpe', 'delta_mpjpe'} (refined - init, None
    without init_kps)."""
    from .sequences import SMPLSkeleton, load_poseopt_from_state_dict
    if gt_kps is None:
        raise ValueError("gt_kps is needed")
    if popt_sd is None:
        popt_sd = torch.load(path, map_location="cpu", weights_only=True)["poseopt_layer_state_dict"]
    layer = load_poseopt_from_state_dict({"poseopt_layer_state_dict": popt_sd},
                                         SMPLSkeleton if skel_type is None else skel_type, device)
    refined = evaluate_pose_layer(layer, gt_kps, **kw)
    init = None if init_kps is None else evaluate_poses(init_kps, gt_kps, **kw)
    return {"refined": refined, "init": init,
            "delta_pa_mpjpe": None if init is None else refined.pa_mpjpe - init.pa_mpjpe,
            "delta_mpjpe": None if init is None else refined.mpjpe - init.mpjpe}


__all__ = ["PoseScores", "FRAME_COLUMNS", "evaluate_poses", "evaluate_poses_reference", "procrustes_align",
           "procrustes", "Criterion_MPJPE", "Criterion3DPose_ProcrustesCorrected", "Criterion3DPose_leastQuaresScaled",
           "evaluate_pampjpe", "evaluate_pampjpe_from_smpl_params", "evaluate_pose_layer", "evaluate_pose_ckpt"]

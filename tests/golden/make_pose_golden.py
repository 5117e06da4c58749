"""Golden fixture for the pose scores: the reference's own core/utils/evaluation_helpers (lines 387-603) run on the
CPU on the seeded pairs of tests/_pose_cases.py, in the style of make_eval_golden.py.

  (a) `procrustes(gt, pred, scaling, reflection)` on float64 arrays, scaling in {True, False} x reflection in
      {'best', False, True}: d, Z, rotation, scale, translation per frame (a_<case>_s<scaling>_r<reflection>_*).
      With it the float64 run of the three Criterion* modules (a64_<case>_*), which are torch arithmetic.
  (b) the three Criterion* modules on float32 tensors, reduction mean / sum / none (b_<case>_<module>_<reduction>,
      and _aligned / _scaled for the tensors they return).
  (c) evaluate_pampjpe_from_smpl_params from its line 566 on, restated by calling those modules on given pred_kps
      (its SMPL part needs files that cannot be shipped): pred in metres, gt in millimetres, root 14, float32 as the
      function runs, and float64 for the gap (c_<variant>_*, c64_<variant>_*).
  (d) fp32_gap_<case> / fp32_gap_c: the largest |float32 result - float64 result| of the case over its pose extent
      (the smallest centred Frobenius norm of gt among its frames), over every per-joint number recorded (on the
      rank-deficient cases the aligned joints, which hang on an arbitrary completion, are left out).

Runs ONLY where the reference is present.  Usage: python tests/golden/make_pose_golden.py
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

REDUCTIONS = ("mean", "sum", "none")


def extent(gt):
    x0 = gt - gt.mean(1, keepdims=True)
    return np.sqrt((x0 ** 2).sum((1, 2)))


def run_modules(eh, torch, pred, gt, dtype):
    """The three modules on tensors of `dtype` -> {name: array}."""
    p, g = torch.tensor(pred, dtype=dtype), torch.tensor(gt, dtype=dtype)
    out = {}
    for red in REDUCTIONS:
        crit = eh.Criterion_MPJPE(reduction=red)
        out[f"mpjpe_{red}"] = crit(p, g).numpy()
        v, al = eh.Criterion3DPose_ProcrustesCorrected(crit)(p, g)
        out[f"pa_{red}"], out["pa_aligned"] = v.numpy(), al.numpy()
        v, sc = eh.Criterion3DPose_leastQuaresScaled(crit)(p, g)
        out[f"lsq_{red}"], out["lsq_scaled"] = v.numpy(), sc.numpy()
    return out


def run_pampjpe(eh, torch, pred_m, gt_mm, dtype, use_normalize, reduction):
    """What the reference computes from its line 566 on, with tensors of `dtype` where it builds FloatTensors."""
    crit = eh.Criterion_MPJPE(reduction=reduction)
    pa_crit = eh.Criterion3DPose_ProcrustesCorrected(crit)
    pred = torch.tensor(pred_m, dtype=dtype)
    pa, aligned = pa_crit(pred, torch.tensor(gt_mm, dtype=dtype))
    gt_c = gt_mm - gt_mm[:, 14:15]
    pred_c = pred - pred[:, 14:15]
    plain = eh.Criterion3DPose_leastQuaresScaled(crit) if use_normalize else crit
    mp = plain(pred_c, torch.tensor(gt_c / 1000, dtype=dtype))
    mp = (mp[0] if use_normalize else mp) * 1000
    pck = (pa < 150).float().mean()
    auc = np.mean([(pa < t).float().mean().item() for t in torch.linspace(0, 150, 31).tolist()])
    return {"pampjpe": pa.numpy(), "mpjpe": mp.numpy(), "aligned": aligned.numpy(), "pck": np.float64(pck.item()),
            "auc": np.float64(auc)}


def gap(lo, hi, ext, keys):
    return max(float(np.abs(np.asarray(lo[k], np.float64) - np.asarray(hi[k], np.float64)).max()) for k in keys) / ext


def main():
    import torch
    cases = importlib.import_module("_pose_cases")
    mg.import_reference()
    eh = importlib.import_module("core.utils.evaluation_helpers")
    out = {}
    per_joint = ("mpjpe_none", "pa_none", "lsq_none", "pa_aligned", "lsq_scaled")
    for name in cases.GOLDEN_CASES:
        pred, gt = cases.golden_pair(name)
        for scaling, reflection in cases.COMBOS:
            key = cases.combo_key(name, scaling, reflection)
            rows = [eh.procrustes(gt[f].copy(), pred[f].copy(), scaling, reflection) for f in range(len(gt))]
            out[key + "_d"] = np.array([r[0] for r in rows], np.float64)
            out[key + "_Z"] = np.stack([r[1] for r in rows]).astype(np.float64)
            out[key + "_T"] = np.stack([r[2]["rotation"] for r in rows]).astype(np.float64)
            out[key + "_b"] = np.array([r[2]["scale"] for r in rows], np.float64)
            out[key + "_c"] = np.stack([r[2]["translation"] for r in rows]).astype(np.float64)
        hi = run_modules(eh, torch, pred, gt, torch.float64)
        lo = run_modules(eh, torch, pred, gt, torch.float32)
        for k, v in hi.items():
            out[f"a64_{name}_{k}"] = v
        for k, v in lo.items():
            out[f"b_{name}_{k}"] = v
        # (where A is rank deficient the aligned joints hang on an arbitrary completion: the scores alone)
        keys = [k for k in per_joint if k != "pa_aligned" or name in cases.WELL_CONDITIONED]
        out[f"fp32_gap_{name}"] = np.float64(gap(lo, hi, extent(gt).min(), keys))
    pred_m, gt_mm = cases.pampjpe_pair()
    gaps = []
    for norm in (False, True):
        for red in ("mean", "none"):
            lo = run_pampjpe(eh, torch, pred_m, gt_mm, torch.float32, norm, red)
            hi = run_pampjpe(eh, torch, pred_m, gt_mm, torch.float64, norm, red)
            for k in lo:
                out[f"c_n{int(norm)}_{red}_{k}"] = lo[k]
                out[f"c64_n{int(norm)}_{red}_{k}"] = hi[k]
            gaps.append(gap(lo, hi, extent(gt_mm).min(), ("pampjpe", "mpjpe", "aligned")))
    out["fp32_gap_c"] = np.float64(max(gaps))
    # the PCK counts must not hang on float32 rounding: no float64 error within 0.01 mm of a threshold
    e = out["c64_n0_none_pampjpe"].reshape(-1, 1)
    margin = np.abs(e - np.linspace(0, 150, 31)[None]).min()
    assert margin > 1e-2, f"an aligned error lies {margin} from a threshold: choose another seed in _pose_cases"
    path = os.path.join(HERE, "pose_scores.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print({k: float(v) for k, v in out.items() if k.startswith("fp32_gap")}, "threshold margin", margin)


if __name__ == "__main__":
    main()

"""Time the scoring of refined poses: 10,000 frames of 24 joints (a sequence's order), pred in metres against gt in
millimetres, root 0, the reference's 31 thresholds.

  * kernel_ms           anerf_pose_scores (the score launch and both launches of the total kernel), by events after
                        warm-up, inputs and outputs already on the device
  * evaluate_poses_ms   evaluate_poses on device tensors, with its allocation and its one device read, wall clock
  * numpy_checker_ms    evaluate_poses_reference on the host (batched np.linalg.svd), one run
  * per_frame_loop_ms   the reference's way, restated: a Python loop over evaluate_poses_reference on single frames
                        (one LAPACK SVD per frame), timed on --loop-frames frames and scaled to all of them

Writes the numbers to profiles/pose_bench.json (--out) and prints the same JSON line.  No threshold is set on them.
The poses are seeded: ground truth of a standing body's extent in millimetres, pred a similarity transform of it with
45 mm of noise, in metres."""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

anerf = importlib.import_module("a-nerf_amd")
ps = importlib.import_module("a-nerf_amd.posescore")
_lib = importlib.import_module("a-nerf_amd._lib")


def make_poses(F, J, seed=2024, noise=45.0):
    """-> (pred in metres, gt in millimetres), float32 [F][J][3]."""
    rs = np.random.default_rng(seed)
    gt = rs.normal(size=(F, J, 3)) * np.array([220.0, 450.0, 160.0]) + np.array([350.0, -900.0, 2600.0])
    q = np.linalg.qr(rs.normal(size=(F, 3, 3)))[0]
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]  # rotations
    b = rs.uniform(0.6, 1.6, size=(F, 1, 1))
    pred = ((gt - rs.normal(size=(F, 1, 3)) * 400.0) / b) @ q + rs.normal(size=gt.shape) * noise / b
    return (pred / 1000.0).astype(np.float32), gt.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_bench.json"))
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--joints", type=int, default=24)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--loop-frames", type=int, default=500)
    a = ap.parse_args()
    F, J = a.frames, a.joints
    pred_h, gt_h = make_poses(F, J)
    pred = torch.from_numpy(pred_h).float().cuda()
    gt = torch.from_numpy(gt_h).float().cuda()
    kw = dict(pred_scale=1000.0, root=0)
    lib = _lib.load()
    th = np.ascontiguousarray(np.append(ps.AUC_THRESHOLDS, 150.0))
    need = _lib.workspace("anerf_pose_scores_workspace", F, J, len(th))
    ws = torch.empty(need // 8, device="cuda", dtype=torch.float64)
    totals = torch.empty(_lib.ANERF_POSE_TOTALS, device="cuda", dtype=torch.float64)
    st = _lib.stream_handle()

    def kernel():
        _lib.check(lib.anerf_pose_scores(_lib.ptr(pred), _lib.ptr(gt), F, J, None, 0, None, 0, 1000.0, 1.0, 0,
                                         th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(th), _lib.ptr(totals),
                                         None, None, None, None, _lib.ptr(ws), need, st), "anerf_pose_scores")

    for _ in range(5):
        kernel()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        kernel()
    e1.record()
    torch.cuda.synchronize()
    kernel_ms = e0.elapsed_time(e1) / a.reps

    for _ in range(3):
        got = anerf.evaluate_poses(pred, gt, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        got = anerf.evaluate_poses(pred, gt, **kw)
    evaluate_ms = (time.perf_counter() - t0) * 1e3 / a.reps

    t0 = time.perf_counter()
    want = ps.evaluate_poses_reference(pred_h.astype(np.float32), gt_h.astype(np.float32), **kw)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    n = min(F, a.loop_frames)
    p32, g32 = pred_h.astype(np.float32), gt_h.astype(np.float32)
    t0 = time.perf_counter()
    for f in range(n):
        ps.evaluate_poses_reference(p32[f:f + 1], g32[f:f + 1], **kw)
    loop_ms = (time.perf_counter() - t0) * 1e3 * F / n

    out = {"what": "anerf_pose_scores: MPJPE, root-centred and scaled MPJPE, PA-MPJPE, 32 threshold counts",
           "frames": F, "joints": J, "reps": a.reps, "kernel_ms": round(kernel_ms, 4),
           "kernel_ns_per_frame": round(kernel_ms / F * 1e6, 2), "evaluate_poses_ms": round(evaluate_ms, 4),
           "numpy_checker_host_ms": round(numpy_ms, 1), "per_frame_python_loop_host_ms": round(loop_ms, 1),
           "per_frame_loop_frames_timed": n, "pa_mpjpe": got.pa_mpjpe, "mpjpe_root": got.mpjpe_root, "pck": got.pck,
           "auc": got.auc, "abs_pa_mpjpe_kernel_vs_numpy": abs(got.pa_mpjpe - want.pa_mpjpe),
           "counts_equal_numpy": bool(np.array_equal(got.pck_counts, want.pck_counts)),
           "device_bytes_read_by_host": int(totals.numel() * 8)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

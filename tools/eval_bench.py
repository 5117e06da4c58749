"""Time the scoring of rendered frames: 8 frames of 512 x 512 with the benchmark's config-3 boxes.

  * kernel_ms      anerf_eval_frames (both launches, whole frames + mask + box weights, no map), by events after warm-up
  * torch_fp32_ms  the fp32 torch conv2d restatement of the SSIM map on the same device (tests/_eval_cases.py), by events
  * numpy_ms       the float64 NumPy checker on the host (evaluate_frames_reference), one run

Writes the numbers to profiles/eval_bench.json (--out) and prints the same JSON line.

Needs the tests folder beside it: the frames (make_case) and the fp32 yardstick (ssim_fp32_torch) are the tests' own,
tests/_eval_cases.py, so that the tool times what the tests pin."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _eval_cases as cases  # noqa: E402

anerf = importlib.import_module("a-nerf_amd")
_lib = importlib.import_module("a-nerf_amd._lib")
syn = importlib.import_module("a-nerf_amd.synthetic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    F_, H, W = 8, 512, 512
    sc = syn.make_scene(n_joints=24, H=H, W=W, seed=13, n_frames=F_, yaw_step=0.4)
    _, _, bboxes = anerf.rays.valid_pixels(sc["c2ws"], H, W, sc["focal"], kps=sc["kps"], ext_scale=0.001)
    c = cases.make_case(H, W, 5, F_)
    pred = torch.from_numpy(np.array(c["pred"])).cuda()
    gt = torch.from_numpy(np.array(c["gt_u8"])).cuda()
    mask = torch.from_numpy(np.array(c["mask"])).cuda()
    rects = np.ascontiguousarray([[0, 0, W, H]] * F_, np.int32)
    boxes = np.ascontiguousarray([[tl[0], tl[1], br[0], br[1]] for tl, br in bboxes], np.int32)
    lib = _lib.load()
    need = _lib.workspace("anerf_eval_workspace", F_, H, W)
    ws = torch.empty(need // 8, device="cuda", dtype=torch.float64)
    sums = torch.empty(F_, 9, device="cuda", dtype=torch.float64)
    st = _lib.stream_handle()

    def kernel():
        _lib.check(lib.anerf_eval_frames(_lib.ptr(pred), _lib.ptr(gt), 1, _lib.ptr(mask),
                                         rects.ctypes.data_as(_lib.c_i32p), boxes.ctypes.data_as(_lib.c_i32p), F_, H, W,
                                         1.0, 0, None, _lib.ptr(sums), _lib.ptr(ws), need, st), "anerf_eval_frames")

    gt_f = gt.float() / 255.0

    def torch_fp32():
        return cases.ssim_fp32_torch(pred, gt_f, 1.0, device="cuda")

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    kernel_ms, torch_ms = timed(kernel), timed(torch_fp32)
    t0 = time.perf_counter()
    want = anerf.evaluate_frames_reference(c["pred"], c["gt_u8"], masks=c["mask"], bboxes=bboxes)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    got = sums.cpu().numpy()
    f32 = torch_fp32().double().mean(dim=(1, 2, 3)).cpu().numpy()
    out = {"what": "anerf_eval_frames: PSNR + SSIM sums of whole frames, mask and box weights",
           "frames": F_, "H": H, "W": W, "reps": a.reps, "kernel_ms": round(kernel_ms, 4),
           "kernel_us_per_frame": round(kernel_ms / F_ * 1e3, 2), "torch_fp32_conv2d_ms": round(torch_ms, 4),
           "numpy_float64_host_ms": round(numpy_ms, 1),
           "max_abs_ssim_kernel_vs_numpy": float(np.abs(got[:, 2] / (3 * got[:, 0]) - want.ssim).max()),
           "max_abs_ssim_torch_fp32_vs_numpy": float(np.abs(f32 - want.ssim).max()),
           "device_bytes_read_by_host": int(got.nbytes)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Time the dataset-preparation kernels at 512 x 512, each beside its NumPy / scipy checker on the host.

  * sampling_masks     256 masks, radius 6 (5 x 5, three iterations) with the band
  * create_kp_masks    256 masks from 2-D key points (two launches)
  * draw_skeletons_3d  91 frames (projection in torch, one launch)
  * median_backgrounds 1,000 frames over 4 cameras, without and with masks

Device times are by events after warm-up, the median over --reps calls; host times are one run of the vectorised
checker (a-nerf_amd/preprocess.py).  The masked median's per-pixel loop (load_zju.py:266-281, tests/_prep_cases.py) is
timed on --loop-rows rows of one camera and scaled to the whole job: that figure is marked as extrapolated.

Writes the numbers to profiles/prep_bench.json (--out) and prints the same JSON line.  Needs the tests folder beside it
(tests/_prep_cases.py), so that the tool times what the tests pin."""
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
import _prep_cases as cases  # noqa: E402

anerf = importlib.import_module("a-nerf_amd")
prep = importlib.import_module("a-nerf_amd.preprocess")
syn = importlib.import_module("a-nerf_amd.synthetic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prep_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-rows", type=int, default=4)
    a = ap.parse_args()
    H = W = 512
    rs = np.random.RandomState(0)

    def device_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times))

    def host_ms(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    def same(got, want):
        return bool(np.array_equal(got.cpu().numpy(), want))

    out = {"what": "dataset preparation at 512 x 512: device kernels (events, median of reps) beside the host checkers",
           "H": H, "W": W, "reps": a.reps}

    # masks: a person-sized blob per mask, from a projected skeleton drawn wide
    n_masks = 256
    sc = syn.make_scene(n_joints=24, H=H, W=W, seed=1, n_frames=n_masks, yaw_step=0.05)
    kp2d = prep.skeleton3d_to_2d_reference(sc["kps"], sc["c2ws"], H, W, 3.0 * H)
    segs = prep.skeleton_segments_reference(kp2d)
    masks = prep.draw_segments_reference(segs, H, W, 41)
    masks_d = torch.from_numpy(masks).cuda()
    ms = device_ms(lambda: anerf.sampling_masks(masks_d, 3, 5, True))
    ref_ms, want = host_ms(lambda: anerf.sampling_masks_reference(masks, 3, 5, True))
    out["sampling_masks"] = {"masks": n_masks, "radius": 6, "band": 2, "device_ms": round(ms, 4),
                             "host_numpy_ms": round(ref_ms, 1),
                             "bit_identical": same(anerf.sampling_masks(masks_d, 3, 5, True), want)}
    try:
        ref_ms, got = host_ms(lambda: np.stack([cases.get_mask_scipy(m, True) for m in masks]))
        out["sampling_masks"]["host_scipy_ms"] = round(ref_ms, 1)
        out["sampling_masks"]["scipy_equals_numpy"] = bool(np.array_equal(got, want))
    except ImportError:
        pass

    kp2d_d = torch.from_numpy(kp2d).cuda()
    ms = device_ms(lambda: anerf.create_kp_masks(masks_d, kp2ds=kp2d_d))
    ref_ms, want = host_ms(lambda: anerf.create_kp_masks_reference(masks, kp2ds=kp2d))
    out["create_kp_masks"] = {"masks": n_masks, "extend_iter": 3, "device_ms": round(ms, 4),
                              "host_numpy_ms": round(ref_ms, 1),
                              "bit_identical": same(anerf.create_kp_masks(masks_d, kp2ds=kp2d_d), want)}

    n_frames = 91
    frames = rs.randint(0, 256, (n_frames, H, W, 3)).astype(np.uint8)
    frames_d = torch.from_numpy(frames).cuda()
    kps_d, c2ws_d = torch.from_numpy(sc["kps"][:n_frames]).cuda(), torch.from_numpy(sc["c2ws"][:n_frames]).cuda()
    ms = device_ms(lambda: anerf.draw_skeletons_3d(frames_d, kps_d, c2ws_d, H, W, 3.0 * H))
    ref_ms, want = host_ms(lambda: anerf.draw_skeletons_3d_reference(frames, sc["kps"][:n_frames], sc["c2ws"][:n_frames],
                                                                     H, W, 3.0 * H))
    out["draw_skeletons_3d"] = {"frames": n_frames, "width": 3, "device_ms_with_copy_and_projection": round(ms, 4),
                                "host_numpy_ms": round(ref_ms, 1),
                                "bit_identical": same(anerf.draw_skeletons_3d(frames_d, kps_d, c2ws_d, H, W, 3.0 * H), want)}
    del frames_d

    n_imgs, n_cams = 1000, 4
    imgs = rs.randint(0, 256, (n_imgs, H * W, 3)).astype(np.uint8)
    cam = np.arange(n_imgs) % n_cams
    fg = np.tile(masks, (4, 1, 1))[:n_imgs].reshape(n_imgs, H * W)
    imgs_d, fg_d = torch.from_numpy(imgs).cuda(), torch.from_numpy(fg).cuda()
    for key, m, m_d in (("median_backgrounds", None, None), ("median_backgrounds_masked", fg, fg_d)):
        ms = device_ms(lambda: anerf.median_backgrounds(imgs_d, cam, m_d, H=H, W=W))
        ref_ms, want = host_ms(lambda: anerf.median_backgrounds_reference(imgs, cam, m, H=H, W=W))
        out[key] = {"frames": n_imgs, "cameras": n_cams, "device_ms": round(ms, 4),
                    "host_numpy_vectorised_ms": round(ref_ms, 1),
                    "bit_identical": same(anerf.median_backgrounds(imgs_d, cam, m_d, H=H, W=W), want)}
    rows = a.loop_rows
    sub = imgs.reshape(n_imgs, H, W, 3)[cam == 0, :rows].reshape(-1, rows * W, 3)
    sub_m = fg.reshape(n_imgs, H, W)[cam == 0, :rows].reshape(-1, rows * W)
    ref_ms, _ = host_ms(lambda: cases.median_loop(sub, sub_m, np.zeros(len(sub), np.int64), 1, rows, W))
    out["median_backgrounds_masked"]["host_per_pixel_loop_rows_timed"] = rows
    out["median_backgrounds_masked"]["host_per_pixel_loop_ms_of_those_rows"] = round(ref_ms, 1)
    out["median_backgrounds_masked"]["host_per_pixel_loop_ms_extrapolated"] = round(ref_ms * (H / rows) * n_cams, 0)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Golden fixture for the AGGREGATION rules of evaluate_metric: the reference's own
core/utils/evaluation_helpers.evaluate_metric (lines 257-385) run on the CPU, in the style of make_golden.py.

The reference imports pytorch_msssim, which is not available; its SSIM is replaced by a stand-in that returns this
project's float64 map (a-nerf_amd/evaluation.ssim_map_reference, data_range 1, border "same") as N x 3 x H x W, the
shape both call sites of the reference expect.  So the fixture pins what the reference does WITH a map -- dropping
frames with an empty mask, denom = max(3 sum(mask), 1), inf -> 0, the mean over frames, which of plain / fg / valid it
returns -- and its fp32 squared error, not the map itself.

Two reference quirks are worked round: it opens vid_base + "psnr.txt" whatever vid_base is (so a temporary directory
is given, and imageio.mimwrite is a stub), and without masks it raises at its return statement (psnr_fg is unbound)
after it has written its scores: for that case the scores are read back from the files it wrote.

Inputs: 3 frames of 48 x 40 (tests/_eval_cases.make_case), masks with the middle one empty, boxes per frame.
Cases: no mask, a mask, eval_both.  The box variant (run_render.evaluate_metric) is recorded too when run_render
imports under the stubs.

Runs ONLY where the reference is present.  Usage: python tests/golden/make_eval_golden.py
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

H, W, SEED = 48, 40, 71
BOXES = np.array([[3, 5, 38, 44], [0, 0, 40, 48], [10, 12, 31, 40]], np.int32)  # x0, y0, x1, y1


def stand_in_ssim():
    import torch
    ev = importlib.import_module("a-nerf_amd.evaluation")
    m = types.ModuleType("pytorch_msssim")

    class SSIM:
        def __init__(self, *a, **k):
            pass

        def __call__(self, X, Y):
            x, y = X.permute(0, 2, 3, 1).numpy(), Y.permute(0, 2, 3, 1).numpy()
            maps = np.stack([ev.ssim_map_reference(a, b, 1.0) for a, b in zip(x, y)])
            return torch.from_numpy(maps).permute(0, 3, 1, 2)

    m.SSIM = SSIM
    sys.modules["pytorch_msssim"] = m


def read_score(path):
    with open(path) as f:
        return float(f.read().split()[-1])


def main():
    import torch
    cases = importlib.import_module("_eval_cases")
    stand_in_ssim()
    mg.import_reference()
    eh = importlib.import_module("core.utils.evaluation_helpers")
    box_px = importlib.import_module("a-nerf_amd.rays").box_pixels
    c = cases.make_case(H, W, SEED, 3)
    rgbs, gt = np.array(c["pred"]), np.array(c["gt"])
    masks = np.array(c["mask"])
    masks[1] = 0  # a frame without a person: dropped
    gt_masks = masks[..., None].astype(np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    valid_idxs = [torch.from_numpy(box_px((b[0], b[1]), (b[2], b[3]), W)) for b in BOXES]
    out = {"rgbs": rgbs, "gt_u8": np.array(c["gt_u8"]), "masks": masks, "boxes": BOXES}
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "nomask", "v_")
        try:
            eh.evaluate_metric(rgbs.copy(), gt.copy(), poses=poses, hwf=(H, W, 100.0), vid_base=base)
            raise SystemExit("the reference returned without masks: record its dict instead")
        except UnboundLocalError:
            out["nomask"] = np.array([read_score(base + "psnr.txt"), read_score(base + "ssim.txt")], np.float64)
        for name, both in (("mask", False), ("both", True)):
            r = eh.evaluate_metric(rgbs.copy(), gt.copy(), gt_masks=gt_masks.copy(), valid_idxs=valid_idxs,
                                   poses=poses, hwf=(H, W, 100.0), vid_base=os.path.join(tmp, name, "v_"),
                                   eval_both=both)
            out[name] = np.array([r["psnr"], r["ssim"], r["psnr_fg"], r["ssim_fg"]], np.float64)
        try:
            rr = importlib.import_module("run_render")
        except Exception as e:  # noqa: BLE001
            print(f"run_render does not import under the stubs ({type(e).__name__}: {e}): no box fixture")
            rr = None
        if rr is not None:
            bd = os.path.join(tmp, "box")
            os.makedirs(bd)
            bboxes = [((b[0], b[1]), (b[2], b[3])) for b in BOXES]
            accs = [None] * 3  # (zipped over, never read)
            rr.evaluate_metric(rgbs.copy(), accs, bboxes,
                               {"gt_paths": [np.array(g).reshape(-1) for g in c["gt_u8"]],
                                "gt_mask_paths": [m.reshape(-1) for m in masks], "is_gt_paths": False,
                                "bg_imgs": None, "bg_indices": None}, bd)
            sd = np.load(os.path.join(bd, "scores.npy"), allow_pickle=True).item()
            for k in ("psnr", "ssim", "fg_psnr", "fg_ssim"):
                out["box_" + k] = np.asarray(sd[k], np.float64)
    path = os.path.join(HERE, "eval_metric.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v for k, v in out.items() if v.size <= 8})


if __name__ == "__main__":
    main()

"""Frame scoring on the host: the float64 checker against the definition, the fp32 yardstick that shows why the device
kernel is double, and evaluate_metric / evaluate_box_metric's aggregation rules against the reference's own code
(tests/golden/eval_metric.npz, written by tests/golden/make_eval_golden.py)."""
import importlib
import os

import numpy as np
import pytest

import _eval_cases as cases

anerf = importlib.import_module("a-nerf_amd")
ev = importlib.import_module("a-nerf_amd.evaluation")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metric.npz")
SSIM_TOL, PSNR_TOL = 1e-6, 1e-5  # the reference squares and averages in fp32: a few 2^-24 relative, ~1e-6 dB


def test_uint8_ground_truth_is_the_nearest_float32():
    """float32(v / 255.) -- the reference's `/ 255.` then astype(float32), and the kernel's rule -- is the fp32 nearest
    to v / 255 for all 256 bytes (no double rounding)."""
    from fractions import Fraction
    for v in range(256):
        got = np.float32(np.float64(v) / 255.)
        exact = Fraction(v, 255)
        err = abs(Fraction(float(got)) - exact)
        for other in (np.nextafter(got, np.float32(2)), np.nextafter(got, np.float32(-1))):
            assert err <= abs(Fraction(float(other)) - exact), v


@pytest.mark.parametrize("border", ["same", "valid"])
@pytest.mark.parametrize("data_range", [1.0, 255.0])
def test_checker_matches_the_direct_121_tap_definition(border, data_range):
    c = cases.make_case(13, 16, 3)
    direct = cases.ssim_direct(c["pred"][0], c["gt"][0], data_range, border)
    sc = anerf.evaluate_frames_reference(c["pred"], c["gt"], data_range=data_range, border=border, return_map=True)
    got = sc.map[0] if border == "same" else sc.map[0][5:-5, 5:-5]
    assert got.shape == direct.shape
    assert np.abs(got - direct).max() <= 1e-12
    assert abs(sc.ssim[0] - direct.mean()) <= 1e-12
    assert sc.n[0] == direct.shape[0] * direct.shape[1]
    if border == "valid":  # nothing is scored outside the interior
        outer = sc.map[0].copy()
        outer[5:-5, 5:-5] = 0
        assert not outer.any()


def test_fp32_restatement_is_off_by_more_than_1e_5_per_pixel():
    """The fp32 conv2d restatement of the package against the float64 checker on the frame with a flat background:
    C2 = 9e-4 sits under differences of fp32 numbers near 1.  This is why the kernel forms its moments in double."""
    c = cases.make_case(48, 40, 5)
    ref = anerf.evaluate_frames_reference(c["pred"], c["gt"], return_map=True).map[0]
    for data_range in (1.0, 255.0):
        f32 = cases.ssim_fp32_torch(c["pred"], c["gt"], data_range)[0].numpy().astype(np.float64)
        r = ref if data_range == 1.0 else anerf.evaluate_frames_reference(c["pred"], c["gt"], data_range=255.0,
                                                                          return_map=True).map[0]
        print(f"data_range {data_range}: max |fp32 - float64| per pixel = {np.abs(f32 - r).max():.3e}")
        if data_range == 1.0:
            assert np.abs(f32 - r).max() > 1e-5


def _golden():
    z = np.load(GOLDEN)
    gt = (z["gt_u8"] / 255.).astype(np.float32)
    boxes = [((int(b[0]), int(b[1])), (int(b[2]), int(b[3]))) for b in z["boxes"]]
    return z, gt, boxes


def _close(got, want):
    assert abs(got["psnr"] - want[0]) <= PSNR_TOL and abs(got["ssim"] - want[1]) <= SSIM_TOL, (got, want)
    if len(want) > 2:
        assert abs(got["psnr_fg"] - want[2]) <= PSNR_TOL and abs(got["ssim_fg"] - want[3]) <= SSIM_TOL, (got, want)


@pytest.mark.parametrize("gt_as", ["float32", "uint8"])
def test_evaluate_metric_reproduces_the_reference(gt_as):
    z, gt, boxes = _golden()
    H, W = gt.shape[1:3]
    g = gt if gt_as == "float32" else z["gt_u8"]
    kw = dict(hwf=(H, W, 100.0), backend=anerf.evaluate_frames_reference)
    assert not z["masks"][1].any() and z["masks"][0].any()
    got = anerf.evaluate_metric(z["rgbs"], g, **kw)
    _close(got, z["nomask"])
    assert got["psnr_fg"] is None and got["ssim_fg"] is None
    _close(anerf.evaluate_metric(z["rgbs"], g, gt_masks=z["masks"][..., None], **kw), z["mask"])
    vids = [anerf.rays.box_pixels(tl, br, W) for tl, br in boxes]
    _close(anerf.evaluate_metric(z["rgbs"], g, gt_masks=z["masks"][..., None], valid_idxs=vids, eval_both=True, **kw),
           z["both"])
    _close(anerf.evaluate_metric(z["rgbs"], g, gt_masks=z["masks"][..., None], bboxes=boxes, eval_both=True, **kw),
           z["both"])


def test_evaluate_box_metric_reproduces_the_reference():
    z, gt, boxes = _golden()
    gd = {"gt_paths": [g.reshape(-1) for g in z["gt_u8"]], "gt_mask_paths": [m.reshape(-1) for m in z["masks"]],
          "is_gt_paths": False, "bg_imgs": None, "bg_indices": None}
    got = anerf.evaluate_box_metric(z["rgbs"], None, boxes, gd, backend=anerf.evaluate_frames_reference)
    for k, tol in (("psnr", PSNR_TOL), ("ssim", SSIM_TOL), ("fg_psnr", PSNR_TOL), ("fg_ssim", SSIM_TOL)):
        assert len(got[k]) == 2  # (the frame with an empty mask is skipped)
        assert np.abs(np.asarray(got[k]) - z["box_" + k]).max() <= tol, k


def test_box_metric_composites_the_background_where_the_mask_is_clear():
    z, gt, boxes = _golden()
    bg = np.full((1,) + gt.shape[1:], 0.25, np.float32)
    gd = {"gt_paths": list(z["gt_u8"]), "gt_mask_paths": list(z["masks"]), "is_gt_paths": False, "bg_imgs": bg,
          "bg_indices": [0, 0, 0]}
    got = anerf.evaluate_box_metric(z["rgbs"], None, boxes, gd, backend=anerf.evaluate_frames_reference)
    m = z["masks"][..., None].astype(np.float64)
    comp = (z["gt_u8"] / 255. * m + (1. - m) * bg).astype(np.float32)
    want = anerf.evaluate_frames_reference(z["rgbs"], comp, masks=z["masks"], bboxes=boxes, crop=True)
    keep = want.n_fg > 0
    assert np.array_equal(np.asarray(got["psnr"]), want.psnr[keep])
    assert np.array_equal(np.asarray(got["fg_ssim"]), want.fg_ssim[keep])


def h36m_case():
    """A 1000-row render with 1002-row ground truth and mask (the h36m images), and the same trimmed by hand."""
    rng = np.random.default_rng(4)
    gt = rng.integers(0, 256, (1002, 12, 3)).astype(np.uint8)
    mask = (rng.random((1002, 12)) < 0.5).astype(np.uint8)
    rgb = ((gt[1:-1] / 255.) + 0.02 * rng.standard_normal((1000, 12, 3))).astype(np.float32)
    boxes = [((2, 1), (11, 1000))]  # (reaches the last row: a frame that was not trimmed would be one row off)
    gd = lambda g, m: {"gt_paths": [g], "gt_mask_paths": [m], "is_gt_paths": False, "bg_imgs": None,  # noqa: E731
                       "bg_indices": None}
    return rgb[None], boxes, gd(gt.reshape(-1), mask.reshape(-1)), gd(gt[1:-1], mask[1:-1])


def test_box_metric_trims_1002_row_images_against_a_1000_row_render():
    rgbs, boxes, gd, gd_trimmed = h36m_case()
    got = anerf.evaluate_box_metric(rgbs, None, boxes, gd, backend=anerf.evaluate_frames_reference)
    want = anerf.evaluate_box_metric(rgbs, None, boxes, gd_trimmed, backend=anerf.evaluate_frames_reference)
    assert got == want and len(got["fg_psnr"]) == 1 and 30.0 < got["psnr"][0] < 40.0
    with pytest.raises(ValueError):  # (neither the frame's size nor the 1002-row one)
        anerf.evaluate_box_metric(rgbs, None, boxes, {**gd, "gt_paths": [gd["gt_paths"][0][:-3]]},
                                  backend=anerf.evaluate_frames_reference)


def test_mask_forms_agree_and_images_are_thresholded_at_128():
    c = cases.make_case(48, 40, 5)
    m = c["mask"]
    base = anerf.evaluate_frames_reference(c["pred"], c["gt"], masks=m).sums
    soft = np.where(m[0] > 0, 200, 90).astype(np.uint8)[None]  # a 0..255 image: 90 is background
    for other in (m.astype(bool), m.astype(np.float32), m[..., None] * np.ones((1, 1, 1, 3), np.float32), soft):
        assert np.array_equal(anerf.evaluate_frames_reference(c["pred"], c["gt"], masks=other).sums, base)


def test_nothing_is_written_without_vid_base_or_basedir(tmp_path, monkeypatch):
    z, gt, boxes = _golden()
    monkeypatch.chdir(tmp_path)
    anerf.evaluate_metric(z["rgbs"], gt, gt_masks=z["masks"][..., None], bboxes=boxes, eval_both=True,
                          hwf=(48, 40, 100.0), backend=anerf.evaluate_frames_reference)
    gd = {"gt_paths": list(z["gt_u8"]), "gt_mask_paths": list(z["masks"]), "is_gt_paths": False, "bg_imgs": None,
          "bg_indices": None}
    anerf.evaluate_box_metric(z["rgbs"], None, boxes, gd, backend=anerf.evaluate_frames_reference)
    assert os.listdir(tmp_path) == []
    # and with them: the reference's files
    anerf.evaluate_metric(z["rgbs"], gt, gt_masks=z["masks"][..., None], bboxes=boxes, eval_both=True,
                          hwf=(48, 40, 100.0), backend=anerf.evaluate_frames_reference,
                          vid_base=str(tmp_path / "out" / "v_"), eval_postfix="_t")
    assert sorted(os.listdir(tmp_path / "out")) == ["v_psnr_t.txt", "v_psnr_t_fg.txt", "v_ssim_t.txt", "v_ssim_t_fg.txt"]
    assert abs(float(open(tmp_path / "out" / "v_psnr_t.txt").read()) - z["both"][0]) <= PSNR_TOL
    anerf.evaluate_box_metric(z["rgbs"], None, boxes, gd, basedir=str(tmp_path / "box"),
                              backend=anerf.evaluate_frames_reference)
    assert sorted(os.listdir(tmp_path / "box")) == ["score_final.txt", "scores.npy"]

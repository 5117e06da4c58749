"""The NumPy checkers of a-nerf_amd/preprocess.py against independent statements (no GPU): scipy.ndimage's grey
morphology, np.median and load_zju.py's per-pixel loop, a brute force over exact fractions, the projection composed
frame by frame.  tests/test_gpu_prep.py holds the kernels bit-identical to these checkers."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prep_cases as cases  # noqa: E402

prep = importlib.import_module("a-nerf_amd.preprocess")
_lib = importlib.import_module("a-nerf_amd._lib")
kin = importlib.import_module("a-nerf_amd.kinematics")


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("op", ["dilate", "erode"])
@pytest.mark.parametrize("radius", [0, 2, 6, 10])
def test_morphology_checker_vs_scipy(radius, op, binary):
    """radius = iterations x 2 with the 5 x 5 element (radius 0: no iteration), on {0, 1} and on random bytes."""
    pytest.importorskip("scipy")
    masks = cases.mask_stack(37, 70, 3, binary)
    want = cases.morph_scipy(masks, op, 5, radius // 2)
    got = prep.mask_morph_reference(masks, op, radius)
    assert got.dtype == np.uint8 and got.shape == masks.shape
    np.testing.assert_array_equal(got, want)
    # a 3 x 3 element, radius iterations: the same window
    np.testing.assert_array_equal(got, cases.morph_scipy(masks, op, 3, radius))


@pytest.mark.parametrize("op", ["dilate", "erode"])
@pytest.mark.parametrize("kernel,iterations", [(5, 0), (5, 1), (5, 3), (5, 5), (3, 4), (7, 2), (1, 3)])
def test_iterated_form_is_the_single_window(kernel, iterations, op):
    for binary in (True, False):
        masks = cases.mask_stack(33, 16, 5, binary)
        np.testing.assert_array_equal(prep.morph_iterated_reference(masks, op, kernel, iterations),
                                      prep.mask_morph_reference(masks, op, prep.fold_radius(kernel, iterations)))
    fn = prep.dilate_masks_reference if op == "dilate" else prep.erode_masks_reference
    np.testing.assert_array_equal(fn(masks, iterations, kernel),
                                  prep.morph_iterated_reference(masks, op, kernel, iterations))


def test_fold_radius_refuses():
    assert prep.fold_radius(5, 5) == 10 and prep.fold_radius(5, 0) == 0 and prep.fold_radius(1, 9) == 0
    for kernel, it in ((4, 1), (0, 1), (5, -1), (5, 17)):
        with pytest.raises(ValueError):
            prep.fold_radius(kernel, it)


@pytest.mark.parametrize("erode_border", [False, True])
def test_band_rule_vs_get_mask(erode_border):
    pytest.importorskip("scipy")
    masks = np.concatenate([cases.mask_stack(37, 70, 7, True), cases.mask_stack(37, 70, 8, False)])
    want = np.stack([cases.get_mask_scipy(m, erode_border) for m in masks])
    got = prep.sampling_masks_reference(masks, 3, 5, erode_border)
    np.testing.assert_array_equal(got, want)
    if erode_border:
        assert (got != prep.sampling_masks_reference(masks, 3, 5, False)).any()  # the band clears something
    flat = prep.sampling_masks_reference(masks.reshape(6, 37 * 70, 1), 3, 5, erode_border, H=37, W=70)
    assert flat.shape == (6, 37 * 70, 1)
    np.testing.assert_array_equal(flat.reshape(6, 37, 70), want)


def test_combine_mode_checker():
    masks = cases.mask_stack(20, 30, 2, True)
    other = (cases.mask_stack(20, 30, 9, False) > 128).astype(np.uint8) * 7
    got = prep.mask_morph_reference(masks, "dilate", 2, other=other)
    want = np.logical_or(other, prep.mask_morph_reference(masks, "dilate", 2)).astype(np.uint8)
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(got)) <= {0, 1}


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_median_checker_vs_numpy(n):
    H, W = 5, 7
    imgs, masks = cases.median_frames(n, H, W, 40 + n)
    cam = np.zeros(n, np.int64)
    want = np.median(imgs.reshape(n, H, W, 3), axis=0).astype(np.uint8)
    np.testing.assert_array_equal(prep.median_backgrounds_reference(imgs, cam, H=H, W=W)[0], want)
    got, counts = prep.median_backgrounds_reference(imgs, cam, masks, H=H, W=W, return_counts=True)
    np.testing.assert_array_equal(got, cases.median_loop(imgs, masks, cam, 1, H, W))
    np.testing.assert_array_equal(counts[0].reshape(-1), (masks == 0).sum(0))


def test_median_checker_cameras():
    """Two cameras of unequal size, interleaved, and an empty third one; a tiny chunk so that the chunking shows."""
    H, W = 5, 7
    imgs, masks = cases.median_frames(7, H, W, 3)
    cam = np.array([1, 0, 1, 1, 0, 1, 1])
    got = prep.median_backgrounds_reference(imgs, cam, masks, n_cams=3, H=H, W=W, chunk=4)
    np.testing.assert_array_equal(got, cases.median_loop(imgs, masks, cam, 3, H, W))
    assert not got[2].any()
    full = prep.median_backgrounds_reference(imgs.reshape(7, H, W, 3), cam, n_cams=3)
    for c in (0, 1):
        np.testing.assert_array_equal(full[c], np.median(imgs[cam == c].reshape(-1, H, W, 3), axis=0).astype(np.uint8))
    order, start = prep.camera_lists(cam, 3)
    assert order.tolist() == [1, 4, 0, 2, 3, 5, 6] and start.tolist() == [0, 2, 7, 7]


@pytest.mark.parametrize("width", [1, 2, 3, 4, 9])
def test_coverage_checker_vs_brute_force(width):
    H, W = 24, 40
    segs = np.array([[[4, 3, 30, 3], [6, 2, 6, 20], [10, 5, 25, 20], [2, 12, 37, 15], [20, 10, 20, 10],
                      [-5, 8, 6, 13], [33, 18, 50, 30], [-30, -30, -10, -20], [12, 22, 14, 1]]], np.int32)
    for b in range(segs.shape[1]):
        got = prep.draw_segments_reference(segs[:, b:b + 1], H, W, width)[0]
        np.testing.assert_array_equal(got.astype(bool), cases.coverage_brute(segs[0, b], H, W, width), err_msg=str(b))
    allb = prep.draw_segments_reference(segs, H, W, width)[0].astype(bool)
    want = np.zeros((H, W), bool)
    for b in range(segs.shape[1]):
        want |= cases.coverage_brute(segs[0, b], H, W, width)
    np.testing.assert_array_equal(allb, want)


def test_paint_checker_order_and_drop():
    H, W = 12, 20
    segs = np.array([[[2, 5, 17, 5], [9, 1, 9, 10], [0, 0, 8193, 0]]], np.int32)
    colors = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    frames = np.full((1, H, W, 3), 50, np.uint8)
    out = prep.draw_segments_reference(segs, H, W, 3, colors, frames)
    assert (frames == 50).all()  # a copy
    assert out[0, 5, 9].tolist() == [4, 5, 6] and out[0, 5, 3].tolist() == [1, 2, 3]  # the higher index wins
    assert out[0, 0, 0].tolist() == [50, 50, 50]  # the segment with an endpoint at 8193 is dropped
    mask = prep.draw_segments_reference(segs, H, W, 3)
    np.testing.assert_array_equal(mask[0] != 0, (out[0] != 50).any(-1))


def test_segments_round_half_to_even_and_drop_non_finite():
    kp = np.zeros((1, 24, 2), np.float32)
    kp[0, 0] = [2.5, 3.5]
    kp[0, 1] = [np.nan, 4.0]
    kp[0, 2] = [1e9, 4.0]
    segs = prep.skeleton_segments_reference(kp, kin.SMPLSkeleton)
    assert segs.dtype == np.int32 and segs.shape == (1, 24, 4)
    assert segs[0, 0].tolist() == [2, 4, 2, 4]  # the root's parent is itself: a disc
    assert abs(segs[0, 1, 0]) > prep.MAX_COORD and abs(segs[0, 2, 0]) > prep.MAX_COORD
    colors = prep.skeleton_colors(kin.SMPLSkeleton)
    assert colors[0].tolist() == [46, 204, 13] and colors[1].tolist() == [100, 149, 237] and colors[2].tolist() == [255, 0, 0]
    assert prep.skeleton_colors(kin.SMPLSkeleton, flip=True)[:3].tolist() == [[128, 0, 128], [0, 128, 128], [128, 128, 0]]


@pytest.mark.parametrize("nj", [24, 17])
def test_projection_checker_vs_frame_loop(nj):
    H, W = 37, 70
    kps, c2ws, focals, centers = cases.skeleton_scene(nj, 3, H, W, 11)
    for f, c, h, w in ((focals, centers, H, W), (focals[:, 0], None, H, W), (55.5, None, H, W),
                       (focals, None, [37, 40, 50], [70, 60, 64])):
        got = prep.skeleton3d_to_2d_reference(kps, c2ws, h, w, f, c)
        want = cases.project_loop(kps, c2ws, h, w, f, c)
        assert got.dtype == np.float64 and got.shape == (3, nj, 2)
        assert np.abs(want).max() < 1e4
        assert np.abs(got - want).max() <= 1e-9


def test_build_compiles_the_unit_on_its_own():
    """anerf_prep.hip is one of build.py's units and reads only the C header; no other unit reads it, so an edit of it
    recompiles one object."""
    build = importlib.import_module("a-nerf_amd.build")
    mine = [s for s in build.SRC if os.path.basename(s) == "anerf_prep.hip"]
    assert len(mine) == 1 and os.path.isfile(mine[0])
    assert build.unit_deps(mine[0]) == [mine[0], build.HEADER]
    for src in build.SRC:
        if src != mine[0]:
            assert mine[0] not in build.unit_deps(src)
    text = open(mine[0]).read()
    assert [ln for ln in text.splitlines() if ln.startswith("#include \"")] == ['#include "../../include/anerf.h"']


def test_signatures_hold_the_new_entries():
    for name, nargs in (("anerf_mask_morph", 10), ("anerf_draw_segments", 10), ("anerf_background_median", 12)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "anerf.h")).read()
    for name, value in (("ANERF_PREP_MAX_RADIUS", _lib.ANERF_PREP_MAX_RADIUS), ("ANERF_PREP_MAX_DIM", _lib.ANERF_PREP_MAX_DIM),
                        ("ANERF_PREP_MAX_SEGMENTS", _lib.ANERF_PREP_MAX_SEGMENTS),
                        ("ANERF_PREP_MAX_COORD", _lib.ANERF_PREP_MAX_COORD), ("ANERF_PREP_MAX_WIDTH", _lib.ANERF_PREP_MAX_WIDTH)):
        assert f"#define {name} {value}" in src
    assert "#define ANERF_PREP_MAX_CAMERA_FRAMES (1 << 20)" in src and _lib.ANERF_PREP_MAX_CAMERA_FRAMES == 1 << 20
    assert _lib.ANERF_PREP_MAX_CAMERA_FRAMES >= 1 << 20 and "#define ANERF_ABI_VERSION 26" in src

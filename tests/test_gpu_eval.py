"""Frame scoring on the GPU (csrc/anerf_eval.hip, a-nerf_amd/evaluation.py) against the float64 checker.

Frames are 48 x 40 (rows x columns) and 33 x 70: with the kernel's 32 x 16 tile a 70-pixel row spans three tiles, the
last ragged, and both heights leave a ragged last tile row.  Bounds (tests/_eval_cases.py): the map within 2^-22 of
the checker (one fp32 ulp at 1, times two: the kernel rounds its double map once), per-frame SSIM within 1e-9 and
PSNR within 1e-9 dB (both sides are float64 sums in different orders)."""
import ctypes
import importlib
import types

import numpy as np
import pytest
import torch

import _eval_cases as cases

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
syn = importlib.import_module("a-nerf_amd.synthetic")
_lib = importlib.import_module("a-nerf_amd._lib")

H, W = 48, 40
# x0, y0, x1, y1: the whole frame, an interior box, 7 x 9 (narrower than the window), 1 x 1, empty, two edges
RECTS = [(0, 0, 40, 48), (3, 5, 38, 44), (20, 10, 27, 19), (11, 13, 12, 14), (9, 9, 9, 20), (25, 30, 40, 48)]
BOXES = [((r[0], r[1]), (r[2], r[3])) for r in RECTS]
RECTS_70 = [(0, 0, 70, 33), (30, 2, 70, 33), (1, 1, 66, 17)]


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_checked = {}


def _checker(h, w, n, mask_kind, crop, data_range, border):
    """The float64 checker's scores for a case, computed once and shared."""
    key = (h, w, n, mask_kind, crop, data_range, border)
    if key not in _checked:
        c = cases.make_case(h, w, 5, n)
        _checked[key] = anerf.evaluate_frames_reference(c["pred"], c["gt"], masks=_masks(c, mask_kind),
                                                        bboxes=_boxes(h), crop=crop, data_range=data_range,
                                                        border=border, return_map=True)
    return _checked[key]


def _boxes(h):
    return BOXES if h == H else [((r[0], r[1]), (r[2], r[3])) for r in RECTS_70]


def _masks(c, kind):
    if kind == "none":
        return None
    m = np.array(c["mask"])
    if kind == "ones":
        m[:] = 1
    if kind == "one_empty":
        m[1] = 0
    return m


def _compare(got, want, n):
    assert np.array_equal(got.sums[:, [0, 3, 6]], want.sums[:, [0, 3, 6]])  # the pixel counts, exactly
    for k in ("psnr", "ssim", "fg_psnr", "fg_ssim", "valid_psnr", "valid_ssim"):
        d = np.abs(getattr(got, k) - getattr(want, k)).max()
        print(f"{k}: max |gpu - checker| = {d:.3e}")
        assert d <= cases.SCORE_TOL, k
    for i in range(n):
        d = np.abs(got.map[i].cpu().numpy().astype(np.float64) - want.map[i]).max()
        assert d <= cases.MAP_TOL, (i, d)


@pytest.mark.parametrize("mask_kind", ["none", "partial"])
@pytest.mark.parametrize("crop", [True, False])  # boxes NULL (the box is the rectangle) / given (a second weight)
@pytest.mark.parametrize("data_range", [1.0, 255.0])
@pytest.mark.parametrize("border", ["same", "valid"])
def test_sweep_against_the_checker(border, data_range, crop, mask_kind):
    n = len(RECTS)
    c = cases.make_case(H, W, 5, n)
    got = anerf.evaluate_frames(torch.from_numpy(np.array(c["pred"])).cuda(), c["gt_u8"], masks=_masks(c, mask_kind),
                                bboxes=BOXES, crop=crop, data_range=data_range, border=border, return_map=True)
    want = _checker(H, W, n, mask_kind, crop, data_range, border)
    _compare(got, want, n)
    empty = RECTS.index((9, 9, 9, 20))
    if crop:
        assert not got.sums[empty].any() and got.psnr[empty] == 0.0
        if border == "valid":  # narrower than the window: nothing is scored
            assert not got.sums[RECTS.index((20, 10, 27, 19))].any()
    else:
        assert not got.sums[empty, 6:].any()


@pytest.mark.parametrize("crop", [True, False])
@pytest.mark.parametrize("border", ["same", "valid"])
def test_ragged_tiles_33_by_70(border, crop):
    n = len(RECTS_70)
    c = cases.make_case(33, 70, 5, n)
    got = anerf.evaluate_frames(c["pred"], c["gt"], masks=c["mask"], bboxes=_boxes(33), crop=crop, border=border,
                                return_map=True)
    _compare(got, _checker(33, 70, n, "partial", crop, 1.0, border), n)


def test_frames_of_two_sizes_in_one_call():
    a, b = cases.make_case(H, W, 5, 2), cases.make_case(33, 70, 5, 1)
    got = anerf.evaluate_frames([a["pred"][0], b["pred"][0], a["pred"][1]], [a["gt_u8"][0], b["gt_u8"][0], a["gt_u8"][1]])
    for i, (c, k) in enumerate(((a, 0), (b, 0), (a, 1))):
        one = anerf.evaluate_frames(c["pred"][k], c["gt_u8"][k])
        assert np.array_equal(got.sums[i], one.sums[0])


def test_uint8_and_float_ground_truth_are_bit_identical():
    c = cases.make_case(H, W, 5, len(RECTS))
    a = anerf.evaluate_frames(c["pred"], c["gt_u8"], masks=c["mask"], bboxes=BOXES, crop=True, return_map=True)
    b = anerf.evaluate_frames(c["pred"], c["gt"], masks=c["mask"], bboxes=BOXES, crop=True, return_map=True)
    assert np.array_equal(a.sums, b.sums)
    assert all(torch.equal(x, y) for x, y in zip(a.map, b.map))


def test_all_ones_mask_and_an_empty_mask():
    n = len(RECTS)
    c = cases.make_case(H, W, 5, n)
    ones = anerf.evaluate_frames(c["pred"], c["gt_u8"], masks=_masks(c, "ones"), bboxes=BOXES, crop=True)
    assert np.array_equal(ones.sums[:, 3:6], ones.sums[:, 0:3])
    assert np.array_equal(ones.fg_psnr, ones.psnr) and np.array_equal(ones.fg_ssim, ones.ssim)
    part = anerf.evaluate_frames(c["pred"], c["gt_u8"], masks=c["mask"], bboxes=BOXES, crop=True)
    hole = anerf.evaluate_frames(c["pred"], c["gt_u8"], masks=_masks(c, "one_empty"), bboxes=BOXES, crop=True)
    assert hole.n_fg[1] == 0 and hole.fg_psnr[1] == 0.0 and hole.fg_ssim[1] == 0.0
    keep = np.arange(n) != 1
    assert np.array_equal(hole.sums[keep], part.sums[keep])
    assert np.array_equal(hole.sums[1, [0, 1, 2, 6, 7, 8]], part.sums[1, [0, 1, 2, 6, 7, 8]])
    _compare(anerf.evaluate_frames(c["pred"], c["gt_u8"], masks=_masks(c, "one_empty"), bboxes=BOXES, crop=True,
                                   return_map=True), _checker(H, W, n, "one_empty", True, 1.0, "same"), n)


@pytest.mark.parametrize("data_range", [1.0, 255.0])
def test_identical_frames_score_exactly_one(data_range):
    c = cases.make_case(H, W, 5, len(RECTS))
    got = anerf.evaluate_frames(c["gt"], c["gt_u8"], masks=c["mask"], bboxes=BOXES, crop=True, data_range=data_range,
                                return_map=True)
    for i, (x0, y0, x1, y1) in enumerate(RECTS):
        m = got.map[i].cpu().numpy()
        inside = np.zeros((H, W), bool)
        inside[y0:y1, x0:x1] = True
        assert (m[inside] == 1.0).all() and not m[~inside].any()
    assert not got.sums[:, [1, 4, 7]].any()  # sum se is exactly 0
    assert np.array_equal(got.sums[:, 2], 3.0 * got.sums[:, 0])
    assert not got.psnr.any() and not got.fg_psnr.any()  # the reference's inf -> 0


def test_sums_are_bit_identical_across_calls_and_launch_shapes():
    n = len(RECTS)
    c = cases.make_case(H, W, 5, n)
    kw = dict(crop=True, border="same")
    a = anerf.evaluate_frames(c["pred"], c["gt_u8"], masks=c["mask"], bboxes=BOXES, **kw)
    b = anerf.evaluate_frames(c["pred"], c["gt_u8"], masks=c["mask"], bboxes=BOXES, **kw)
    assert np.array_equal(a.sums, b.sums)
    for i in range(n):
        one = anerf.evaluate_frames(c["pred"][i:i + 1], c["gt_u8"][i:i + 1], masks=c["mask"][i:i + 1],
                                    bboxes=BOXES[i:i + 1], **kw)
        assert np.array_equal(one.sums[0], a.sums[i]), i


def test_evaluate_frames_reads_the_device_once():
    """Frames, ground truth and masks in HBM, two frame sizes (two launches): one synchronising read, the sums --
    counted by torch's synchronisation debug mode after a warm-up call."""
    import warnings
    a, b = cases.make_case(H, W, 5, 2), cases.make_case(33, 70, 5, 1)
    dev = [[torch.from_numpy(np.array(c[k][i])).cuda() for c, i in ((a, 0), (b, 0), (a, 1))]
           for k in ("pred", "gt_u8", "mask")]
    want = anerf.evaluate_frames(*dev[:2], masks=dev[2], return_map=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            got = anerf.evaluate_frames(*dev[:2], masks=dev[2], return_map=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]
    print("\nsynchronising calls in evaluate_frames:", len(syncs), syncs)
    assert len(syncs) == 1, syncs
    assert np.array_equal(got.sums, want.sums) and all(m.is_cuda for m in got.map)


def test_more_frames_than_one_launch_takes():
    """65 frames: the rectangles travel 64 per launch.  Frame 64 equals the same frame scored alone."""
    c = cases.make_case(H, W, 5, len(RECTS))
    idx = [i % len(RECTS) for i in range(65)]
    got = anerf.evaluate_frames(c["pred"][idx], c["gt_u8"][idx], masks=c["mask"][idx], bboxes=[BOXES[i] for i in idx],
                                crop=True, return_map=True)
    base = anerf.evaluate_frames(c["pred"], c["gt_u8"], masks=c["mask"], bboxes=BOXES, crop=True, return_map=True)
    assert np.array_equal(got.sums, base.sums[idx])
    assert torch.equal(got.map[64], base.map[idx[64]]) and torch.equal(got.map[63], base.map[idx[63]])


def _raw(pred, gt, sums, rects, boxes=None, n=1, h=H, w=W, data_range=1.0, border=0, mp=None, mask=None,
         ws="own", ws_bytes=None):
    """anerf_eval_frames itself.  ws: "own" (as asked for), None, "misaligned"; ws_bytes: what the call is told."""
    lib = _lib.load()
    need = _lib.workspace("anerf_eval_workspace", max(n, 0), max(h, 0), max(w, 0))
    buf = torch.empty(need + 8, device="cuda", dtype=torch.uint8)
    wp = {"own": ctypes.c_void_p(buf.data_ptr()), None: None, "misaligned": ctypes.c_void_p(buf.data_ptr() + 4)}[ws]
    r = None if rects is None else np.ascontiguousarray(rects, np.int32)
    b = None if boxes is None else np.ascontiguousarray(boxes, np.int32)
    return lib.anerf_eval_frames(_lib.ptr(pred), _lib.ptr(gt), 0, _lib.ptr(mask),
                                 None if r is None else r.ctypes.data_as(_lib.c_i32p),
                                 None if b is None else b.ctypes.data_as(_lib.c_i32p), n, h, w, float(data_range),
                                 border, _lib.ptr(mp), _lib.ptr(sums), wp, need if ws_bytes is None else ws_bytes,
                                 _lib.stream_handle())


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    pred = torch.rand(1, H, W, 3, device="cuda")
    gt = torch.rand(1, H, W, 3, device="cuda")
    sums = torch.full((1, 9), -7.0, device="cuda", dtype=torch.float64)
    mp = torch.full((1, H, W, 3), -7.0, device="cuda")
    whole = [[0, 0, W, H]]
    bad = [
        dict(pred=None), dict(gt=None), dict(sums=None),
        dict(n=-1), dict(h=-1), dict(w=-1),
        dict(rects=[[0, 0, W + 1, H]]), dict(rects=[[0, 0, W, H + 1]]), dict(rects=[[-1, 0, W, H]]),
        dict(rects=[[0, -1, W, H]]), dict(rects=[[5, 0, 4, H]]), dict(rects=[[0, 5, W, 4]]),
        dict(boxes=[[0, 0, W + 1, H]]), dict(boxes=[[-1, 0, W, H]]), dict(boxes=[[5, 0, 4, H]]),
        dict(border=2), dict(border=-1),
        dict(data_range=0.0), dict(data_range=-1.0), dict(data_range=float("nan")),
        dict(rects=None), dict(ws=None), dict(ws="misaligned"),
        dict(ws_bytes=8),  # too small: ANERF_EWORKSPACE
    ]
    for case in bad:
        args = dict(pred=pred, gt=gt, sums=sums, rects=whole, mp=mp)
        args.update(case)
        rc = _raw(**args)
        assert rc == (-3 if "ws_bytes" in case else -1), case
        assert lib.anerf_last_error().decode().startswith("anerf_eval_frames: "), case
    assert _lib.load().anerf_eval_workspace(-1, H, W) == 0 and lib.anerf_last_error()
    torch.cuda.synchronize()
    assert bool((sums == -7.0).all()) and bool((mp == -7.0).all())
    assert _raw(pred, gt, sums, whole, mp=mp) == 0  # (and the good call writes both)
    torch.cuda.synchronize()
    assert sums[0, 0].item() == H * W and bool((mp != -7.0).all())


@pytest.mark.parametrize("border", [0, 1])
def test_a_rectangle_with_a_separate_box(border):
    """The C ABI takes a box that is not the rectangle (the Python wrapper passes one or the other): the box's sums
    are the checker's map and squared error over rectangle x box, with a mask on top."""
    c = cases.make_case(H, W, 5, 2)
    rects, boxes = [RECTS[1], RECTS[5]], [[10, 0, 33, 20], [0, 35, 40, 48]]  # overlapping / partly outside
    want = anerf.evaluate_frames_reference(c["pred"], c["gt"], masks=c["mask"], bboxes=[BOXES[1], BOXES[5]], crop=True,
                                           border=("same", "valid")[border], return_map=True)
    pred, gt = torch.from_numpy(np.array(c["pred"])).cuda(), torch.from_numpy(np.array(c["gt"])).cuda()
    mask = torch.from_numpy(np.array(c["mask"])).cuda()
    sums = torch.empty(2, 9, device="cuda", dtype=torch.float64)
    assert _raw(pred, gt, sums, rects, boxes=boxes, n=2, border=border, mask=mask) == 0
    got = sums.cpu().numpy()
    se = (c["gt"].astype(np.float64) - c["pred"].astype(np.float64)) ** 2
    s = 5 * border
    for f, ((x0, y0, x1, y1), (bx0, by0, bx1, by1)) in enumerate(zip(rects, boxes)):
        wt = np.zeros((H, W), bool)
        wt[max(y0 + s, by0):min(y1 - s, by1), max(x0 + s, bx0):min(x1 - s, bx1)] = True
        assert wt.any()
        assert got[f, 6] == wt.sum()
        assert abs(got[f, 7] - se[f][wt].sum()) <= 1e-12 * wt.sum()
        assert abs(got[f, 8] - want.map[f][wt].sum()) <= 1e-12 * wt.sum()
    assert np.abs(got[:, :6] - want.sums[:, :6]).max() <= 1e-9


def test_box_metric_trims_1002_row_images_on_the_device():
    """The h36m case (tests/test_eval_host.py): 1002-row images against a 1000-row render, 63 tile rows."""
    from test_eval_host import h36m_case
    rgbs, boxes, gd, _ = h36m_case()
    got = anerf.evaluate_box_metric(torch.from_numpy(rgbs).cuda(), None, boxes, gd)
    want = anerf.evaluate_box_metric(rgbs, None, boxes, gd, backend=anerf.evaluate_frames_reference)
    for k in want:
        assert len(got[k]) == 1 and abs(got[k][0] - want[k][0]) <= cases.SCORE_TOL, k


def test_new_symbols_and_the_abi_version():
    lib = _lib.load()
    assert lib.anerf_abi_version() == 26
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("anerf_eval_workspace", "anerf_eval_frames"):
        assert hasattr(cdll, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["anerf_eval_workspace"] == (ctypes.c_size_t, [ctypes.c_int32] * 3)
    assert len(_lib.SIGNATURES["anerf_eval_frames"][1]) == 16
    assert lib.anerf_eval_workspace(3, 33, 70) == 3 * 3 * 3 * 9 * 8  # 3 frames x (3 x 3 tiles) x 9 doubles


def test_render_testset_end_to_end():
    """render_testset on a synthetic scene: the frames it returns have render_path's bits, its metrics are
    evaluate_metric's with the checker on the downloaded frames, and evaluate_box_metric agrees with its checker."""
    sc = syn.make_scene(n_joints=24, H=64, W=64, seed=3, n_frames=2, yaw_step=0.7)
    cfg = anerf.RenderConfig(n_joints=24, netdepth=4, netwidth=128, N_samples=32, N_importance=0).validate()
    ck = syn.make_checkpoint(11, n_joints=24, D=4, W=128, fine=False, tau=20.0)
    kw = {"ray_caster": anerf.RayCaster(cfg, ck, device=0), "N_samples": 32, "N_importance": 0, "perturb": False,
          "raw_noise_std": 0., "ray_noise_std": 0., "use_viewdirs": True, "preproc_kwargs": {"density_scale": 1.0},
          "lindisp": False}
    args = types.SimpleNamespace(chunk=4096 * 8, render_factor=0, ext_scale=0.001, white_bkgd=False)
    poses, hwf = torch.from_numpy(sc["c2ws"]), (64, 64, sc["focal"])
    kp, skts = torch.from_numpy(sc["kps"]), torch.from_numpy(sc["skts"])
    rgbs0, disps0, accs0, _, bbs = anerf.render_path(poses, hwf, args.chunk // 8, kw, kp=kp, skts=skts, ret_acc=True,
                                                     ext_scale=0.001)
    d0 = np.where(np.isnan(disps0), np.float32(0), disps0)  # (run_nerf.py:140-141)
    rng = np.random.default_rng(9)
    gt_u8 = np.clip(np.round((rgbs0 + 0.05 * rng.standard_normal(rgbs0.shape)) * 255.0), 0, 255).astype(np.uint8)
    masks = (accs0[..., 0] > 0.05).astype(np.uint8)
    assert masks.reshape(2, -1).any(-1).all()
    # the ground truth as RayImageDataset holds it: uint8 [F][H*W][3] and [F][H*W] in HBM
    gt_dev, mask_dev = torch.from_numpy(gt_u8).cuda().reshape(2, -1, 3), torch.from_numpy(masks).cuda().reshape(2, -1)
    for both in (False, True):
        metrics, rgbs, disps = anerf.render_testset(poses, hwf, args, kw, kps=kp, skts=skts, gt_imgs=gt_dev,
                                                    gt_masks=mask_dev, eval_metrics=True, eval_both=both)
        assert np.array_equal(rgbs, rgbs0) and np.array_equal(disps, d0 / d0.max())
        want = anerf.evaluate_metric(rgbs, gt_u8, gt_masks=masks, bboxes=bbs, hwf=hwf, eval_both=both,
                                     backend=anerf.evaluate_frames_reference)
        for k in ("psnr", "ssim", "psnr_fg", "ssim_fg"):
            assert abs(metrics[k] - want[k]) <= cases.SCORE_TOL, (both, k, metrics[k], want[k])
    metrics, rgbs, _ = anerf.render_testset(poses, hwf, args, kw, kps=kp, skts=skts)
    assert metrics == {"psnr": None, "ssim": None} and np.array_equal(rgbs, rgbs0)
    gd = {"gt_paths": [g.reshape(-1) for g in gt_u8], "gt_mask_paths": [m.reshape(-1) for m in masks],
          "is_gt_paths": False, "bg_imgs": None, "bg_indices": None}
    got = anerf.evaluate_box_metric(torch.from_numpy(rgbs0).cuda(), None, bbs, gd)
    want = anerf.evaluate_box_metric(rgbs0, None, bbs, gd, backend=anerf.evaluate_frames_reference)
    for k in ("psnr", "ssim", "fg_psnr", "fg_ssim"):
        assert len(got[k]) == 2 and np.abs(np.asarray(got[k]) - np.asarray(want[k])).max() <= cases.SCORE_TOL, k

"""Dataset preparation on the GPU (csrc/anerf_prep.hip, a-nerf_amd/preprocess.py): every kernel bit-identical to its
NumPy checker, which tests/test_prep_host.py holds to scipy, np.median and a brute force."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prep_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
anerf = importlib.import_module("a-nerf_amd")
prep = importlib.import_module("a-nerf_amd.preprocess")
_lib = importlib.import_module("a-nerf_amd._lib")
kin = importlib.import_module("a-nerf_amd.kinematics")
syn = importlib.import_module("a-nerf_amd.synthetic")
SHAPES = [(37, 70), (33, 16)]  # ragged 64 x 32 tiles in both directions; a row of 70 spans two tiles


def _np(t):
    return t.detach().cpu().numpy()


def _stacks(H, W):
    flat = np.stack([np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8), cases.mask_stack(H, W, 1, True)[1]])
    return {"binary": cases.mask_stack(H, W, 1, True), "bytes": cases.mask_stack(H, W, 2, False), "flat": flat}


# ---------------------------------------------------------------- morphology
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("op", ["dilate", "erode"])
def test_morphology_vs_checker(op, H, W):
    """All-zero, all-one, corner pixels, blobs, stripes and random bytes at every radius, 32 above either half side."""
    for name, masks in _stacks(H, W).items():
        dev = torch.from_numpy(masks).cuda()
        for radius in (0, 1, 2, 6, 10, 32):
            got = prep.mask_morph(dev, op, radius)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == masks.shape
            np.testing.assert_array_equal(_np(got), prep.mask_morph_reference(masks, op, radius),
                                          err_msg=f"{name} radius {radius}")
        np.testing.assert_array_equal(_np(dev), masks)  # the source is not written


@pytest.mark.parametrize("H,W", SHAPES)
def test_named_morphology_and_layouts(H, W):
    masks = cases.mask_stack(H, W, 4, True)
    for fn, ref in ((anerf.dilate_masks, anerf.dilate_masks_reference), (anerf.erode_masks, anerf.erode_masks_reference)):
        np.testing.assert_array_equal(_np(fn(masks, 5)), ref(masks, 5))  # a NumPy input: uploaded, radius 10
        np.testing.assert_array_equal(_np(fn(masks, extend_iter=2, kernel=3)), ref(masks, 2, 3))
    four = masks[..., None]
    got = anerf.dilate_masks(torch.from_numpy(four).cuda(), 1)
    assert tuple(got.shape) == four.shape
    np.testing.assert_array_equal(_np(got), anerf.dilate_masks_reference(four, 1))
    flat = masks.reshape(3, H * W, 1)  # the dataset's layout
    got = anerf.dilate_masks(flat, 3, H=H, W=W)
    assert tuple(got.shape) == flat.shape
    np.testing.assert_array_equal(_np(got).reshape(3, H, W), anerf.dilate_masks_reference(masks, 3))


@pytest.mark.parametrize("H,W", SHAPES)
def test_sampling_and_combine_modes(H, W):
    for name, masks in _stacks(H, W).items():
        got = prep.mask_morph(masks, "dilate", 6, band=2)  # sampling mode
        np.testing.assert_array_equal(_np(got), prep.mask_morph_reference(masks, "dilate", 6, band=2), err_msg=name)
        np.testing.assert_array_equal(_np(anerf.sampling_masks(masks, 3, 5, True)), _np(got), err_msg=name)
        np.testing.assert_array_equal(_np(anerf.sampling_masks(masks, 3, 5, False)),
                                      prep.mask_morph_reference(masks, "dilate", 6), err_msg=name)
        other = (cases.mask_stack(H, W, 9, False) > 200).astype(np.uint8) * 3
        for op, radius in (("dilate", 2), ("erode", 1), ("dilate", 0)):
            got = prep.mask_morph(masks, op, radius, other=other)  # combine mode
            want = prep.mask_morph_reference(masks, op, radius, other=other)
            np.testing.assert_array_equal(_np(got), want, err_msg=name)
            np.testing.assert_array_equal(want, np.logical_or(other, prep.mask_morph_reference(masks, op, radius))
                                          .astype(np.uint8))
    binary = _stacks(H, W)["binary"]
    assert (prep.mask_morph_reference(binary, "dilate", 6, band=2) != prep.mask_morph_reference(binary, "dilate", 6)).any()


def test_morphology_refusals():
    lib = _lib.load()
    src = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    dst = torch.full_like(src, 9)
    st = _lib.stream_handle()

    def call(s=src, d=dst, n=2, H=8, W=8, op=0, radius=1, band=0):
        return lib.anerf_mask_morph(_lib.ptr(s), _lib.ptr(d), n, H, W, op, radius, band, None, st)

    assert call() == 0
    for kw, word in ((dict(radius=33), b"radius"), (dict(radius=-1), b"radius"), (dict(s=None), b"NULL"),
                     (dict(d=None), b"NULL"), (dict(H=0), b"H and W"), (dict(W=0), b"H and W"),
                     (dict(H=32769), b"H and W"), (dict(W=32769), b"H and W"), (dict(op=2), b"unknown operation"),
                     (dict(op=-1), b"unknown operation"), (dict(band=33), b"band"), (dict(op=1, band=1), b"band"),
                     (dict(d=src), b"dst must not be src"), (dict(n=-1), b"n_masks")):
        dst.fill_(9)
        assert call(**kw) == -1, kw
        msg = lib.anerf_last_error()
        assert b"anerf_mask_morph" in msg and word in msg, (kw, msg)
        if kw.get("d", dst) is dst:
            assert int(dst.min()) == 9  # nothing was launched
    assert call(n=0) == 0
    with pytest.raises(ValueError):
        anerf.dilate_masks(src, 17)


# ---------------------------------------------------------------- segments
@pytest.mark.parametrize("width", [1, 3, 4, 9])
def test_segments_vs_checker(width):
    H, W = 37, 70
    segs = cases.segment_frames(H, W)
    got = prep.draw_segments(segs, H, W, width)
    want = prep.draw_segments_reference(segs, H, W, width)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, H, W)
    np.testing.assert_array_equal(_np(got), want)
    assert want[0].any() and want[1].any()
    # the dropped segments of frame 2 (an endpoint at +-8193) leave the rest of the frame as frame 0 without them
    keep = [b for b in range(segs.shape[1]) if b not in (1, 3)]
    np.testing.assert_array_equal(want[2], prep.draw_segments_reference(segs[:1, keep], H, W, width)[0])
    # paint: on a background that differs from every colour, the mask is paint != background
    colors = np.random.RandomState(0).randint(1, 255, (segs.shape[1], 3)).astype(np.uint8)
    colors[10], colors[11] = (9, 9, 9), (200, 100, 50)  # the overlapping pair
    back = np.random.RandomState(1).randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    for frames in (np.full((3, H, W, 3), 255, np.uint8), back):
        dev = torch.from_numpy(frames).cuda()
        out = prep.draw_segments(segs, H, W, width, colors, dev)
        assert out.data_ptr() == dev.data_ptr()  # in place
        wantp = prep.draw_segments_reference(segs, H, W, width, colors, frames)
        np.testing.assert_array_equal(_np(out), wantp)
        np.testing.assert_array_equal(_np(out)[want == 0], frames[want == 0])  # uncovered bytes untouched
    white = torch.full((3, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    np.testing.assert_array_equal(_np(got) != 0, (_np(prep.draw_segments(segs, H, W, width, colors, white)) != 255).any(-1))
    # segments 10 (horizontal) and 11 (vertical) cross at (30, 14): the higher index wins
    assert wantp[0, 14, 30].tolist() == [200, 100, 50] and wantp[0, 14, 22].tolist() == [9, 9, 9]


def test_segment_refusals():
    lib = _lib.load()
    segs = torch.zeros(1, 2, 4, dtype=torch.int32, device="cuda")
    mask = torch.empty(1, 8, 8, dtype=torch.uint8, device="cuda")
    frames = torch.empty(1, 8, 8, 3, dtype=torch.uint8, device="cuda")
    st = _lib.stream_handle()
    assert lib.anerf_draw_segments(_lib.ptr(segs), 1, 2, 8, 8, 3, None, _lib.ptr(mask), None, st) == 0
    for args in ((_lib.ptr(segs), 1, 2, 8, 8, 3, None, None, None), (_lib.ptr(segs), 1, 2, 8, 8, 3, None, None, _lib.ptr(frames)),
                 (_lib.ptr(segs), 1, 129, 8, 8, 3, None, _lib.ptr(mask), None), (None, 1, 2, 8, 8, 3, None, _lib.ptr(mask), None),
                 (_lib.ptr(segs), 1, 2, 8193, 8, 3, None, _lib.ptr(mask), None), (_lib.ptr(segs), 1, 2, 8, 0, 3, None, _lib.ptr(mask), None),
                 (_lib.ptr(segs), 1, 2, 8, 8, 0, None, _lib.ptr(mask), None), (_lib.ptr(segs), 1, 2, 8, 8, 4097, None, _lib.ptr(mask), None),
                 (_lib.ptr(segs), -1, 2, 8, 8, 3, None, _lib.ptr(mask), None)):
        assert lib.anerf_draw_segments(*args, st) == -1, args
        assert b"anerf_draw_segments" in lib.anerf_last_error()


@pytest.mark.parametrize("nj", [24, 17])
def test_skeletons_end_to_end(nj):
    """kp3d -> skeleton3d_to_2d -> segments -> overlay and keypoint masks, F = 3 frames of 37 x 70."""
    H, W = 37, 70
    skel = kin.SMPLSkeleton if nj == 24 else kin.CanonicalSkeleton
    kps, c2ws, focals, centers = cases.skeleton_scene(nj, 3, H, W, 11)
    want2d = prep.skeleton3d_to_2d_reference(kps, c2ws, H, W, focals, centers)
    plain2d = prep.skeleton3d_to_2d_reference(kps, c2ws, H, W, focals)  # (what create_kp_masks projects: no centers)
    par = np.asarray(skel.joint_trees)
    for p2d in (want2d, plain2d):
        ends = np.concatenate([p2d, p2d + (p2d[:, par] - p2d)], -1)
        assert np.abs((ends - np.floor(ends)) - 0.5).min() > 1e-6  # no coordinate next to a half: both sides round alike
    got2d = anerf.skeleton3d_to_2d(kps, c2ws, H, W, focals, centers)
    assert got2d.is_cuda and got2d.dtype == torch.float64
    assert np.abs(_np(got2d) - want2d).max() <= 1e-9
    np.testing.assert_array_equal(_np(prep.skeleton_segments(got2d, skel)), prep.skeleton_segments_reference(want2d, skel))
    imgs = np.random.RandomState(3).randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    dev = torch.from_numpy(imgs).cuda()
    for width, flip in ((3, False), (1, True), (4, False), (9, False)):
        out = anerf.draw_skeletons_3d(dev, kps, c2ws, H, W, focals, centers, width=width, flip=flip, skel_type=skel)
        want = anerf.draw_skeletons_3d_reference(imgs, kps, c2ws, H, W, focals, centers, width, flip, skel)
        np.testing.assert_array_equal(_np(out), want)
        assert (want != imgs).any()
    np.testing.assert_array_equal(_np(dev), imgs)  # the result is a copy
    one = anerf.draw_skeleton2d(imgs[1], want2d[1], None if nj == 24 else skel)
    np.testing.assert_array_equal(_np(one), anerf.draw_skeletons_reference(imgs[1:2], want2d[1:2], skel)[0])
    # keypoint masks, from 3-D key points (no centers: create_kp_masks projects with hwf alone) and from 2-D ones
    masks = cases.mask_stack(H, W, 6, True)[..., None]
    for it in (1, 3):
        got = anerf.create_kp_masks(masks, kp3ds=kps, c2ws=c2ws, hwf=(H, W, focals), extend_iter=it, skel_type=skel)
        want = anerf.create_kp_masks_reference(masks, kp3ds=kps, c2ws=c2ws, hwf=(H, W, focals), extend_iter=it,
                                               skel_type=skel)
        assert tuple(got.shape) == masks.shape and set(np.unique(want)) == {0, 1}
        np.testing.assert_array_equal(_np(got), want)
        assert (want >= masks).all() and (want > masks).any()
    got = anerf.create_kp_mask(masks[0], want2d[0], H, W, skel_type=skel)
    np.testing.assert_array_equal(_np(got), anerf.create_kp_masks_reference(masks[:1], kp2ds=want2d[:1], skel_type=skel)[0])


# ---------------------------------------------------------------- medians
def test_medians_vs_checker():
    """5 x 7 pixels; lists of 1, 2, 5 and 8 frames in one call (cameras 0..3) and an empty camera 4."""
    H, W = 5, 7
    imgs, masks = cases.median_frames(16, H, W, 21)
    cam = np.array([3, 0, 3, 2, 1, 3, 2, 3, 1, 2, 3, 2, 3, 3, 2, 3])
    assert np.bincount(cam).tolist() == [1, 2, 5, 8]
    for m in (None, masks):
        got, counts = anerf.median_backgrounds(imgs, cam, m, n_cams=5, H=H, W=W, return_counts=True)
        want, wcounts = anerf.median_backgrounds_reference(imgs, cam, m, n_cams=5, H=H, W=W, return_counts=True)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (5, H, W, 3) and counts.dtype == torch.int32
        np.testing.assert_array_equal(_np(got), want)
        np.testing.assert_array_equal(_np(counts), wcounts)
        assert not want[4].any() and not wcounts[4].any()
        again = anerf.median_backgrounds(torch.from_numpy(imgs).cuda().reshape(16, H, W, 3), cam, m, n_cams=5)
        assert torch.equal(again, got)  # the same bits on a second run, from the (N, H, W, 3) layout
    assert set(np.unique(wcounts[3])) >= {0, 1, 2, 8}
    for c in range(4):  # without masks: np.median
        np.testing.assert_array_equal(_np(anerf.median_backgrounds(imgs, cam, n_cams=5, H=H, W=W))[c],
                                      np.median(imgs[cam == c].reshape(-1, H, W, 3), axis=0).astype(np.uint8))


@pytest.mark.parametrize("n,H,W", [(300, 6, 5), (70000, 2, 3)])
def test_median_counters_are_wide(n, H, W):
    """More frames than a byte-wide (300) or a 16-bit (70,000) counter holds; few distinct values so that the counts
    at a value pass 255 and 65,535."""
    rs = np.random.RandomState(n)
    imgs = rs.choice(np.array([3, 4, 250], np.uint8), size=(n, H * W, 3), p=[0.49, 0.02, 0.49])
    masks = (rs.uniform(size=(n, H * W)) < 0.02).astype(np.uint8)
    cam = np.zeros(n, np.int64)
    for m in (None, masks):
        got, counts = anerf.median_backgrounds(imgs, cam, m, H=H, W=W, return_counts=True)
        want, wcounts = anerf.median_backgrounds_reference(imgs, cam, m, H=H, W=W, return_counts=True)
        np.testing.assert_array_equal(_np(got), want)
        np.testing.assert_array_equal(_np(counts), wcounts)
    assert wcounts.min() > (255 if n == 300 else 65535)


def test_median_refusals():
    lib = _lib.load()
    imgs = torch.zeros(2, 4, 3, dtype=torch.uint8, device="cuda")
    out = torch.empty(1, 4, 3, dtype=torch.uint8, device="cuda")
    st = _lib.stream_handle()
    i32 = _lib.c_i32p

    def call(order, start, n_imgs=2, n_pixels=4, n_cams=1, im=imgs, o=out):
        order, start = np.asarray(order, np.int32), np.asarray(start, np.int32)
        od, sd = torch.from_numpy(order[:8].copy()).cuda(), torch.from_numpy(start).cuda()
        return lib.anerf_background_median(_lib.ptr(im), None, n_imgs, n_pixels, order.ctypes.data_as(i32),
                                           start.ctypes.data_as(i32), _lib.ptr(od), _lib.ptr(sd), n_cams, _lib.ptr(o),
                                           None, st)

    assert call([0, 1], [0, 2]) == 0
    limit = _lib.ANERF_PREP_MAX_CAMERA_FRAMES
    assert limit >= 1 << 20
    assert call(np.zeros(limit + 1, np.int32), [0, limit + 1]) == -1  # a list longer than the declared limit
    assert b"limit" in lib.anerf_last_error()
    for args, kw in ((([0, 2], [0, 2]), {}), (([0, -1], [0, 2]), {}), (([0, 1], [1, 2]), {}), (([0, 1], [0, 2, 1]), dict(n_cams=2)),
                     (([0, 1], [0, 2]), dict(n_pixels=0)), (([0, 1], [0, 2]), dict(im=None)), (([0, 1], [0, 2]), dict(o=None)),
                     (([0, 1], [0, 2]), dict(n_imgs=-1))):
        assert call(*args, **kw) == -1, (args, kw)
        assert b"anerf_background_median" in lib.anerf_last_error()
    with pytest.raises(ValueError):
        anerf.median_backgrounds(np.zeros((2, 4, 3), np.uint8), [0, 3], n_cams=2, H=2, W=2)


# ---------------------------------------------------------------- the dataset end
def test_prepare_dataset_feeds_the_ray_dataset():
    raw, cam, H, W = cases.raw_dataset()
    n = len(raw["imgs"])
    data = anerf.prepare_dataset(raw, bkgd="masked_median", cam_idxs=cam)
    assert "sampling_masks" not in raw and set(raw) < set(data)
    want = dict(raw)
    want["sampling_masks"] = anerf.sampling_masks_reference(raw["masks"], 2, 5, False, H=H, W=W)
    want["bkgds"] = anerf.median_backgrounds_reference(raw["imgs"], cam, raw["masks"], H=H, W=W)
    want["bkgd_idxs"] = cam
    assert isinstance(data["sampling_masks"], np.ndarray) and data["sampling_masks"].shape == (n, H * W, 1)
    assert isinstance(data["bkgds"], np.ndarray) and data["bkgds"].shape == (2, H, W, 3)
    assert want["sampling_masks"].sum() > raw["masks"].sum()
    a = anerf.RayImageDataset(data, N_samples=40)
    b = anerf.RayImageDataset(want, N_samples=40)
    np.testing.assert_array_equal(a.sampling_masks, b.sampling_masks)
    assert torch.equal(a._bgs, b._bgs) and torch.equal(a._bg_idxs, b._bg_idxs)
    batches = []
    for ds in (a, b):
        np.random.seed(5)
        batches.append(ds.get_batch([0, 2, 3]))
    for k in ("rays_o", "rays_d", "target_s", "fgs", "bgs", "kp_idx"):
        assert torch.equal(batches[0][k], batches[1][k]), k
    # the other options: the band, keypoint masks first, the plain median
    data = anerf.prepare_dataset(raw, extend_iter=3, erode_border=True, kp_masks=True, bkgd="median", cam_idxs=cam)
    kp2d = anerf.skeleton3d_to_2d_reference(raw["kp3d"], raw["c2ws"], H, W, raw["focals"])
    ends = np.concatenate([kp2d, kp2d + (kp2d[:, kin.SMPLSkeleton.joint_trees] - kp2d)], -1)
    assert np.abs((ends - np.floor(ends)) - 0.5).min() > 1e-6  # (both sides round alike)
    kpm = anerf.create_kp_masks_reference(raw["masks"].reshape(n, H, W, 1), kp2ds=kp2d)
    np.testing.assert_array_equal(data["sampling_masks"].reshape(n, H, W),
                                  anerf.sampling_masks_reference(kpm.reshape(n, H, W), 3, 5, True))
    np.testing.assert_array_equal(data["bkgds"], anerf.median_backgrounds_reference(raw["imgs"], cam, H=H, W=W))
    assert "bkgds" not in anerf.prepare_dataset(raw)


# ---------------------------------------------------------------- the overlay
def test_render_sequence_skeleton_overlay(tmp_path):
    seq = importlib.import_module("a-nerf_amd.sequences")
    sc = syn.make_scene(n_joints=24, H=32, W=32, seed=3)
    cfg = anerf.RenderConfig(n_joints=24, netdepth=4, netwidth=128, N_samples=8, N_importance=8).validate()
    ck = syn.make_checkpoint(11, n_joints=24, D=4, W=128, fine=True, tau=20.0)
    kw = {"ray_caster": anerf.RayCaster(cfg, ck, device=0), "N_samples": 8, "N_importance": 8, "perturb": False,
          "raw_noise_std": 0., "ray_noise_std": 0., "use_viewdirs": True, "preproc_kwargs": {"density_scale": 1.0},
          "lindisp": False}
    s = seq.pose_sequence("bullet", sc["kps"], sc["bones"], sc["c2ws"], sc["focal"], sc["rest"], np.array([0]), n_bullet=2)
    out = str(tmp_path / "frames")
    plain = seq.render_sequence(s, 32, 32, 4096, kw, ext_scale=0.001, skeleton=False)
    assert len(plain) == 3
    rgbs, disps, accs, skels = seq.render_sequence(s, 32, 32, 4096, kw, ext_scale=0.001, skeleton=True, out_dir=out)
    assert torch.equal(rgbs, plain[0]) and torch.equal(disps, plain[1]) and accs == []
    assert skels.is_cuda and skels.dtype == torch.uint8 and tuple(skels.shape) == (2, 32, 32, 3)
    rk = s.render_kwargs(32, 32)
    want = anerf.draw_skeletons_3d(rgbs, s.kp, rk["render_poses"], *rk["hwf"])
    assert torch.equal(skels, want) and not torch.equal(skels, rgbs)
    assert sorted(os.listdir(out)) == ["00000.png", "00001.png", "skel"]
    assert sorted(os.listdir(os.path.join(out, "skel"))) == ["00000.png", "00001.png"]
    for i in range(2):
        np.testing.assert_array_equal(seq.read_png(os.path.join(out, "skel", f"{i:05d}.png")), _np(want)[i])
        np.testing.assert_array_equal(seq.read_png(os.path.join(out, f"{i:05d}.png")), _np(rgbs)[i])
    host = seq.render_sequence(s, 32, 32, 4096, kw, ext_scale=0.001, skeleton=True, to_host=True)
    assert isinstance(host[3], np.ndarray)
    np.testing.assert_array_equal(host[3], _np(want))

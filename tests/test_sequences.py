"""CPU: the pose and camera sequences of the render CLI (a-nerf_amd/sequences.py) without a GPU.

The NumPy float64 checker `pose_sequence_reference` -- which the GPU tests (tests/test_gpu_sequences.py) compare the
device path with -- is itself held to tests/golden/sequences.npz, the outputs of the reference's own run_render.py
loaders (tests/golden/make_sequence_golden.py): cameras, cam_idxs and focals must be EQUAL (the same float32
products), kps / skts / bones agree to 1e-12 (the float64 path, as tests/test_kinematics.py gives it).  poserot gets
the fixture's `poserot_d` on top: the reference builds its rotated roots with float32 matrices and float32 casts of
the pytorch3d stand-ins, the checker in float64, and the maker measured that difference with the reference's own
chain.  Everything else here is host logic: the wrappers' signatures, the refusals, the clip expansion, idx_map,
write_png, and the pose-checkpoint bridge's `legacy` swap.
"""
import importlib
import inspect
import os
import struct
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
cases = importlib.import_module("_sequence_cases")
seq = importlib.import_module("a-nerf_amd.sequences")
anerf = importlib.import_module("a-nerf_amd")
Z = np.load(os.path.join(HERE, "golden", "sequences.npz"), allow_pickle=False)


def test_fixture_inputs_are_the_seeded_case():
    c = cases.make_case()
    for k, v in c.items():
        np.testing.assert_array_equal(Z[k], v, err_msg=k)
    np.testing.assert_array_equal(Z["idx_map"], cases.IDX_MAP)
    b = c["bones"]
    assert not b[1, 5].any() and abs(np.linalg.norm(b[3, 7].astype(np.float64)) - 1e-8) < 1e-14
    assert abs(np.linalg.norm(b[4, 9].astype(np.float64)) - 3.0) < 1e-6
    assert 0 < float(Z["d"]) < 1e-6 and 0 < float(Z["poserot_d"]) < 1e-6 and 0 < float(Z["ckpt_d"]) < 1e-6


@pytest.mark.parametrize("name", list(cases.LOADER_ARGS))
def test_checker_against_the_reference_loaders(name):
    args, kw = cases.call_args(cases.make_case(), name)
    s = seq.pose_sequence_reference(*args, **kw)
    ref = {k: Z[f"{name}_{k}"] for k in ("kps", "skts", "c2ws", "cam_idxs", "focals")}
    for got, k in ((s.render_poses, "c2ws"), (s.cams, "cam_idxs"), (s.focals, "focals")):
        assert got.shape == ref[k].shape and got.dtype == ref[k].dtype, (k, got.dtype, ref[k].dtype)
        np.testing.assert_array_equal(got, ref[k], err_msg=k)
    tol = cases.F64_TOL + (float(Z["poserot_d"]) if name == "poserot" else 0.0)
    for got, k in ((s.kp, "kps"), (s.skts, "skts")):
        err = float(np.abs(got - ref[k]).max())
        print(f"{name} {k}: max |checker - reference| = {err:.3e} (bound {tol:.3e})")
        assert got.shape == ref[k].shape and err <= tol, (k, err)
    if f"{name}_bones" in Z.files:
        rb = Z[f"{name}_bones"]
        mine = s.bones if name == "poserot" else s.ref_bones
        assert mine.shape == rb.shape
        err = float(np.abs(mine - rb).max())
        print(f"{name} bones: {err:.3e}")
        assert err <= tol
    else:
        assert s.ref_bones is None


def test_wrappers_have_the_reference_signatures():
    want = {
        "load_correction": ["pose_h5", "c2ws", "focals", "rest_pose", "pose_keys", "selected_idxs", "n_step", "refined",
                            "center_kps", "idx_map", "init"],
        "load_retarget": ["pose_h5", "c2ws", "focals", "rest_pose", "pose_keys", "selected_idxs", "length", "skip",
                          "refined", "center_kps", "idx_map", "is_surreal", "undo_rot", "is_neuralbody"],
        "load_animate": ["pose_h5", "c2ws", "focals", "rest_pose", "pose_keys", "selected_idxs", "joints", "n_step",
                         "refined", "undo_rot", "center_cam", "center_kps", "idx_map"],
        "load_pose_rotate": ["pose_h5", "c2ws", "focals", "rest_pose", "pose_keys", "selected_idxs", "refined",
                             "n_bullet", "undo_rot", "center_cam", "center_kps", "idx_map"],
        "load_interpolate": ["pose_h5", "c2ws", "focals", "rest_pose", "pose_keys", "selected_idxs", "n_step", "refined",
                             "undo_rot", "center_cam", "center_kps", "idx_map"],
        "load_bullettime": ["pose_h5", "c2ws", "focals", "rest_pose", "pose_keys", "selected_idxs", "refined",
                            "n_bullet", "undo_rot", "center_cam", "center_kps", "idx_map"],
        "load_selected": ["pose_h5", "c2ws", "focals", "rest_pose", "pose_keys", "selected_idxs", "refined", "idx_map"],
        "load_bubble": ["pose_h5", "c2ws", "focals", "rest_pose", "pose_keys", "selected_idxs", "x_deg", "y_deg", "z_t",
                        "refined", "n_step", "center_kps", "idx_map"],
    }
    defaults = {"load_correction": {"n_step": 8}, "load_animate": {"n_step": 10}, "load_interpolate": {"n_step": 10},
                "load_bubble": {"n_step": 5, "x_deg": 15., "y_deg": 25., "z_t": 0.1, "center_kps": True},
                "load_bullettime": {"n_bullet": 30, "center_cam": True, "center_kps": True},
                "load_pose_rotate": {"n_bullet": 30, "center_cam": True, "center_kps": False},
                "load_retarget": {"skip": 1}}
    for name, params in want.items():
        fn = getattr(seq, name)
        assert getattr(anerf, name) is fn
        sig = inspect.signature(fn)
        assert list(sig.parameters) == params, name
        for k, v in defaults.get(name, {}).items():
            assert sig.parameters[k].default == v, (name, k)


class _Seq:
    """What pose_sequence returns, from the checker: stands in for the device path in the wrapper tests."""

    def __init__(self):
        self.calls = []

    def __call__(self, kind, *a, **kw):
        self.calls.append((kind, kw))
        return seq.pose_sequence_reference(kind, *a, **kw)


def test_wrappers_pass_arguments_on_and_return_in_the_reference_order(monkeypatch):
    c = cases.make_case()
    spy = _Seq()
    monkeypatch.setattr(seq, "pose_sequence", spy)
    refined = (c["kps"], c["bones"])
    base = ("x.h5", c["c2ws"], c["focals"], c["rest_pose"], ["/kp3d", "/bones"])

    def same(got, name, keys):
        assert len(got) == len(keys)
        for g, k in zip(got, keys):
            ref = Z[f"{name}_{k}"]
            assert np.shape(g) == ref.shape, (name, k)
            np.testing.assert_allclose(np.asarray(g, np.float64), ref, atol=2e-7, rtol=0, err_msg=f"{name} {k}")

    five = ("kps", "skts", "c2ws", "cam_idxs", "focals")
    same(seq.load_selected(*base, cases.SELECTED, refined), "selected", five)
    same(seq.load_retarget(*base, cases.SELECTED, 2, 1, refined, undo_rot=True), "retarget", five + ("bones",))
    same(seq.load_bullettime(*base, cases.SELECTED, refined, 4), "bullet", five + ("bones",))
    same(seq.load_bullettime(*base, cases.SELECTED, refined, 4, idx_map=cases.IDX_MAP), "bullet_map", five + ("bones",))
    same(seq.load_pose_rotate(*base, cases.SELECTED_POSEROT, refined, 6), "poserot",
         ("kps", "skts", "bones", "c2ws", "cam_idxs", "focals"))
    same(seq.load_interpolate(*base, cases.SELECTED, 3, refined), "interpolate", five)
    same(seq.load_animate(*base, cases.SELECTED, [16, 18, 20], 3, refined), "animate", five)
    same(seq.load_bubble(*base, cases.SELECTED, 15., 25., 0.1, refined, 4), "bubble", five)
    same(seq.load_correction(*base, cases.SELECTED, 3, refined, init=(c["kps"], c["init_bones"])), "correction", five)
    assert [k for k, _ in spy.calls] == ["selected", "retarget", "bullet", "bullet", "poserot", "interpolate", "animate",
                                         "bubble", "correction"]
    assert spy.calls[1][1]["undo_rot"] is True and spy.calls[1][1]["length"] == 2


def test_refusals():
    c = cases.make_case()
    a = (c["kps"], c["bones"], c["c2ws"], c["focals"], c["rest_pose"])
    with pytest.raises(NotImplementedError, match="render type orbit is not implemented!"):
        seq.pose_sequence_reference("orbit", *a, cases.SELECTED)
    with pytest.raises(NotImplementedError, match="render type orbit is not implemented!"):
        seq.pose_sequence("orbit", *a, cases.SELECTED)  # (refused before any device work)
    with pytest.raises(ValueError, match="poserot"):
        seq.pose_sequence_reference("poserot", *a, cases.SELECTED)
    with pytest.raises(ValueError, match="poserot"):
        seq.pose_sequence("poserot", *a, cases.SELECTED)
    with pytest.raises(ValueError, match="init_bones"):
        seq.pose_sequence_reference("correction", *a, cases.SELECTED)
    with pytest.raises(ValueError, match="joints"):
        seq.pose_sequence_reference("animate", *a, cases.SELECTED)
    with pytest.raises(ValueError, match="interp"):
        seq.pose_sequence_reference("interpolate", *a, cases.SELECTED, interp="cubic")
    with pytest.raises(TypeError, match="n_bulet"):
        seq.pose_sequence_reference("bullet", *a, cases.SELECTED, n_bulet=3)
    msg = "reading poses from the h5 through deepdish is not covered: pass refined=\\(kps, bones\\)"
    base = ("x.h5", c["c2ws"], c["focals"], c["rest_pose"], ["/kp3d", "/bones"], cases.SELECTED)
    for fn, extra in ((seq.load_selected, ()), (seq.load_retarget, (1,)), (seq.load_bullettime, ()),
                      (seq.load_pose_rotate, ()), (seq.load_interpolate, ()), (seq.load_animate, ([1],)),
                      (seq.load_bubble, ()), (seq.load_correction, ())):
        with pytest.raises(NotImplementedError, match=msg):
            fn(*base, *extra, refined=None)
    with pytest.raises(NotImplementedError, match="init="):
        seq.load_correction(*base, refined=(c["kps"], c["bones"]))


def test_capi_refuses_bad_tables_before_any_launch():
    """anerf_sequence_bones / anerf_rotation_to_axis_angle validate on the host (include/anerf.h): a key outside
    [0, K), F < 1, an unknown mode return ANERF_EINVAL with a message, and no HIP call is made (none could be here)."""
    import ctypes
    _lib = importlib.import_module("a-nerf_amd._lib")
    lib = _lib.load()
    keys = np.array([[0, 1, 0, 0, 0], [1, 2, 0, 0, 0]], np.int32)
    vals = np.zeros((2, 2), np.float64)
    one = ctypes.c_void_p(8)  # (a non-NULL stand-in: validation returns before any pointer is read on the device)

    def call(k=keys, v=vals, n_keys=3, nj=24, root=0, n=2, interp=0, mode=0, const=None):
        return lib.anerf_sequence_bones(one, one, n_keys, nj, root, k.ctypes.data_as(_lib.c_i32p),
                                        v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), one, one, None, n, interp,
                                        mode, const, one, one, None)

    assert call(n_keys=2) == -1 and b"outside [0, n_keys = 2)" in lib.anerf_last_error()
    bad = keys.copy()
    bad[1, 3] = -1
    assert call(k=bad) == -1 and b"frame 1" in lib.anerf_last_error()
    assert call(n=0) == -1 and b"n_frames" in lib.anerf_last_error()
    assert call(nj=129) == -1 and b"n_joints" in lib.anerf_last_error()
    assert call(root=24) == -1 and b"root_id" in lib.anerf_last_error()
    assert call(interp=2) == -1 and b"interp" in lib.anerf_last_error()
    assert call(mode=3) == -1 and b"root_mode" in lib.anerf_last_error()
    assert call(mode=1) == -1 and b"root_const" in lib.anerf_last_error()
    ax = keys.copy()
    ax[0, 4] = 3
    assert call(k=ax, mode=2) == -1 and b"axis id" in lib.anerf_last_error()
    nf = vals.copy()
    nf[1, 0] = np.nan
    assert call(v=nf) == -1 and b"finite" in lib.anerf_last_error()
    assert lib.anerf_rotation_to_axis_angle(one, 3, 1, one, None) == -1 and b"rot_dim" in lib.anerf_last_error()
    assert lib.anerf_rotation_to_axis_angle(None, 9, 1, one, None) == -1 and b"NULL" in lib.anerf_last_error()
    assert lib.anerf_rotation_to_axis_angle(None, 9, 0, None, None) == 0


def test_length_skip_expansion():
    # the reference expands only when skip > 1 and length > 1, and clips at the dataset's end
    np.testing.assert_array_equal(seq.expand_selected(np.array([1, 3]), 4, 2, 5), [1, 3, 3])
    np.testing.assert_array_equal(seq.expand_selected(np.array([0, 2]), 3, 2, 5), [0, 2, 2, 4])
    np.testing.assert_array_equal(seq.expand_selected(np.array([1, 3]), 4, 1, 5), [1, 3])
    np.testing.assert_array_equal(seq.expand_selected(np.array([1, 3]), 1, 2, 5), [1, 3])
    c = cases.make_case()
    a = (c["kps"], c["bones"], c["c2ws"], c["focals"], c["rest_pose"])
    s = seq.pose_sequence_reference("retarget", *a, np.array([0, 2]), length=3, skip=2)
    rows = np.array([0, 2, 2, 4])
    np.testing.assert_array_equal(s.cams, rows)
    np.testing.assert_array_equal(s.render_poses, c["c2ws"][rows])
    np.testing.assert_array_equal(s.focals, c["focals"][rows])
    one = seq.pose_sequence_reference("selected", *a, rows)
    np.testing.assert_array_equal(s.kp, one.kp)
    np.testing.assert_array_equal(s.skts, one.skts)


def test_idx_map_lookup():
    np.testing.assert_array_equal(seq.find_idxs_with_map(cases.SELECTED, cases.IDX_MAP), [3, 1, 0])
    np.testing.assert_array_equal(seq.find_idxs_with_map(np.array([9, 7, 4]), cases.IDX_MAP), [4, 0])  # 7: dropped
    assert seq.find_idxs_with_map(cases.SELECTED, None) is cases.SELECTED
    c = cases.make_case()
    a = (c["kps"], c["bones"], c["c2ws"], c["focals"], c["rest_pose"])
    s = seq.pose_sequence_reference("selected", *a, cases.SELECTED, idx_map=cases.IDX_MAP)
    t = seq.pose_sequence_reference("selected", *a, np.array([3, 1, 0]))
    np.testing.assert_array_equal(s.kp, t.kp)  # the poses of the mapped rows ...
    np.testing.assert_array_equal(s.cams, [3, 1, 0])
    np.testing.assert_array_equal(s.render_poses, c["c2ws"][cases.SELECTED])  # ... under the selected cameras
    s = seq.pose_sequence_reference("selected", *a, cases.SELECTED, selected_framecode=2)
    np.testing.assert_array_equal(s.cams, [2, 2, 2])


def test_render_kwargs_and_render_res():
    args, kw = cases.call_args(cases.make_case(), "bullet")
    s = seq.pose_sequence_reference(*args, **kw)
    r = s.render_kwargs(100, 80)
    assert set(r) == {"kp", "skts", "render_poses", "cams", "hwf", "bones", "bg_imgs", "bg_indices", "subject_idxs"}
    assert r["hwf"][:2] == (100, 80) and r["bg_imgs"] is None and r["subject_idxs"] is None
    np.testing.assert_array_equal(r["hwf"][2], s.focals)
    r = s.render_kwargs(100, 80, render_res=(50, 64))
    assert r["hwf"][:2] == (50, 64)
    np.testing.assert_array_equal(r["hwf"][2], s.focals * (50.0 / 100.0))
    np.testing.assert_array_equal(s.focals, Z["bullet_focals"])  # (the sequence's own focals are not scaled in place)
    assert len(s) == 12


def test_matrix_to_axis_angle_reference_round_trip_and_formula():
    """scipy's from_matrix().as_rotvec() inverts from_rotvec().as_matrix(); the kernel's formula, restated in float64
    (matrix_to_axis_angle_formula), agrees with scipy; its agreement on the GPU test's own float32 matrices
    (tests/_sequence_cases.formula_agreement, printed here) is the first term of the GPU bound."""
    from scipy.spatial.transform import Rotation
    rs = np.random.RandomState(3)
    v = rs.normal(size=(500, 3))
    v *= (rs.uniform(0, np.pi - 1e-3, size=(500, 1)) / np.linalg.norm(v, axis=-1, keepdims=True))
    R = Rotation.from_rotvec(v).as_matrix()
    np.testing.assert_allclose(seq.matrix_to_axis_angle_reference(R), v, atol=1e-12, rtol=0)
    np.testing.assert_allclose(seq.matrix_to_axis_angle_reference(R[..., :3, :2].reshape(500, 6)), v, atol=1e-12, rtol=0)
    np.testing.assert_allclose(seq.matrix_to_axis_angle_reference(R.reshape(5, 100, 3, 3)), v.reshape(5, 100, 3),
                               atol=1e-12, rtol=0)
    # exactly orthogonal input: the same rotation vector to rounding (8.9e-16 on the issue's probe)
    exact = float(np.abs(seq.matrix_to_axis_angle_formula(R) - v).max())
    print(f"formula vs scipy, float64, exact matrices: {exact:.3e}")
    assert exact <= 1e-14
    # float32 roundings of rotations (the GPU test's input): scipy projects onto the nearest rotation first, the
    # formula reads the quaternion off the matrix as it is.  Both estimate a rotation from entries off by up to 2^-24,
    # a perturbation of Frobenius norm <= 3 * 2^-24 = 1.8e-7 that moves either estimate by about that angle at most
    m, ang = cases.rotations()
    far = ang <= np.pi - 1e-3
    f = seq.matrix_to_axis_angle_formula(m)
    s = seq.matrix_to_axis_angle_reference(m)
    assert np.isfinite(f).all()
    err = cases.formula_agreement()
    print(f"formula vs scipy, float64, float32 matrices, angle <= pi - 1e-3: {err:.3e}")
    assert err == float(np.abs(f - s)[far].max()) and err <= 2 * 3 * 2.0 ** -24
    # next to pi the axis' sign is free: compare the rotations
    back = Rotation.from_rotvec(f[~far]).as_matrix()
    assert float(np.abs(back - Rotation.from_rotvec(s[~far]).as_matrix()).max()) <= 2 * 3 * 2.0 ** -24
    assert np.all(np.linalg.norm(f, axis=-1) <= np.pi + 1e-12)


def _png_chunks(blob):
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(blob):
        n, = struct.unpack(">I", blob[at:at + 4])
        tag, data = blob[at + 4:at + 8], blob[at + 8:at + 8 + n]
        assert struct.unpack(">I", blob[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff
        out.append((tag, data))
        at += 12 + n
    return out


@pytest.mark.parametrize("shape", [(7, 5, 3), (7, 5), (4, 9, 1), (1, 1, 3)])
def test_write_png_round_trip(tmp_path, shape):
    rs = np.random.RandomState(sum(shape))
    img = rs.randint(0, 256, size=shape).astype(np.uint8)
    p = str(tmp_path / "a.png")
    seq.write_png(p, img)
    chunks = _png_chunks(open(p, "rb").read())
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    h, w = shape[:2]
    ch = 3 if len(shape) == 3 and shape[2] == 3 else 1
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (w, h, 8, 2 if ch == 3 else 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert not raw[:, 0].any()  # filter type 0 on every row
    np.testing.assert_array_equal(raw[:, 1:].reshape(h, w, ch), img.reshape(h, w, ch))
    np.testing.assert_array_equal(seq.read_png(p), img.reshape(h, w, ch) if ch == 3 else img.reshape(h, w))
    with pytest.raises(ValueError, match="uint8"):
        seq.write_png(p, img.astype(np.float32))
    with pytest.raises(ValueError, match="takes"):
        seq.write_png(p, np.zeros((2, 2, 4), np.uint8))


def test_to8b_is_the_reference_rule():
    x = np.array([-0.5, 0.0, 0.4999, 0.5, 0.999, 1.0, 1.7], np.float32)
    np.testing.assert_array_equal(seq.to8b(x), [0, 0, 127, 127, 254, 255, 255])
    import torch
    np.testing.assert_array_equal(seq.to8b(torch.from_numpy(x)).numpy(), seq.to8b(x))


@pytest.mark.parametrize("legacy", [True, False])
def test_pose_data_checker_legacy_against_the_reference(legacy):
    """pose_data_reference (the checker of pose_ckpt_to_pose_data) against the reference's own legacy outputs; without
    legacy against the plain chain.  The bound is 1e-12 plus the fixture's ckpt_d, what the reference's float32 root
    re-rotation and float32 rest offsets cost against float64, measured by the maker with the reference's chain."""
    c = cases.make_case()
    pelvis, bones, rest = c["kps"][:, 0], c["bones"], c["rest_pose"]
    kp3d, b, skts, cyls, rp, pel = seq.pose_data_reference(pelvis, bones, rest, ext_scale=0.001, legacy=legacy)
    if not legacy:
        kp, sk, _ = seq.kinematic_chain_reference(bones, rest, pelvis=pelvis)
        np.testing.assert_array_equal(kp3d, kp)
        np.testing.assert_array_equal(skts, sk)
        np.testing.assert_array_equal(b, bones)
        return
    tol = cases.F64_TOL + float(Z["ckpt_d"])
    for got, k in ((kp3d, "kp3d"), (b, "bones"), (skts, "skts")):
        err = float(np.abs(got - Z[f"ckpt_{k}"]).max())
        print(f"legacy {k}: {err:.3e} (bound {tol:.3e})")
        assert err <= tol, k
    np.testing.assert_array_equal(rp.astype(np.float32), Z["ckpt_rest_pose"])
    np.testing.assert_array_equal(pel.astype(np.float32), Z["ckpt_pelvis"])
    # the cylinder is float32 arithmetic on kp3d: one float32 ulp of its inputs' difference
    np.testing.assert_allclose(cyls, Z["ckpt_cyls"], atol=4 * tol, rtol=0)
    # 6-D parameters give the same pose data as the axis-angle they encode
    from scipy.spatial.transform import Rotation
    R = Rotation.from_rotvec(bones.reshape(-1, 3).astype(np.float64)).as_matrix().reshape(bones.shape[:2] + (3, 3))
    out6 = seq.pose_data_reference(pelvis, R[..., :3, :2].reshape(bones.shape[:2] + (6,)), rest, legacy=True)
    np.testing.assert_allclose(out6[0], kp3d, atol=1e-12, rtol=0)
    np.testing.assert_allclose(out6[2], skts, atol=1e-11, rtol=0)

"""GPU: the pose sequences of the render CLI on the device (anerf_sequence_bones + anerf_pose_kinematics), the inverse
rotation map (anerf_rotation_to_axis_angle), the pose-checkpoint bridge and render_sequence.

Bounds (tests/_sequence_cases.py holds the constants):
* cameras, cam_idxs and focals are host work with the reference's own products: EQUAL to the fixture.
* selected, retarget, bullet and bubble feed the chain the float32 key bones themselves: kps and l2ws are held to
  tests/test_kinematics.py's GPU bounds for get_smpl_l2ws (atol 2.5e-7, rtol 1.2e-7; skts atol 5e-7, rtol 2.4e-7).
* the interpolated kinds (interpolate, animate, correction, poserot) emit float32 bones where the reference chains
  float64 ones.  The fixture's `d` is that effect measured on the CPU with the reference's own chain (1.6e-7); these
  kinds get the bounds above plus 2 d, the factor covering frames the maker's set does not reach.  poserot is compared
  with a fixture that itself carries float32 steps (float32 rotate matrices, float32 casts), measured by the maker as
  `poserot_d`: that is added for poserot alone.
* matrix_to_axis_angle and slerp: the float64 agreement of the kernel's formula with scipy
  (_sequence_cases.formula_agreement, recorded by tests/test_sequences.py) plus 2.4e-7, one float32 ulp in [2, 4), for
  the rounding of the output.
"""
import importlib
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
cases = importlib.import_module("_sequence_cases")
syn = importlib.import_module("a-nerf_amd.synthetic")
Z = np.load(os.path.join(HERE, "golden", "sequences.npz"), allow_pickle=False)
TOL_GPU = 4e-6  # tests/test_kinematics.py: float32 rounding of the chain (rots, PoseOptLayer paths)

pytestmark = pytest.mark.gpu


def _mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("a-nerf_amd.sequences"), importlib.import_module("a-nerf_amd.kinematics")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _close(got, ref, atol, rtol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    print(f"{what}: max |gpu - ref| = {float(err.max()):.3e} (atol {atol:.3e}, rtol {rtol:.1e})")
    assert np.isfinite(got).all(), what
    assert (err <= atol + rtol * np.abs(ref)).all(), (what, float(err.max()))


def _extra(name):
    if name in cases.DIRECT_KINDS:
        return 0.0
    return 2.0 * float(Z["d"]) + (float(Z["poserot_d"]) if name == "poserot" else 0.0)


@pytest.mark.parametrize("name", list(cases.LOADER_ARGS))
def test_gpu_every_kind_against_the_fixture(name):
    seq, _ = _mods()
    c = cases.make_case()
    args, kw = cases.call_args(c, name)
    s = seq.pose_sequence(*args, **kw)
    for got, k in ((s.render_poses, "c2ws"), (s.cams, "cam_idxs"), (s.focals, "focals")):
        ref = Z[f"{name}_{k}"]
        assert got.shape == ref.shape and got.dtype == ref.dtype, k
        np.testing.assert_array_equal(got, ref, err_msg=k)
    for t in (s.kp, s.skts, s.bones, s.l2ws):
        assert t.is_cuda and t.dtype == torch.float32
    x = _extra(name)
    chk = seq.pose_sequence_reference(*args, **kw)  # (held to the fixture at 1e-12 by tests/test_sequences.py)
    _close(_np(s.kp), Z[f"{name}_kps"], cases.L2W_ATOL + x, cases.L2W_RTOL, f"{name} kps")
    _close(_np(s.skts), Z[f"{name}_skts"], cases.SKT_ATOL + x, cases.SKT_RTOL, f"{name} skts")
    _close(_np(s.l2ws), chk.l2ws, cases.L2W_ATOL + x, cases.L2W_RTOL, f"{name} l2ws")  # (the loaders return no l2ws)
    if name in cases.DIRECT_KINDS:
        # the frames' bones are the key rows, bit for bit
        np.testing.assert_array_equal(_np(s.bones), chk.bones)
        if f"{name}_bones" in Z.files:
            np.testing.assert_array_equal(s.ref_bones, Z[f"{name}_bones"])
    else:
        # float32 roundings of the float64 formula (|component| < 4)
        _close(_np(s.bones), chk.bones, cases.ULP_2_4, 0.0, f"{name} bones")
        if name == "poserot":
            _close(_np(s.bones), Z["poserot_bones"], cases.ULP_2_4 + float(Z["poserot_d"]), 0.0, "poserot bones")


def _random_keys(rs, n, nj):
    kps = rs.normal(scale=0.5, size=(n, nj, 3)).astype(np.float32)
    bones = (0.4 * rs.normal(size=(n, nj, 3))).astype(np.float32)
    c2ws = np.stack([syn.camera_c2w(distance=5.0, yaw=0.2 * i) for i in range(n)])
    return kps, bones, c2ws, np.linspace(300, 350, n).astype(np.float32)


def test_gpu_interpolate_65_joints():
    """The second half-wave of the chain (joints 64 ...), which the 24-joint loaders of the reference never reach."""
    seq, _ = _mods()
    skel, rest = cases.skeleton65()
    kps, bones, c2ws, focals = _random_keys(np.random.RandomState(65), 3, 65)
    a = ("interpolate", kps, bones, c2ws, focals, rest.astype(np.float64), np.array([2, 0, 1]))
    s = seq.pose_sequence(*a, n_step=4, skel_type=skel)
    chk = seq.pose_sequence_reference(*a, n_step=4, skel_type=skel)
    assert len(s) == 9 and s.kp.shape == (9, 65, 3)
    x = 2.0 * float(Z["d"])
    _close(_np(s.bones), chk.bones, cases.ULP_2_4, 0.0, "bones")
    _close(_np(s.kp), chk.kp, cases.L2W_ATOL + x, cases.L2W_RTOL, "kps")
    _close(_np(s.l2ws), chk.l2ws, cases.L2W_ATOL + x, cases.L2W_RTOL, "l2ws")
    _close(_np(s.skts), chk.skts, cases.SKT_ATOL + x, cases.SKT_RTOL, "skts")


@pytest.mark.parametrize("n_keys,n_step,frames", [(3, 3, 7), (2, 11, 12)])
def test_gpu_frame_counts(n_keys, n_step, frames):
    """F = 7 and F = 12: counts that are not, and are, a multiple of the kinematics kernel's four waves per block."""
    seq, _ = _mods()
    c = cases.make_case()
    a = ("interpolate", c["kps"], c["bones"], c["c2ws"], c["focals"], c["rest_pose"], np.arange(n_keys) + 1)
    s = seq.pose_sequence(*a, n_step=n_step)
    chk = seq.pose_sequence_reference(*a, n_step=n_step)
    assert len(s) == frames and tuple(s.skts.shape) == (frames, 24, 4, 4) and tuple(s.bones.shape) == (frames, 24, 3)
    x = 2.0 * float(Z["d"])
    _close(_np(s.kp), chk.kp, cases.L2W_ATOL + x, cases.L2W_RTOL, "kps")
    _close(_np(s.skts), chk.skts, cases.SKT_ATOL + x, cases.SKT_RTOL, "skts")
    np.testing.assert_array_equal(_np(s.bones)[-1], c["bones"][n_keys])  # the last frame is the last key


def test_gpu_animate_joint_masks():
    seq, _ = _mods()
    c = cases.make_case()
    a = (c["kps"], c["bones"], c["c2ws"], c["focals"], c["rest_pose"], cases.SELECTED)
    none = seq.pose_sequence("animate", *a, joints=[], n_step=3)
    first = c["bones"][cases.SELECTED[0]]
    assert len(none) == 7
    np.testing.assert_array_equal(_np(none.bones), np.broadcast_to(first, (7, 24, 3)))
    for t in (none.kp, none.skts):
        assert bool((t == t[:1]).all())
    every = seq.pose_sequence("animate", *a, joints=list(range(24)), n_step=3)
    inter = seq.pose_sequence("interpolate", *a, n_step=3)
    for x, y in ((every.bones, inter.bones), (every.kp, inter.kp), (every.skts, inter.skts), (every.l2ws, inter.l2ws)):
        assert torch.equal(x, y)
    np.testing.assert_array_equal(every.render_poses, inter.render_poses)


def test_gpu_root_modes_and_the_device_table_guard():
    """ANERF_SEQ_ROOT_CONST reads every key's root as the constant (the same bits as undo_rot applied to the key rows
    on the host); a key outside [0, K) in the DEVICE copy of the table, which the host check cannot see, gives that
    frame NaN and is not read through."""
    seq, _ = _mods()
    _lib = importlib.import_module("a-nerf_amd._lib")
    c = cases.make_case()
    a = (c["kps"], c["bones"], c["c2ws"], c["focals"], c["rest_pose"], cases.SELECTED)
    o = seq._options(dict(n_step=3))
    plan = seq._plan_of("interpolate", *a[:4], a[5], o)
    for interp in ("linear", "slerp"):
        const, pel = seq.sequence_bones(plan.key_bones, plan.key_root, plan.keys, plan.vals, interp=interp,
                                        root_mode=_lib.ANERF_SEQ_ROOT_CONST, root_const=seq.UNDO_ROT)
        host = seq.pose_sequence("interpolate", *a, n_step=3, undo_rot=True, interp=interp)
        assert torch.equal(const, host.bones)
        np.testing.assert_array_equal(_np(pel), np.broadcast_to(plan.key_root[0], (7, 3)))
        if interp == "linear":
            np.testing.assert_array_equal(_np(const)[:, 0], np.broadcast_to(seq.UNDO_ROT, (7, 3)))
    with pytest.raises(_lib.AnerfError, match="outside"):
        bad = plan.keys.copy()
        bad[2, 1] = 3
        seq.sequence_bones(plan.key_bones, plan.key_root, bad, plan.vals)
    # the device copy alone carries the bad key (one past the last): call the entry point with two different tables
    lib, dev = _lib.load(), torch.device("cuda", 0)
    kb, kr = torch.from_numpy(plan.key_bones).to(dev), torch.from_numpy(plan.key_root).to(dev)
    bad_d, vals_d = torch.from_numpy(bad).to(dev), torch.from_numpy(plan.vals).to(dev)
    out, pel = torch.zeros(7, 24, 3, device=dev), torch.zeros(7, 3, device=dev)
    ct = _lib.ctypes
    rc = lib.anerf_sequence_bones(_lib.ptr(kb), _lib.ptr(kr), 3, 24, 0, plan.keys.ctypes.data_as(_lib.c_i32p),
                                  plan.vals.ctypes.data_as(ct.POINTER(ct.c_double)), _lib.ptr(bad_d), _lib.ptr(vals_d),
                                  None, 7, 0, 0, None, _lib.ptr(out), _lib.ptr(pel), _lib.stream_handle(dev))
    assert rc == 0
    good = seq.sequence_bones(plan.key_bones, plan.key_root, plan.keys, plan.vals)[0]
    assert bool(torch.isnan(out[2]).all()) and bool(torch.isnan(pel[2]).all())
    keep = [0, 1, 3, 4, 5, 6]
    assert torch.equal(out[keep], good[keep])


def test_gpu_matrix_to_axis_angle():
    seq, kin = _mods()
    from scipy.spatial.transform import Rotation
    m, ang = cases.rotations()
    m = np.array(m)  # (a writable copy for torch)
    far = ang <= np.pi - 1e-3
    tol = cases.formula_agreement() + cases.ULP_2_4
    ref = seq.matrix_to_axis_angle_reference(m)  # scipy on the same float32 matrices
    got = _np(seq.matrix_to_axis_angle(m))
    assert got.shape == (len(m), 3) and np.isfinite(got).all()
    _close(got[far], ref[far], tol, 0.0, "matrices, angle <= pi - 1e-3")
    assert np.all(np.linalg.norm(got, axis=-1) <= np.pi + cases.ULP_2_4)  # the angle lies in [0, pi]
    # the identity and the angles of 1e-8
    tiny = np.where(ang < 1e-6)[0]
    assert len(tiny) == 3 and not got[tiny[0]].any()
    np.testing.assert_allclose(got[tiny[1:]], ref[tiny[1:]], atol=1e-14, rtol=0)
    np.testing.assert_allclose(np.linalg.norm(got[tiny[1:]], axis=-1), 1e-8, rtol=1e-6)
    # within 1e-3 of pi the sign of the axis is free: compare the matrices the chain rebuilds.  Their bound: the two
    # estimates of a rotation from float32 entries (2 * 3 * 2^-24, as tests/test_sequences.py), the output's rounding
    # (|dv| <= sqrt(3) * 1.2e-7 moves no entry further) and the float32 rounding of the rebuilt entries (2^-24)
    near = ~far
    one_joint = kin.Skeleton(["root"], np.zeros(1, np.int64), 0, [], {}, [])
    rots = kin.pose_kinematics(torch.from_numpy(got[near].astype(np.float32))[:, None], np.zeros((1, 3)), one_joint,
                               outputs=("rots",))["rots"][:, 0]
    _close(_np(rots), Rotation.from_rotvec(ref[near]).as_matrix(), 6 * 2.0 ** -24 + np.sqrt(3) * 1.2e-7 + 2.0 ** -24,
           0.0, "matrices rebuilt next to pi")
    # 6-D input, in another leading shape
    far_i = np.where(far)[0][:1998]
    m6 = np.ascontiguousarray(m[far_i][:, :, :2].reshape(-1, 6)).reshape(2, 999, 6)
    ref6 = seq.matrix_to_axis_angle_reference(m6)
    got6 = seq.matrix_to_axis_angle(torch.from_numpy(m6).cuda())
    assert tuple(got6.shape) == (2, 999, 3) and got6.is_cuda
    _close(_np(got6), ref6, tol, 0.0, "6-D parameters")


def test_gpu_get_bones_of_a_rot6d_layer():
    seq, kin = _mods()
    c = cases.make_case()
    L = kin.PoseOptLayer(c["kps"], c["bones"], c["rest_pose"][None], use_rot6d=True)
    assert L.bones.shape[-1] == 6
    aa = L.get_bones()
    assert tuple(aa.shape) == (5, 24, 3) and aa.is_cuda and torch.isfinite(aa).all()
    rots = kin.pose_kinematics(aa, c["rest_pose"], outputs=("rots",))["rots"]
    want = seq.rot6d_to_rotmat_reference(_np(L.bones))
    _close(_np(rots), want, TOL_GPU, 0.0, "kin_rotation(get_bones) vs rot6d_to_rotmat(parameters)")
    sub = L.get_bones(np.array([4, 1]))
    assert torch.equal(sub, aa[[4, 1]])
    # an axis-angle layer returns its parameters, as before
    L3 = kin.PoseOptLayer(c["kps"], c["bones"], c["rest_pose"][None])
    np.testing.assert_array_equal(_np(L3.get_bones()), c["bones"])


def test_gpu_slerp_against_scipy():
    seq, _ = _mods()
    from scipy.spatial.transform import Rotation, Slerp
    rs = np.random.RandomState(12)
    kps, bones, c2ws, focals = _random_keys(rs, 2, 24)
    u = np.array([0.6, -0.48, 0.64])
    bones[0, 5], bones[1, 5] = 2.8 * u, -2.8 * u  # quaternions with a negative dot product: the arc through pi
    bones[1, 7] = bones[0, 7]  # equal keys
    bones[0, 9] = bones[1, 9] = 0.0
    q = [Rotation.from_rotvec(bones[k, 5].astype(np.float64)).as_quat() for k in (0, 1)]
    assert float(np.dot(q[0], q[1])) < -0.5
    rest = cases.make_case()["rest_pose"]
    a = ("interpolate", kps, bones, c2ws, focals, rest, np.array([0, 1]))
    n_step = 3
    s = seq.pose_sequence(*a, n_step=n_step, interp="slerp")
    got = _np(s.bones)
    assert got.shape == (n_step + 1, 24, 3) and np.isfinite(got).all()
    assert all(bool(torch.isfinite(t).all()) for t in (s.kp, s.skts, s.l2ws))
    w = np.concatenate([np.linspace(0, 1.0, n_step, endpoint=False), [1.0]])
    want = np.stack([Slerp([0.0, 1.0], Rotation.from_rotvec(bones[:, j].astype(np.float64)))(w).as_rotvec()
                     for j in range(24)], 1)
    tol = cases.formula_agreement() + cases.ULP_2_4
    _close(got, want, tol, 0.0, "slerp bones vs scipy Slerp")
    # the lerp of the reference leaves the geodesic on that pair: at w = 1/3 it is a rotation by 2.8 / 3 about u, far
    # from the short arc, which stays within 0.35 rad of pi
    lin = _np(seq.pose_sequence(*a, n_step=n_step).bones)
    assert abs(np.linalg.norm(lin[1, 5]) - 2.8 / 3) < 1e-6 and np.linalg.norm(got[1, 5]) > np.pi - 0.35
    # the checker takes the same path
    chk = seq.pose_sequence_reference(*a, n_step=n_step, interp="slerp")
    _close(got, chk.bones, tol, 0.0, "slerp bones vs the checker")
    x = 2.0 * float(Z["d"])
    _close(_np(s.skts), chk.skts, cases.SKT_ATOL + x, cases.SKT_RTOL, "slerp skts")


def test_gpu_two_calls_give_the_same_bits():
    seq, _ = _mods()
    c = cases.make_case()
    for name, interp in (("interpolate", "linear"), ("interpolate", "slerp"), ("poserot", "linear")):
        args, kw = cases.call_args(c, name)
        a, b = (seq.pose_sequence(*args, interp=interp, **kw) for _ in range(2))
        for x, y in ((a.bones, b.bones), (a.kp, b.kp), (a.skts, b.skts), (a.l2ws, b.l2ws)):
            assert torch.equal(x, y), (name, interp)
    m = np.array(cases.rotations()[0])
    assert torch.equal(seq.matrix_to_axis_angle(m), seq.matrix_to_axis_angle(m))


def test_gpu_pose_ckpt_to_pose_data(tmp_path):
    """A save_popt-shaped checkpoint of a 6-D layer -> pose data, with and without `legacy`, against the float64
    checker on the layer's own parameters (TOL_GPU: float32 rounding of the chain, as tests/test_kinematics.py)."""
    seq, kin = _mods()
    c = cases.make_case()
    L = kin.PoseOptLayer(c["kps"], c["bones"], c["rest_pose"][None], use_rot6d=True)
    sd = {k: v.detach().cpu() for k, v in L.state_dict().items()}
    path = str(tmp_path / "popt.tar")
    torch.save({"global_step": 7, "poseopt_layer_state_dict": sd, "poseopt_anchors": None}, path)
    for legacy in (False, True):
        kp3d, bones, skts, cyls, rest, pelvis = seq.pose_ckpt_to_pose_data(path, legacy=legacy)
        for v in (kp3d, bones, skts, cyls, rest, pelvis):
            assert isinstance(v, np.ndarray) and v.dtype == np.float32
        want = seq.pose_data_reference(_np(L.pelvis), _np(L.bones), c["rest_pose"], legacy=legacy)
        for got, ref, k in zip((kp3d, skts, cyls, rest, pelvis), (want[0], want[2], want[3], want[4], want[5]),
                               ("kp3d", "skts", "cyls", "rest_pose", "pelvis")):
            _close(got, ref, TOL_GPU, 0.0, f"legacy={legacy} {k}")
        R = kin.pose_kinematics(bones, rest, outputs=("rots",))["rots"]
        from scipy.spatial.transform import Rotation
        _close(_np(R), Rotation.from_rotvec(want[1].reshape(-1, 3)).as_matrix().reshape(5, 24, 3, 3), TOL_GPU, 0.0,
               f"legacy={legacy} rotations of the bones")
    same = seq.pose_ckpt_to_pose_data(popt_sd=sd, legacy=True)
    np.testing.assert_array_equal(same[0], kp3d)


def test_gpu_render_sequence_end_to_end(tmp_path):
    seq, _ = _mods()
    anerf = importlib.import_module("a-nerf_amd")
    sc = syn.make_scene(n_joints=24, H=32, W=32, seed=3)
    cfg = anerf.RenderConfig(n_joints=24, netdepth=4, netwidth=128, N_samples=8, N_importance=8).validate()
    ck = syn.make_checkpoint(11, n_joints=24, D=4, W=128, fine=True, tau=20.0)
    kw = {"ray_caster": anerf.RayCaster(cfg, ck, device=0), "N_samples": 8, "N_importance": 8, "perturb": False,
          "raw_noise_std": 0., "ray_noise_std": 0., "use_viewdirs": True, "preproc_kwargs": {"density_scale": 1.0},
          "lindisp": False}
    s = seq.pose_sequence("bullet", sc["kps"], sc["bones"], sc["c2ws"], sc["focal"], sc["rest"], np.array([0]),
                          n_bullet=3)
    assert len(s) == 3
    out = str(tmp_path / "frames")
    rgbs, disps, accs = seq.render_sequence(s, 32, 32, 4096, kw, ret_acc=True, ext_scale=0.001, to_uint8=False)
    rk = s.render_kwargs(32, 32)
    frames, _, _ = anerf.render_frames(rk["render_poses"], rk["hwf"], 4096, kw, kp=rk["kp"], skts=rk["skts"],
                                       bones=rk["bones"], cams=rk["cams"], ret_acc=True, ext_scale=0.001,
                                       to_host=False)
    assert tuple(rgbs.shape) == (3, 32, 32, 3) and rgbs.is_cuda and rgbs.dtype == torch.float32
    assert tuple(disps.shape) == (3, 32, 32, 1) and tuple(accs.shape) == (3, 32, 32, 1)
    for i, f in enumerate(frames):
        assert torch.equal(rgbs[i], f[0]) and torch.equal(disps[i], f[1]) and torch.equal(accs[i], f[2])
    assert float(accs.max()) > 0.0 and not torch.equal(rgbs[0], rgbs[1])  # something is rendered, and the orbit moves
    u8, _, none = seq.render_sequence(s, 32, 32, 4096, kw, ext_scale=0.001, out_dir=out)
    assert u8.dtype == torch.uint8 and u8.is_cuda and none == []
    want = (255 * np.clip(rgbs.cpu().numpy(), 0, 1)).astype(np.uint8)
    np.testing.assert_array_equal(u8.cpu().numpy(), want)
    assert sorted(os.listdir(out)) == ["00000.png", "00001.png", "00002.png"]
    for i in range(3):
        np.testing.assert_array_equal(seq.read_png(os.path.join(out, f"{i:05d}.png")), want[i])
    host = seq.render_sequence(s, 32, 32, 4096, kw, ext_scale=0.001, to_host=True)[0]
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8
    np.testing.assert_array_equal(host, want)

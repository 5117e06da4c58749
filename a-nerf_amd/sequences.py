"""The pose and camera sequences of the reference's render CLI, built on the device (run_render.py:473-865), and the
bridge from a pose checkpoint to them (core/pose_opt.py:523-559).

`pose_sequence(kind, ...)` covers the eight render types -- selected, retarget, bullet, poserot, interpolate, animate,
bubble, correction -- and returns a `RenderSequence` whose kp / skts / bones are float32 DEVICE tensors: the K key
poses go up once with two small per-frame tables, `anerf_sequence_bones` writes every frame's bones and pelvis in one
launch, and the existing `anerf_pose_kinematics` chains them.  `render_sequence` hands those tensors to
`render_frames(..., to_host=False)`, so the cylinder and the pixel boxes take the device path too and no pose row
crosses PCIe.  The cameras stay on the host: F 4x4 matrices the renderer reads there anyway, computed with the
reference's own float32 products.

`load_retarget` ... `load_correction` are drop-ins with the reference's names, argument order and return order
(NumPy out); `refined=(kps, bones)` is required, since reading the h5 through deepdish is not covered.
`pose_sequence_reference` restates the device path in NumPy float64 (scipy rotations) and is the checker of the tests;
tests/golden/sequences.npz holds the reference loaders' own outputs.

Beyond the reference: `interp="slerp"` interpolates per joint on the rotation group (the lerp of axis-angle vectors
leaves the geodesic and jumps where two keys sit on either side of pi), any tree skeleton up to 128 joints.
Not covered: reading h5 files, mp4 writing, the perfcap `/ 1.05` camera quirk (divide
`render_poses[..., :3, -1]`), gradients through the sequence layer.
"""
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib
from . import rays as host_rays
from .kinematics import PoseOptLayer, SMPLSkeleton, matrix_to_axis_angle, pose_kinematics
from .preprocess import draw_skeletons_3d
from .render import render_frames

KINDS = ("selected", "retarget", "bullet", "poserot", "interpolate", "animate", "bubble", "correction")
N_STEP_DEFAULT = {"interpolate": 10, "animate": 10, "bubble": 5, "correction": 8}  # run_render.py's signatures
CENTER_CAM_DEFAULT = {"bullet": True, "poserot": True, "interpolate": False, "animate": False}
CENTER_KPS_DEFAULT = {"retarget": False, "bullet": True, "poserot": False, "interpolate": False, "animate": False,
                      "bubble": True, "correction": False}
UNDO_ROT = np.array([1.5708, 0., 0.], dtype=np.float32)  # run_render.py:557
H5_MESSAGE = "reading poses from the h5 through deepdish is not covered: pass refined=(kps, bones)"


# ---------------------------------------------------------------- cameras (host, the reference's float32 products)
def rotate_x(phi):
    """skeleton_utils.py:21-27."""
    cos, sin = np.cos(phi), np.sin(phi)
    return np.array([[1, 0, 0, 0], [0, cos, -sin, 0], [0, sin, cos, 0], [0, 0, 0, 1]], dtype=np.float32)


def rotate_z(psi):
    """skeleton_utils.py:29-35."""
    cos, sin = np.cos(psi), np.sin(psi)
    return np.array([[cos, -sin, 0, 0], [sin, cos, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)


def rotate_y(theta):
    """skeleton_utils.py:36-42 (with the reference's sign)."""
    cos, sin = np.cos(theta), np.sin(theta)
    return np.array([[cos, 0, -sin, 0], [0, 1, 0, 0], [sin, 0, cos, 0], [0, 0, 0, 1]], dtype=np.float32)


_ROTATE = {"x": rotate_x, "y": rotate_y, "z": rotate_z}
_AXIS_ID = {"x": 0, "y": 1, "z": 2}


def bullet_angles(n_views):
    """load_data.py:55."""
    return np.linspace(0, math.radians(360), n_views + 1)[:-1]


def generate_bullet_time(c2w, n_views=20, axis="y"):
    """load_data.py:45-60: rotate_{axis}(a) @ c2w for n_views angles of a turn."""
    if axis not in _ROTATE:
        raise NotImplementedError(f"rotate axis {axis} is not defined")
    return np.array([_ROTATE[axis](a) @ c2w for a in bullet_angles(n_views)])


def find_idxs_with_map(selected_idxs, idx_map):
    """run_render.py:473-482: the position of each selected index in idx_map (an index without a match is dropped)."""
    if idx_map is None:
        return selected_idxs
    match_idxs = []
    for sel in selected_idxs:
        for i, m in enumerate(idx_map):
            if m == sel:
                match_idxs.append(i)
                break
    return np.array(match_idxs)


def expand_selected(selected_idxs, length, skip, n_total):
    """load_retarget's clip expansion (run_render.py:521-523): `length` frames from each index at stride `skip`,
    clipped at the dataset's end; as the reference, only when skip > 1 and length > 1."""
    if skip > 1 and length > 1:
        return np.concatenate([np.arange(s, min(s + length, n_total))[::skip] for s in selected_idxs])
    return selected_idxs


# ---------------------------------------------------------------- the plan: K key rows and per-frame tables (host)
def _rows(x, idx):
    """Rows idx of a host array or a tensor on any device, as a float32 NumPy copy (K rows)."""
    idx = np.asarray(idx, dtype=np.int64)
    if isinstance(x, torch.Tensor):
        return x.detach()[torch.as_tensor(idx, device=x.device)].to(torch.float32).cpu().numpy()
    return np.array(np.asarray(x)[idx], dtype=np.float32)


def _focal_rows(focals, idx):
    if isinstance(focals, float):
        return np.array([focals] * len(idx))
    return np.asarray(focals)[idx]


class _Plan:
    """What a render type asks of the device: key_bones (K, NJ, 3) and key_root (K, 3) float32, the per-frame tables
    (first key, second key, base key, pelvis key, axis id; weight, angle), the joint mask, the root mode, and the
    host outputs render_poses, focals, cams."""

    def __init__(self, key_bones, key_root, first, second=None, base=None, pelvis=None, axis=None, weight=None,
                 angle=None, mask=None, root_mode=_lib.ANERF_SEQ_ROOT_KEEP):
        n = len(first)
        col = lambda v, d: np.ascontiguousarray(first if v is None else v, dtype=d).reshape(n)  # noqa: E731
        zero = np.zeros(n)
        self.key_bones, self.key_root = key_bones, key_root
        self.keys = np.ascontiguousarray(np.stack([col(first, np.int32), col(second, np.int32), col(base, np.int32),
                                                   col(pelvis, np.int32),
                                                   col(zero if axis is None else axis, np.int32)], 1))
        self.vals = np.ascontiguousarray(np.stack([col(zero if weight is None else weight, np.float64),
                                                   col(zero if angle is None else angle, np.float64)], 1))
        self.mask = mask
        self.root_mode = root_mode
        self.ref_bones = None  # what the reference's loader returns as `bones` (host, float32), if it returns any


def _interp_tables(n_keys, n_step):
    """load_interpolate's frames (run_render.py:702-710): n_step per consecutive pair, then the last key."""
    w = np.linspace(0, 1.0, n_step, endpoint=False)
    first = np.concatenate([np.repeat(np.arange(n_keys - 1), n_step), [n_keys - 1]])
    second = np.concatenate([np.repeat(np.arange(1, n_keys), n_step), [n_keys - 1]])
    weight = np.concatenate([np.tile(w, n_keys - 1), [0.0]])
    return first, second, weight


def _plan(kind, kps, bones, c2ws, focals, selected_idxs, skel_type, n_bullet, n_step, joints, length, skip, undo_rot,
          center_cam, center_kps, idx_map, init_bones, x_deg, y_deg, z_t, selected_framecode):
    if kind not in KINDS:
        raise NotImplementedError(f"render type {kind} is not implemented!")
    root = int(skel_type.root_id)
    nj = len(skel_type.joint_trees)
    sel = np.asarray(selected_idxs).reshape(-1)
    if n_step is None:
        n_step = N_STEP_DEFAULT.get(kind)
    if center_cam is None:
        center_cam = CENTER_CAM_DEFAULT.get(kind, False)
    if center_kps is None:
        center_kps = CENTER_KPS_DEFAULT.get(kind, False)
    c2ws = np.asarray(c2ws.detach().cpu().numpy() if isinstance(c2ws, torch.Tensor) else c2ws)
    if isinstance(focals, torch.Tensor):
        focals = focals.detach().cpu().numpy()
    if kind == "retarget":
        sel = np.asarray(expand_selected(sel, length, skip, len(c2ws)))
    if kind == "correction":
        if init_bones is None:
            raise ValueError("correction needs init_bones, the poses the refinement started from")
        midx = sel  # (load_correction indexes both pose sets by the selected indices themselves)
    else:
        midx = np.asarray(find_idxs_with_map(sel, idx_map)).reshape(-1)
    if kind == "poserot" and len(midx) != 1:
        raise ValueError(f"poserot rotates the root of one pose, {len(midx)} are selected")
    if len(midx) < 1:
        raise ValueError("no pose is selected")

    # cameras, as the loaders' first lines
    cam_sel = midx if kind == "poserot" else sel  # (load_pose_rotate indexes the cameras after the idx_map lookup)
    c2w_k = np.array(c2ws[cam_sel])
    shift = None
    if kind == "bubble" or (center_cam and kind in ("bullet", "interpolate", "animate")):
        shift = (c2w_k[..., 0, -1].copy(), c2w_k[..., 1, -1].copy())
        c2w_k[..., :2, -1] = 0.
    focal_k = _focal_rows(focals, cam_sel)

    # key rows and the centring rules (float32, on K rows)
    kp_k = _rows(kps, midx)
    bone_k = _rows(bones, midx)
    if bone_k.shape[1:] != (nj, 3):
        raise ValueError(f"bones must be (N, {nj}, 3) axis-angle, got {bone_k.shape}")
    if kind == "bubble" or (center_kps and kind in ("retarget", "bullet", "interpolate", "animate")):
        kp_k -= kp_k[..., root:root + 1, :].copy()
    elif shift is not None:
        kp_k[..., :, 0] -= shift[0][:, None]
        kp_k[..., :, 1] -= shift[1][:, None]
    if undo_rot and kind in ("retarget", "bullet", "interpolate", "animate"):
        bone_k[..., root, :] = UNDO_ROT.reshape(1, 3)
    key_root = np.ascontiguousarray(kp_k[:, root])
    n_k = len(midx)
    ar = np.arange(n_k)

    if kind in ("selected", "retarget"):
        plan = _Plan(bone_k, key_root, ar)
        poses, foc, cams = c2w_k, focal_k, (sel if kind == "retarget" else midx)
        if kind == "retarget":
            plan.ref_bones = bone_k
    elif kind == "bullet":
        plan = _Plan(bone_k, key_root, np.repeat(ar, n_bullet))
        poses = generate_bullet_time(c2w_k, n_bullet).transpose(1, 0, 2, 3).reshape(-1, 4, 4)
        foc = focal_k[:, None].repeat(n_bullet, 1).reshape(-1)
        cams = midx[:, None].repeat(n_bullet, 1).reshape(-1)
        plan.ref_bones = bone_k
    elif kind == "poserot":
        n_views = n_bullet // 3
        if n_views < 1:
            raise ValueError("poserot needs n_bullet >= 3 (a third of the views per axis)")
        n = 3 * n_views
        axis = np.repeat([_AXIS_ID["y"], _AXIS_ID["x"], _AXIS_ID["z"]], n_views)  # run_render.py:644-647
        plan = _Plan(bone_k, key_root, np.zeros(n, np.int32), axis=axis, angle=np.tile(bullet_angles(n_views), 3),
                     root_mode=_lib.ANERF_SEQ_ROOT_COMPOSE)
        poses, foc, cams = c2w_k.repeat(n, 0), focal_k.repeat(n, 0), midx.repeat(n, 0)
    elif kind in ("interpolate", "animate"):
        first, second, weight = _interp_tables(n_k, n_step)
        zero = np.zeros(len(first), np.int32)
        mask = None
        if kind == "animate":
            if joints is None:
                raise ValueError("animate needs joints, the joints to interpolate")
            mask = np.zeros(nj, np.uint8)
            mask[np.asarray(joints, dtype=np.int64).reshape(-1)] = 1
        plan = _Plan(bone_k, key_root, first, second, base=zero, pelvis=zero, weight=weight, mask=mask)
        n = len(first)
        poses, foc, cams = c2w_k[:1].repeat(n, 0), focal_k[:1].repeat(n, 0), midx[:1].repeat(n, 0)
    elif kind == "bubble":
        plan = _Plan(bone_k, key_root, np.repeat(ar, n_step))
        x_rad, y_rad = x_deg * np.pi / 180., y_deg * np.pi / 180.
        z_t = z_t * c2w_k[0, 2, -1]
        motions = np.linspace(0., 2 * np.pi, n_step, endpoint=True)
        x_motions, y_motions = (np.cos(motions) - 1.) * x_rad, np.sin(motions) * y_rad
        z_trans = (np.sin(motions) + 1.) * z_t
        cam_motions = [rotate_x(xm) @ rotate_y(ym) for xm, ym in zip(x_motions, y_motions)]
        bubble = []
        for c2w in c2w_k:
            for cam_motion, z_tran in zip(cam_motions, z_trans):
                c = c2w.copy()
                c[2, -1] += z_tran
                bubble.append(cam_motion @ c)
        poses = np.array(bubble).reshape(-1, 4, 4)
        foc = focal_k[:, None].repeat(n_step, 1).reshape(-1)
        cams = midx[:, None].repeat(n_step, 1).reshape(-1)
    else:  # correction: from the initial bones (keys 0 .. S-1) to the refined ones (keys S .. 2S-1)
        init_k = _rows(init_bones, sel)
        if init_k.shape != bone_k.shape:
            raise ValueError(f"init_bones rows are {init_k.shape}, the refined ones {bone_k.shape}")
        w = np.linspace(0, 1.0, n_step, endpoint=False)
        first = np.repeat(ar, n_step)
        plan = _Plan(np.concatenate([init_k, bone_k], 0), np.concatenate([key_root, key_root], 0), first,
                     second=first + n_k, pelvis=first + n_k, weight=np.tile(w, n_k))
        poses = c2w_k[:, None].repeat(n_step, 1).reshape(-1, 4, 4)
        foc = focal_k[:, None].repeat(n_step, 1).reshape(-1)
        cams = sel[:, None].repeat(n_step, 1).reshape(-1)
    cams = np.array(cams, dtype=np.int64)
    if selected_framecode is not None:
        cams[:] = selected_framecode
    plan.render_poses, plan.focals, plan.cams = poses, np.asarray(foc), cams
    plan.n_frames = plan.keys.shape[0]
    return plan


# ---------------------------------------------------------------- the result
class RenderSequence:
    """kp (F, NJ, 3), skts (F, NJ, 4, 4), bones (F, NJ, 3), l2ws (F, NJ, 4, 4): float32 device tensors (NumPy float64
    from pose_sequence_reference); render_poses (F, 4, 4), focals (F,), cams (F,) int64: NumPy."""

    def __init__(self, kind, kp, skts, bones, l2ws, render_poses, focals, cams, ref_bones=None):
        self.kind = kind
        self.kp, self.skts, self.bones, self.l2ws = kp, skts, bones, l2ws
        self.render_poses, self.focals, self.cams = render_poses, focals, cams
        self.ref_bones = ref_bones

    def __len__(self):
        return int(self.render_poses.shape[0])

    def render_kwargs(self, H, W, render_res=None):
        """The ret_dict of load_render_data (run_render.py:285-291).  With render_res = (H_r, W_r) the focals are
        scaled by H_r / H and the frames are H_r x W_r (run_render.py:166-172; one side is checked, as there)."""
        focals = np.array(self.focals, copy=True)
        if render_res is not None:
            if len(render_res) != 2:
                raise ValueError("Image resolution should be in (H, W)")
            H_r, W_r = render_res
            focals = focals * (float(H_r) / float(H))
            H, W = int(H_r), int(W_r)
        return {"kp": self.kp, "skts": self.skts, "render_poses": self.render_poses, "cams": self.cams,
                "hwf": (H, W, focals), "bones": self.bones, "bg_imgs": None, "bg_indices": None, "subject_idxs": None}


_OPTIONS = dict(skel_type=SMPLSkeleton, n_bullet=30, n_step=None, joints=None, length=1, skip=1, undo_rot=False,
                center_cam=None, center_kps=None, idx_map=None, init_bones=None, x_deg=15., y_deg=25., z_t=0.1,
                interp="linear", selected_framecode=None, device=None)


def _options(kw):
    unknown = set(kw) - set(_OPTIONS)
    if unknown:
        raise TypeError(f"pose_sequence got unexpected options {sorted(unknown)}")
    o = dict(_OPTIONS)
    o.update(kw)
    if o["interp"] not in _lib.ANERF_SEQ_INTERPS:
        raise ValueError(f"interp must be 'linear' or 'slerp', got {o['interp']!r}")
    return o


def _plan_of(kind, kps, bones, c2ws, focals, selected_idxs, o):
    return _plan(kind, kps, bones, c2ws, focals, selected_idxs, o["skel_type"], o["n_bullet"], o["n_step"], o["joints"],
                 o["length"], o["skip"], o["undo_rot"], o["center_cam"], o["center_kps"], o["idx_map"],
                 o["init_bones"], o["x_deg"], o["y_deg"], o["z_t"], o["selected_framecode"])


def sequence_bones(key_bones, key_root, keys, vals, skel_type=SMPLSkeleton, mask=None, interp="linear",
                   root_mode=_lib.ANERF_SEQ_ROOT_KEEP, root_const=None, device=None):
    """`anerf_sequence_bones`: key_bones (K, NJ, 3), key_root (K, 3) and the per-frame tables keys (F, 5) int32 /
    vals (F, 2) float64 (include/anerf.h) -> bones (F, NJ, 3), pelvis (F, 3), float32 device tensors.  The tables are
    checked on the host by the library and uploaded here, once."""
    if device is None:
        device = key_bones.device if isinstance(key_bones, torch.Tensor) and key_bones.is_cuda else \
            torch.device("cuda", 0)
    device = torch.device(device)
    kb = (key_bones.detach().to(device=device, dtype=torch.float32) if isinstance(key_bones, torch.Tensor)
          else torch.as_tensor(np.ascontiguousarray(key_bones, dtype=np.float32), device=device)).contiguous()
    kr = (key_root.detach().to(device=device, dtype=torch.float32) if isinstance(key_root, torch.Tensor)
          else torch.as_tensor(np.ascontiguousarray(key_root, dtype=np.float32), device=device)).contiguous()
    nj = len(skel_type.joint_trees)
    if kb.dim() != 3 or tuple(kb.shape[1:]) != (nj, 3) or tuple(kr.shape) != (kb.shape[0], 3):
        raise ValueError(f"key_bones must be (K, {nj}, 3) and key_root (K, 3)")
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    n = int(keys.shape[0])
    if keys.shape != (n, 5) or vals.shape != (n, 2):
        raise ValueError("the frame tables must be keys (F, 5) and vals (F, 2)")
    keys_d, vals_d = torch.from_numpy(keys).to(device), torch.from_numpy(vals).to(device)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(nj)
    rc_ = None if root_const is None else np.ascontiguousarray(root_const, dtype=np.float32).reshape(3)
    out = torch.empty(max(n, 0), nj, 3, dtype=torch.float32, device=device)
    pel = torch.empty(max(n, 0), 3, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        rc = _lib.load().anerf_sequence_bones(
            _lib.ptr(kb), _lib.ptr(kr), int(kb.shape[0]), nj, int(skel_type.root_id),
            keys.ctypes.data_as(_lib.c_i32p), vals.ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_double)),
            _lib.ptr(keys_d), _lib.ptr(vals_d),
            None if m is None else m.ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_uint8)), n,
            _lib.ANERF_SEQ_INTERPS[interp], int(root_mode), None if rc_ is None else rc_.ctypes.data_as(_lib.c_f),
            _lib.ptr(out), _lib.ptr(pel), _lib.stream_handle(device))
    _lib.check(rc, "anerf_sequence_bones")
    return out, pel


@torch.no_grad()
def pose_sequence(kind, kps, bones, c2ws, focals, rest_pose, selected_idxs, **kw):
    """The sequence of one render type (module docstring) -> RenderSequence with device tensors.

    kps (N, NJ, 3) and bones (N, NJ, 3) axis-angle: the (refined) poses, host arrays or tensors; c2ws (N, 4, 4),
    focals (N,) or a float; rest_pose (NJ, 3); selected_idxs: the indices the render type starts from.  Options
    (defaults per kind as in run_render.py): skel_type, n_bullet=30, n_step, joints, length=1, skip=1, undo_rot,
    center_cam, center_kps, idx_map, init_bones (correction), x_deg=15, y_deg=25, z_t=0.1 (bubble),
    interp="linear" | "slerp", selected_framecode, device."""
    o = _options(kw)
    plan = _plan_of(kind, kps, bones, c2ws, focals, selected_idxs, o)
    device = o["device"]
    if device is None:
        device = next((x.device for x in (bones, kps) if isinstance(x, torch.Tensor) and x.is_cuda),
                      torch.device("cuda", 0))
    skel = o["skel_type"]
    b, pel = sequence_bones(plan.key_bones, plan.key_root, plan.keys, plan.vals, skel, mask=plan.mask,
                            interp=o["interp"], root_mode=plan.root_mode, device=device)
    out = pose_kinematics(b, rest_pose, skel, pelvis=pel, device=torch.device(device), outputs=("kps", "skts", "l2ws"))
    return RenderSequence(kind, out["kps"], out["skts"], b, out["l2ws"], plan.render_poses, plan.focals, plan.cams,
                          plan.ref_bones)


# ---------------------------------------------------------------- the checker (NumPy float64, scipy rotations)
def _scipy_rotation():
    from scipy.spatial.transform import Rotation
    return Rotation


def matrix_to_axis_angle_reference(R):
    """(..., 3, 3) matrices or (..., 6) parameters -> axis-angle (..., 3) float64: scipy's
    Rotation.from_matrix(...).as_rotvec() (6-D parameters through rot6d_to_rotmat first)."""
    R = np.asarray(R, dtype=np.float64)
    if R.shape[-1] == 6 and R.shape[-2:] != (3, 3):
        R = rot6d_to_rotmat_reference(R)
    lead = R.shape[:-2]
    return _scipy_rotation().from_matrix(R.reshape(-1, 3, 3)).as_rotvec().reshape(lead + (3,))


def rot6d_to_rotmat_reference(x):
    """skeleton_utils.py:420-436 in float64 (F.normalize's eps 1e-12)."""
    x = np.asarray(x, dtype=np.float64)
    lead = x.shape[:-1]
    x = x.reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=-1, keepdims=True), 1e-12)
    c = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = c / np.maximum(np.linalg.norm(c, axis=-1, keepdims=True), 1e-12)
    return np.stack([b1, b2, np.cross(b1, b2)], -1).reshape(lead + (3, 3))


def matrix_to_axis_angle_formula(R):
    """The device kernel's formula in NumPy float64 -- pytorch3d's matrix_to_quaternion (the best conditioned of the
    four candidates), normalised, real part >= 0, then quaternion_to_axis_angle with its series below 1e-6 -- for the
    tests to measure its agreement with scipy."""
    R = np.asarray(R, dtype=np.float64)
    lead = R.shape[:-2]
    m = R.reshape(-1, 9)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[:, i] for i in range(9))
    s = np.maximum(0.0, np.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22,
                                  1 - m00 - m11 + m22], -1))
    cand = np.stack([np.stack([s[:, 0], m21 - m12, m02 - m20, m10 - m01], -1),
                     np.stack([m21 - m12, s[:, 1], m10 + m01, m02 + m20], -1),
                     np.stack([m02 - m20, m10 + m01, s[:, 2], m12 + m21], -1),
                     np.stack([m10 - m01, m20 + m02, m21 + m12, s[:, 3]], -1)], 1)
    best = np.argmax(s, -1)
    rows = np.arange(len(m))
    q = cand[rows, best] / (2.0 * np.maximum(np.sqrt(s[rows, best]), 0.1))[:, None]
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    q = np.where(q[:, :1] < 0, -q, q)
    n = np.linalg.norm(q[:, 1:], axis=-1)
    half = np.arctan2(n, q[:, 0])
    a = 2.0 * half
    small = a < 1e-6
    sho = np.where(small, 0.5 - a * a / 48.0, np.sin(half) / np.where(small, 1.0, a))
    return (q[:, 1:] / sho[:, None]).reshape(lead + (3,))


def _axis_matrix(axis, angle):
    """The 3x3 of rotate_x / _y / _z in float64 (rotate_y with the reference's sign)."""
    c, s = np.cos(angle), np.sin(angle)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    if axis == 1:
        return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], dtype=np.float64)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def kinematic_chain_reference(bones, rest_pose, skel_type=SMPLSkeleton, pelvis=None):
    """get_smpl_l2ws (skeleton_utils.py:334-376) over a batch, for any tree: bones (F, NJ, 3) axis-angle ->
    kps (F, NJ, 3), skts, l2ws (F, NJ, 4, 4) in float64; pelvis (F, 3) is added to every translation."""
    Rot = _scipy_rotation()
    bones = np.asarray(bones, dtype=np.float64)
    n, nj = bones.shape[:2]
    rest = np.asarray(rest_pose, dtype=np.float64).reshape(nj, 3)
    parents = np.asarray(skel_type.joint_trees)
    root = int(skel_type.root_id)
    R = Rot.from_rotvec(bones.reshape(-1, 3)).as_matrix().reshape(n, nj, 3, 3)
    l2ws = np.zeros((n, nj, 4, 4))
    done = np.zeros(nj, bool)
    loc = np.zeros((n, 4, 4))
    loc[:, 3, 3] = 1.0
    loc[:, :3, :3], loc[:, :3, 3] = R[:, root], rest[root]
    l2ws[:, root] = loc
    done[root] = True
    while not done.all():
        progressed = False
        for j in range(nj):
            p = int(parents[j])
            if done[j] or not done[p]:
                continue
            loc = np.zeros((n, 4, 4))
            loc[:, 3, 3] = 1.0
            loc[:, :3, :3], loc[:, :3, 3] = R[:, j], rest[j] - rest[p]
            l2ws[:, j] = l2ws[:, p] @ loc
            done[j] = progressed = True
        if not progressed:
            raise ValueError("the skeleton's parents do not form a tree under its root")
    if pelvis is not None:
        l2ws[..., :3, 3] += np.asarray(pelvis, dtype=np.float64)[:, None]
    return l2ws[..., :3, 3].copy(), np.linalg.inv(l2ws), l2ws


def sequence_bones_reference(key_bones, key_root, keys, vals, skel_type=SMPLSkeleton, mask=None, interp="linear",
                             root_mode=_lib.ANERF_SEQ_ROOT_KEEP, root_const=None):
    """What anerf_sequence_bones computes, before its rounding: bones (F, NJ, 3), pelvis (F, 3) in float64."""
    Rot = _scipy_rotation()
    kb = np.array(key_bones, dtype=np.float64)
    root = int(skel_type.root_id)
    if root_mode == _lib.ANERF_SEQ_ROOT_CONST:
        kb[:, root] = np.asarray(root_const, dtype=np.float32).astype(np.float64)
    keys, vals = np.asarray(keys), np.asarray(vals, dtype=np.float64)
    a, b = kb[keys[:, 0]], kb[keys[:, 1]]
    w = vals[:, 0].reshape(-1, 1, 1)
    if interp == "linear":
        out = a * (1 - w) + b * w
    else:
        n, nj = a.shape[:2]
        ra, rb = Rot.from_rotvec(a.reshape(-1, 3)), Rot.from_rotvec(b.reshape(-1, 3))
        rel = (ra.inv() * rb).as_rotvec() * np.broadcast_to(w, (n, nj, 1)).reshape(-1, 1)
        out = (ra * Rot.from_rotvec(rel)).as_rotvec().reshape(n, nj, 3)
    if mask is not None:
        # load_animate writes its float64 interpolation into a copy of the float32 first key (run_render.py:613-614):
        # there, alone among the loaders, the reference chains bones that were rounded to float32, as the device does
        keep = np.asarray(mask).reshape(-1) == 0
        out[:, keep] = kb[keys[:, 2]][:, keep]
        out = out.astype(np.float32).astype(np.float64)
    if root_mode == _lib.ANERF_SEQ_ROOT_COMPOSE:
        for f in range(len(out)):
            M = _axis_matrix(int(keys[f, 4]), vals[f, 1]) @ Rot.from_rotvec(out[f, root]).as_matrix()
            out[f, root] = Rot.from_matrix(M).as_rotvec()
    return out, np.asarray(key_root, dtype=np.float64)[keys[:, 3]]


def pose_sequence_reference(kind, kps, bones, c2ws, focals, rest_pose, selected_idxs, **kw):
    """pose_sequence in NumPy float64 (the checker): the same plan, the frames' bones in float64 as the reference
    chains them (they are NOT rounded to float32 first), scipy rotations, get_smpl_l2ws's chain and np.linalg.inv."""
    o = _options(kw)
    plan = _plan_of(kind, kps, bones, c2ws, focals, selected_idxs, o)
    skel = o["skel_type"]
    b, pel = sequence_bones_reference(plan.key_bones, plan.key_root, plan.keys, plan.vals, skel, mask=plan.mask,
                                      interp=o["interp"], root_mode=plan.root_mode)
    kp, skts, l2ws = kinematic_chain_reference(b, rest_pose, skel, pelvis=pel)
    return RenderSequence(kind, kp, skts, b, l2ws, plan.render_poses, plan.focals, plan.cams, plan.ref_bones)


# ---------------------------------------------------------------- drop-in loaders (run_render.py:484-865)
def _refined(refined):
    if refined is None:
        raise NotImplementedError(H5_MESSAGE)
    return refined


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def load_correction(pose_h5, c2ws, focals, rest_pose, pose_keys, selected_idxs, n_step=8, refined=None,
                    center_kps=False, idx_map=None, init=None):
    """run_render.py:484-514; init=(kps, bones) stands for its h5 read -> kps, skts, c2ws, cam_idxs, focals."""
    kps, bones = _refined(refined)
    if init is None:
        raise NotImplementedError(H5_MESSAGE.replace("refined=", "init="))
    s = pose_sequence("correction", kps, bones, c2ws, focals, rest_pose, selected_idxs, n_step=n_step,
                      init_bones=init[1])
    return _host(s.kp), _host(s.skts), s.render_poses, s.cams, s.focals


def load_retarget(pose_h5, c2ws, focals, rest_pose, pose_keys, selected_idxs, length, skip=1, refined=None,
                  center_kps=False, idx_map=None, is_surreal=False, undo_rot=False, is_neuralbody=False):
    """run_render.py:516-563 -> kps, skts, c2ws, cam_idxs, focals, bones."""
    kps, bones = _refined(refined)
    s = pose_sequence("retarget", kps, bones, c2ws, focals, rest_pose, selected_idxs, length=length, skip=skip,
                      center_kps=center_kps, idx_map=idx_map, undo_rot=undo_rot)
    return _host(s.kp), _host(s.skts), s.render_poses, s.cams, s.focals, s.ref_bones


def load_animate(pose_h5, c2ws, focals, rest_pose, pose_keys, selected_idxs, joints, n_step=10, refined=None,
                 undo_rot=False, center_cam=False, center_kps=False, idx_map=None):
    """run_render.py:565-623 -> kps, skts, c2ws, cam_idxs, focals."""
    kps, bones = _refined(refined)
    s = pose_sequence("animate", kps, bones, c2ws, focals, rest_pose, selected_idxs, joints=joints, n_step=n_step,
                      undo_rot=undo_rot, center_cam=center_cam, center_kps=center_kps, idx_map=idx_map)
    return _host(s.kp), _host(s.skts), s.render_poses, s.cams, s.focals


def load_pose_rotate(pose_h5, c2ws, focals, rest_pose, pose_keys, selected_idxs, refined=None, n_bullet=30,
                     undo_rot=False, center_cam=True, center_kps=False, idx_map=None):
    """run_render.py:626-662 -> kps, skts, bones, c2ws, cam_idxs, focals."""
    kps, bones = _refined(refined)
    s = pose_sequence("poserot", kps, bones, c2ws, focals, rest_pose, selected_idxs, n_bullet=n_bullet,
                      idx_map=idx_map)
    return _host(s.kp), _host(s.skts), _host(s.bones), s.render_poses, s.cams, s.focals


def load_interpolate(pose_h5, c2ws, focals, rest_pose, pose_keys, selected_idxs, n_step=10, refined=None,
                     undo_rot=False, center_cam=False, center_kps=False, idx_map=None):
    """run_render.py:664-719 -> kps, skts, c2ws, cam_idxs, focals."""
    kps, bones = _refined(refined)
    s = pose_sequence("interpolate", kps, bones, c2ws, focals, rest_pose, selected_idxs, n_step=n_step,
                      undo_rot=undo_rot, center_cam=center_cam, center_kps=center_kps, idx_map=idx_map)
    return _host(s.kp), _host(s.skts), s.render_poses, s.cams, s.focals


def load_bullettime(pose_h5, c2ws, focals, rest_pose, pose_keys, selected_idxs, refined=None, n_bullet=30,
                    undo_rot=False, center_cam=True, center_kps=True, idx_map=None):
    """run_render.py:721-771 -> kps, skts, c2ws, cam_idxs, focals, bones."""
    kps, bones = _refined(refined)
    s = pose_sequence("bullet", kps, bones, c2ws, focals, rest_pose, selected_idxs, n_bullet=n_bullet,
                      undo_rot=undo_rot, center_cam=center_cam, center_kps=center_kps, idx_map=idx_map)
    return _host(s.kp), _host(s.skts), s.render_poses, s.cams, s.focals, s.ref_bones


def load_selected(pose_h5, c2ws, focals, rest_pose, pose_keys, selected_idxs, refined=None, idx_map=None):
    """run_render.py:773-798 -> kps, skts, c2ws, cam_idxs, focals."""
    kps, bones = _refined(refined)
    s = pose_sequence("selected", kps, bones, c2ws, focals, rest_pose, selected_idxs, idx_map=idx_map)
    return _host(s.kp), _host(s.skts), s.render_poses, s.cams, s.focals


def load_bubble(pose_h5, c2ws, focals, rest_pose, pose_keys, selected_idxs, x_deg=15., y_deg=25., z_t=0.1,
                refined=None, n_step=5, center_kps=True, idx_map=None):
    """run_render.py:800-865 -> kps, skts, c2ws, cam_idxs, focals."""
    kps, bones = _refined(refined)
    s = pose_sequence("bubble", kps, bones, c2ws, focals, rest_pose, selected_idxs, x_deg=x_deg, y_deg=y_deg,
                      z_t=z_t, n_step=n_step, idx_map=idx_map)
    return _host(s.kp), _host(s.skts), s.render_poses, s.cams, s.focals


# ---------------------------------------------------------------- pose checkpoint -> pose data (pose_opt.py:523-559)
LEGACY_ROOT_ANGLE = math.pi / 2  # rot_on_root [[1, 0, 0], [0, 0, -1], [0, 1, 0]] is rotate_x(pi / 2)


def _identity_tables(n, angle=0.0):
    ar = np.arange(n, dtype=np.int32)
    keys = np.stack([ar, ar, ar, ar, np.zeros(n, np.int32)], 1)
    return keys, np.stack([np.zeros(n), np.full(n, angle)], 1)


def _legacy_swap(x):
    """(x, y, z) -> (x, -z, y), pose_opt.py:536-541."""
    return np.concatenate([x[..., :1], -x[..., 2:3], x[..., 1:2]], axis=-1)


def _cylinders(kp3d, ext_scale, skel_type):
    """get_kp_bounding_cylinder(kp3d, ext_scale, skel_type, extend_mm=250, head='-y') with its own default ratios."""
    return host_rays.bounding_cylinder(kp3d, ext_scale, extend_mm=250, top_expand_ratio=1., bot_expand_ratio=0.25,
                                       head="-y", root_id=int(skel_type.root_id)).astype(np.float32)


def load_poseopt_from_state_dict(state_dict, skel_type=SMPLSkeleton, device=None):
    """pose_opt.py:212-238: a PoseOptLayer shaped by, and loaded from, state_dict['poseopt_layer_state_dict']."""
    sd = state_dict["poseopt_layer_state_dict"]
    pelvis, bones = sd["pelvis"], sd["bones"]
    kp_map = kp_uidxs = None
    if "kp_map" in sd:
        kp_map, kp_uidxs = sd["kp_map"].cpu().numpy(), sd["kp_uidxs"].cpu().numpy()
    n, nj, nd = int(pelvis.shape[0]), int(bones.shape[1]), int(bones.shape[2])
    if kp_map is not None:
        nj += 1
    rest = sd["rest_pose"] if "rest_pose" in sd else torch.zeros(1, nj, 3)
    layer = PoseOptLayer(torch.zeros(n, nj, 3), torch.zeros(n, nj, 3), torch.zeros_like(rest.cpu()), skel_type=skel_type,
                         use_rot6d=nd == 6, kp_map=kp_map, kp_uidxs=kp_uidxs, device=device)
    layer.load_state_dict({k: v for k, v in sd.items()})
    return layer


@torch.no_grad()
def pose_ckpt_to_pose_data(path=None, popt_sd=None, ext_scale=0.001, legacy=False, skel_type=SMPLSkeleton,
                           device=None):
    """pose_opt.py:523-559: a `Trainer.save_popt` checkpoint (or its poseopt_layer_state_dict) ->
    (kp3d, bones, skts, cyls, rest_pose, pelvis) as float32 NumPy, the `refined=(kp3d, bones)` of the loaders.
    6-D parameters become axis-angle through matrix_to_axis_angle; `legacy` swaps (x, y, z) -> (x, -z, y) in the
    pelvis (as the reference: its y and z negated), the rest pose and the bones, and re-rotates the root by
    rotate_x(pi / 2).  Chain and inverse run on the device."""
    if popt_sd is None:
        popt_sd = torch.load(path, map_location="cpu", weights_only=True)["poseopt_layer_state_dict"]
    layer = load_poseopt_from_state_dict({"poseopt_layer_state_dict": popt_sd}, skel_type, device)
    dev = layer.device
    pelvis = layer.get_pelvis().detach().cpu().numpy()
    bones_d = layer.get_bones().detach()
    rest_pose = layer.get_rest_pose()[0].detach().cpu().numpy()
    if legacy:
        pelvis[..., 1:] *= -1
        rest_pose = _legacy_swap(rest_pose)
        bones_d = torch.cat([bones_d[..., :1], -bones_d[..., 2:3], bones_d[..., 1:2]], dim=-1).contiguous()
        keys, vals = _identity_tables(int(bones_d.shape[0]), LEGACY_ROOT_ANGLE)
        bones_d, _ = sequence_bones(bones_d, torch.zeros(bones_d.shape[0], 3), keys, vals, skel_type,
                                    root_mode=_lib.ANERF_SEQ_ROOT_COMPOSE, device=dev)
    o = pose_kinematics(bones_d, rest_pose, skel_type, pelvis=pelvis, device=dev, outputs=("kps", "skts"))
    kp3d = o["kps"].cpu().numpy()
    return kp3d, bones_d.cpu().numpy(), o["skts"].cpu().numpy(), _cylinders(kp3d, ext_scale, skel_type), rest_pose, \
        pelvis


def pose_data_reference(pelvis, bones, rest_pose, ext_scale=0.001, legacy=False, skel_type=SMPLSkeleton):
    """pose_ckpt_to_pose_data on the layer's parameters in NumPy float64 (the checker): pelvis (N, 3), bones
    (N, NJ, 3 | 6), rest_pose (NJ, 3) -> (kp3d, bones, skts, cyls, rest_pose, pelvis)."""
    Rot = _scipy_rotation()
    pelvis = np.array(pelvis, dtype=np.float64)
    bones = np.array(bones, dtype=np.float64)
    rest_pose = np.array(rest_pose, dtype=np.float64)
    if bones.shape[-1] == 6:
        bones = matrix_to_axis_angle_reference(bones)
    if legacy:
        root = int(skel_type.root_id)
        pelvis[..., 1:] *= -1
        rest_pose, bones = _legacy_swap(rest_pose), _legacy_swap(bones)
        on_root = np.array([[1., 0., 0.], [0., 0., -1.], [0., 1., 0.]])
        bones[:, root] = Rot.from_matrix(on_root[None] @ Rot.from_rotvec(bones[:, root]).as_matrix()).as_rotvec()
    kp3d, skts, _ = kinematic_chain_reference(bones, rest_pose, skel_type, pelvis=pelvis)
    return kp3d, bones, skts, _cylinders(kp3d.astype(np.float32), ext_scale, skel_type), rest_pose, pelvis


# ---------------------------------------------------------------- frames: render, 8 bits, PNG
def to8b(x):
    """run_nerf.py's to8b, (255 * clip(x, 0, 1)).astype(uint8), on a tensor where it lies (or a NumPy array)."""
    if isinstance(x, torch.Tensor):
        return (255 * torch.clip(x, 0, 1)).to(torch.uint8)
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(path, img_u8):
    """An 8-bit RGB (H, W, 3) or grey (H, W) / (H, W, 1) image as a PNG: zlib from the standard library, filter type
    0 on every row, no interlace."""
    img = _host(img_u8)
    if img.dtype != np.uint8:
        raise ValueError(f"write_png takes uint8, got {img.dtype}")
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[..., 0]
    if img.ndim == 2:
        colour = 0
    elif img.ndim == 3 and img.shape[2] == 3:
        colour = 2
    else:
        raise ValueError(f"write_png takes (H, W), (H, W, 1) or (H, W, 3), got {img.shape}")
    h, w = int(img.shape[0]), int(img.shape[1])
    if h < 1 or w < 1:
        raise ValueError("write_png: an empty image")
    rows = np.ascontiguousarray(img).reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], 1).tobytes()  # (a filter byte 0 before every row)
    blob = b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour, 0, 0, 0)) + \
        _png_chunk(b"IDAT", zlib.compress(raw, 6)) + _png_chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(blob)


def read_png(path):
    """What write_png wrote, back as uint8 (H, W, 3) or (H, W): 8-bit RGB or grey, filter type 0 only."""
    with open(path, "rb") as f:
        blob = f.read()
    if blob[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path} is not a PNG")
    at, chunks = 8, []
    while at < len(blob):
        n, = struct.unpack(">I", blob[at:at + 4])
        tag, data = blob[at + 4:at + 8], blob[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", blob[at + 8 + n:at + 12 + n])
        if zlib.crc32(tag + data) & 0xffffffff != crc:
            raise ValueError(f"{path}: bad CRC in chunk {tag!r}")
        chunks.append((tag, data))
        at += 12 + n
    w, h, depth, colour, _, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if chunks[0][0] != b"IHDR" or depth != 8 or colour not in (0, 2) or flt != 0 or lace != 0:
        raise ValueError(f"{path}: only 8-bit RGB or grey, not interlaced")
    ch = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + w * ch)
    if raw[:, 0].any():
        raise ValueError(f"{path}: only filter type 0 is read")
    img = raw[:, 1:].reshape(h, w, ch)
    return img.copy() if ch == 3 else img[..., 0].copy()


@torch.no_grad()
def render_sequence(seq, H, W, chunk, render_kwargs, *, white_bkgd=False, bg_imgs=None, bg_indices=None,
                    ret_acc=False, ext_scale=0.00035, to_uint8=True, to_host=False, out_dir=None, skeleton=False):
    """Render every frame of a RenderSequence at H x W -> (rgbs (F, H, W, 3), disps (F, H, W, 1), accs (F, H, W, 1) or
    [] without ret_acc): device tensors (NumPy with to_host), rgbs as uint8 through to8b with to_uint8.  The frames
    come from render_frames(..., to_host=False) on the sequence's device tensors.  With out_dir the 8-bit frames are
    also written there as %05d.png.  With skeleton a fourth value follows: the 8-bit frames with the sequence's
    joints drawn through its cameras (run_render.py:1032-1043; preprocess.draw_skeletons_3d), written as
    skel/%05d.png under out_dir."""
    kw = seq.render_kwargs(H, W)
    frames, _, _ = render_frames(kw["render_poses"], kw["hwf"], chunk, render_kwargs, kp=kw["kp"], skts=kw["skts"],
                                 bones=kw["bones"], cams=kw["cams"], bg_imgs=bg_imgs, bg_indices=bg_indices,
                                 white_bkgd=white_bkgd, ret_acc=ret_acc, ext_scale=ext_scale, to_host=False)
    rgbs = torch.stack([f[0] for f in frames], 0)
    disps = torch.stack([f[1] for f in frames], 0)
    accs = torch.stack([f[2] for f in frames], 0) if ret_acc else []
    rgb8 = to8b(rgbs) if (to_uint8 or skeleton or out_dir is not None) else None
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        for i, img in enumerate(rgb8.cpu().numpy()):
            write_png(os.path.join(out_dir, f"{i:05d}.png"), img)
    skels = None
    if skeleton:
        skels = draw_skeletons_3d(rgb8, seq.kp, kw["render_poses"], *kw["hwf"])
        if out_dir is not None:
            os.makedirs(os.path.join(out_dir, "skel"), exist_ok=True)
            for i, img in enumerate(skels.cpu().numpy()):
                write_png(os.path.join(out_dir, "skel", f"{i:05d}.png"), img)
    if to_uint8:
        rgbs = rgb8
    if to_host:
        rgbs, disps = rgbs.cpu().numpy(), disps.cpu().numpy()
        accs = accs.cpu().numpy() if ret_acc else []
        skels = skels.cpu().numpy() if skeleton else None
    if skeleton:
        return rgbs, disps, accs, skels
    return rgbs, disps, accs


__all__ = ["KINDS", "RenderSequence", "pose_sequence", "pose_sequence_reference", "sequence_bones",
           "sequence_bones_reference", "kinematic_chain_reference", "load_correction", "load_retarget", "load_animate",
           "load_pose_rotate", "load_interpolate", "load_bullettime", "load_selected", "load_bubble",
           "matrix_to_axis_angle", "matrix_to_axis_angle_reference", "matrix_to_axis_angle_formula",
           "rot6d_to_rotmat_reference", "pose_ckpt_to_pose_data", "pose_data_reference",
           "load_poseopt_from_state_dict", "render_sequence", "write_png", "read_png", "to8b", "find_idxs_with_map",
           "expand_selected", "generate_bullet_time", "rotate_x", "rotate_y", "rotate_z"]

"""Golden fixture for the pose and camera sequences of the render CLI: the reference's own run_render.py loaders
(load_selected, load_retarget, load_bullettime, load_pose_rotate, load_interpolate, load_animate, load_bubble,
load_correction, lines 484-865) and core/pose_opt.pose_ckpt_to_pose_data (legacy) run on the CPU, in the style of
make_eval_golden.py, on the seeded case of tests/_sequence_cases.py, each called with refined=(kps, bones).

Stand-ins.  pytorch3d is not available, and run_render / pose_opt need two of its functions through skeleton_utils:
axisang_to_rot and rot_to_axisang.  They are replaced by scipy (Rotation.from_rotvec(...).as_matrix() and
Rotation.from_matrix(...).as_rotvec()), cast to float32 tensors as pytorch3d would return for float32 input.  So the
fixture pins the LOADERS' logic -- which rows, which cameras, which products, in which types -- not pytorch3d's
rounding.  deepdish is a stub; dd.io.load is replaced only for load_correction, to hand back the initial arrays.

Measured scalars, stored with the arrays (bounds of the tests; none comes from the code under test):
  d          the effect of feeding the chain float32 bones where the reference chains float64 ones: the reference's
             get_smpl_l2ws and np.linalg.inv on the float64 bones of the interpolated kinds (interpolate, animate,
             correction, and poserot's float64 root, below), then on the same bones rounded to float32; the largest
             absolute difference over l2ws and skts.
  poserot_d  what load_pose_rotate's float32 steps cost (float32 rotate_* matrices and products, the stand-ins'
             float32 casts): its outputs against the same construction in float64 -- float64 rotate matrices times
             scipy's matrix of the root bone, scipy's as_rotvec, the reference's get_smpl_l2ws -- the largest absolute
             difference over kps, skts and bones.
  ckpt_d     the same for pose_ckpt_to_pose_data(legacy=True): its float32 root re-rotation against float64.

Runs ONLY where the reference is present.  Usage: python tests/golden/make_sequence_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402


def stand_ins(mods):
    import torch
    from scipy.spatial.transform import Rotation

    def axisang_to_rot(axisang):
        a = axisang.detach().cpu().numpy().astype(np.float64)
        return torch.tensor(Rotation.from_rotvec(a.reshape(-1, 3)).as_matrix().reshape(a.shape[:-1] + (3, 3))).float()

    def rot_to_axisang(rot):
        r = rot.detach().cpu().numpy().astype(np.float64)
        return torch.tensor(Rotation.from_matrix(r.reshape(-1, 3, 3)).as_rotvec().reshape(r.shape[:-2] + (3,))).float()

    for m in mods:
        m.axisang_to_rot, m.rot_to_axisang = axisang_to_rot, rot_to_axisang


def chain(sk, bones, rest, pelvis):
    """The reference's chain on a batch: get_smpl_l2ws per frame, + pelvis, np.linalg.inv."""
    l2ws = np.array([sk.get_smpl_l2ws(b, rest, 1.0) for b in bones])
    l2ws[..., :3, -1] += pelvis[:, None]
    return l2ws, np.linalg.inv(l2ws)


def rounding_effect(sk, bones64, rest):
    zero = np.zeros((len(bones64), 3))
    a, ai = chain(sk, bones64, rest, zero)
    b, bi = chain(sk, bones64.astype(np.float32), rest, zero)
    return max(float(np.abs(a - b).max()), float(np.abs(ai - bi).max()))


def main():
    import torch
    from scipy.spatial.transform import Rotation
    cases = importlib.import_module("_sequence_cases")
    _, _, _, _, sk = mg.import_reference()
    rr = importlib.import_module("run_render")
    po = importlib.import_module("core.pose_opt")
    stand_ins((rr, po))
    c = cases.make_case()
    rest = c["rest_pose"]
    out = {k: np.array(v) for k, v in c.items()}
    out["idx_map"] = cases.IDX_MAP
    loaders = {"selected": (rr.load_selected, ("kps", "skts", "c2ws", "cam_idxs", "focals")),
               "retarget": (rr.load_retarget, ("kps", "skts", "c2ws", "cam_idxs", "focals", "bones")),
               "bullet": (rr.load_bullettime, ("kps", "skts", "c2ws", "cam_idxs", "focals", "bones")),
               "poserot": (rr.load_pose_rotate, ("kps", "skts", "bones", "c2ws", "cam_idxs", "focals")),
               "interpolate": (rr.load_interpolate, ("kps", "skts", "c2ws", "cam_idxs", "focals")),
               "animate": (rr.load_animate, ("kps", "skts", "c2ws", "cam_idxs", "focals")),
               "bubble": (rr.load_bubble, ("kps", "skts", "c2ws", "cam_idxs", "focals")),
               "correction": (rr.load_correction, ("kps", "skts", "c2ws", "cam_idxs", "focals"))}
    for name, (sel, kw) in cases.LOADER_ARGS.items():
        fn, names = loaders[cases.kind_of(name)]
        kw = dict(kw)
        if name == "correction":
            class _ASlice:
                def __getitem__(self, item):
                    return item

            # (stands for deepdish's partial read of the selected rows of /kp3d and /bones)
            rr.dd = types.SimpleNamespace(aslice=_ASlice(), io=types.SimpleNamespace(
                load=lambda path, keys, sel=None: (c["kps"][sel[0]].copy(), c["init_bones"][sel[0]].copy())))
        # (the loaders write into the arrays they are given: every call gets its own copies)
        ret = fn("unused.h5", c["c2ws"].copy(), c["focals"].copy(), rest.copy(), ["/kp3d", "/bones"], sel.copy(),
                 refined=(c["kps"].copy(), c["bones"].copy()), **kw)
        assert len(ret) == len(names)
        for k, v in zip(names, ret):
            out[f"{name}_{k}"] = np.asarray(v)
        print(name, {k: (np.asarray(v).shape, str(np.asarray(v).dtype)) for k, v in zip(names, ret)})

    # ---- d: float32 bones where the reference chains float64 ones
    b = c["bones"][cases.SELECTED]
    w = np.linspace(0, 1.0, 3, endpoint=False).reshape(-1, 1, 1)
    interp = np.concatenate([b[i:i + 1] * (1 - w) + b[i + 1:i + 2] * w for i in range(len(b) - 1)] + [b[-1:]], 0)
    anim = b[:1].repeat(len(interp), 0).astype(np.float64)
    anim[:, [16, 18, 20]] = interp[:, [16, 18, 20]]
    corr = np.concatenate([i0[None] * (1 - w) + r0[None] * w for i0, r0 in zip(c["init_bones"][cases.SELECTED], b)], 0)
    # poserot in float64: rotate_{y,x,z}(a) R(root), as load_pose_rotate's order
    bp = c["bones"][cases.SELECTED_POSEROT].astype(np.float64)
    R0 = Rotation.from_rotvec(bp[0, 0]).as_matrix()
    angles = np.linspace(0, np.radians(360), 6 // 3 + 1)[:-1]

    def rot3(axis, a):
        cs, sn = np.cos(a), np.sin(a)
        return {"x": np.array([[1, 0, 0], [0, cs, -sn], [0, sn, cs]]),
                "y": np.array([[cs, 0, -sn], [0, 1, 0], [sn, 0, cs]]),
                "z": np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]])}[axis].astype(np.float64)

    roots = np.array([Rotation.from_matrix(rot3(ax, a) @ R0).as_rotvec() for ax in "yxz" for a in angles])
    prot = bp.repeat(len(roots), 0)
    prot[:, 0] = roots
    d = max(rounding_effect(sk, x, rest) for x in (interp, anim, corr, prot))
    out["d"] = np.float64(d)
    pel = c["kps"][cases.SELECTED_POSEROT][:, 0].astype(np.float64).repeat(len(roots), 0)
    l2ws64, skts64 = chain(sk, prot, rest, pel)
    out["poserot_d"] = np.float64(max(np.abs(l2ws64[..., :3, -1] - out["poserot_kps"]).max(),
                                      np.abs(skts64 - out["poserot_skts"]).max(),
                                      np.abs(prot - out["poserot_bones"]).max()))

    # ---- pose_ckpt_to_pose_data(legacy=True) on an axis-angle layer's state dict
    sd = {"pelvis": torch.tensor(c["kps"][:, 0].copy()), "bones": torch.tensor(c["bones"].copy()),
          "rest_pose": torch.tensor(rest.astype(np.float32))[None]}
    ck = po.pose_ckpt_to_pose_data(popt_sd={k: v.clone() for k, v in sd.items()}, ext_scale=0.001, legacy=True)
    for k, v in zip(("kp3d", "bones", "skts", "cyls", "rest_pose", "pelvis"), ck):
        out[f"ckpt_{k}"] = np.asarray(v)
    sw = lambda x: np.concatenate([x[..., :1], -x[..., 2:3], x[..., 1:2]], -1)  # noqa: E731
    b64 = sw(c["bones"].astype(np.float64))
    on_root = np.array([[1., 0., 0.], [0., 0., -1.], [0., 1., 0.]])
    b64[:, 0] = Rotation.from_matrix(on_root[None] @ Rotation.from_rotvec(b64[:, 0]).as_matrix()).as_rotvec()
    pel64 = c["kps"][:, 0].astype(np.float64)
    pel64[:, 1:] *= -1
    l2, sk64 = chain(sk, b64, sw(rest), pel64)
    out["ckpt_d"] = np.float64(max(np.abs(l2[..., :3, -1] - out["ckpt_kp3d"]).max(),
                                   np.abs(sk64 - out["ckpt_skts"]).max(), np.abs(b64 - out["ckpt_bones"]).max()))
    path = os.path.join(HERE, "sequences.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: float(out[k]) for k in ("d", "poserot_d", "ckpt_d")})


if __name__ == "__main__":
    main()

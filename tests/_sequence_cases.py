"""Shared, seeded inputs and bounds of the pose-sequence tests (tests/test_sequences.py, tests/test_gpu_sequences.py)
and of the fixture maker (tests/golden/make_sequence_golden.py).

* make_case: N = 5 poses of SMPL-24 -- bones ~ 0.4 N(0, 1) with one zero bone, one of norm 1e-8 and one of norm 3.0,
  key points, non-trivial cameras and focals, an idx_map, and the initial bones a correction clip starts from.  The
  rest pose holds float32 values in a float64 array: the reference subtracts parent offsets in the array's own type,
  the device kernel in double, and both must see the same numbers.
* LOADER_ARGS: how the maker calls each of the reference's loaders, and the tests pose_sequence.
* rotations: the seeded matrices of the matrix_to_axis_angle tests.
"""
import functools
import importlib

import numpy as np

syn = importlib.import_module("a-nerf_amd.synthetic")

SEED = 4107
N_POSES = 5
SELECTED = np.array([1, 3, 4])
SELECTED_POSEROT = np.array([3])
IDX_MAP = np.array([4, 3, 0, 1, 9])  # dataset index -> row: 1 -> 3, 3 -> 1, 4 -> 0

# kind -> (selected indices, keyword arguments); "bullet_map" is bullet through the idx_map
LOADER_ARGS = {
    "selected": (SELECTED, {}),
    "retarget": (SELECTED, dict(length=2, skip=1, undo_rot=True)),
    "bullet": (SELECTED, dict(n_bullet=4)),
    "bullet_map": (SELECTED, dict(n_bullet=4, idx_map=IDX_MAP)),
    "poserot": (SELECTED_POSEROT, dict(n_bullet=6)),
    "interpolate": (SELECTED, dict(n_step=3)),
    "animate": (SELECTED, dict(joints=[16, 18, 20], n_step=3)),
    "bubble": (SELECTED, dict(n_step=4)),
    "correction": (SELECTED, dict(n_step=3)),
}
DIRECT_KINDS = ("selected", "retarget", "bullet", "bullet_map", "bubble")  # the chain reads the float32 keys themselves
INTERPOLATED_KINDS = ("poserot", "interpolate", "animate", "correction")  # float32 bones of a float64 formula

# tests/test_kinematics.py's GPU bounds for get_smpl_l2ws: float32 rounding of float64 results
L2W_ATOL, L2W_RTOL = 2.5e-7, 1.2e-7
SKT_ATOL, SKT_RTOL = 5e-7, 2.4e-7
F64_TOL = 1e-12  # the float64 path, as tests/test_kinematics.py gives it
ULP_2_4 = 2.4e-7  # one float32 ulp in [2, 4): the rounding of an axis-angle component (|v| <= pi)


def kind_of(name):
    return "bullet" if name == "bullet_map" else name


@functools.lru_cache(maxsize=None)
def make_case(seed=SEED):
    """-> dict of read-only arrays: kps, bones, init_bones (N, 24, 3) float32, c2ws (N, 4, 4) float32, focals (N,)
    float32, rest_pose (24, 3) float64."""
    rs = np.random.RandomState(seed)
    n = N_POSES
    bones = (0.4 * rs.normal(size=(n, 24, 3))).astype(np.float32)
    bones[1, 5] = 0.0
    u = rs.normal(size=3)
    bones[3, 7] = (1e-8 * u / np.linalg.norm(u)).astype(np.float32)
    u = rs.normal(size=3)
    bones[4, 9] = (3.0 * u / np.linalg.norm(u)).astype(np.float32)
    init_bones = (bones + 0.1 * rs.normal(size=bones.shape)).astype(np.float32)
    kps = (rs.normal(scale=0.5, size=(n, 24, 3)) + np.array([0.3, -0.2, 0.1])).astype(np.float32)
    c2ws = np.stack([syn.camera_c2w(distance=4.0 + 0.5 * i, yaw=0.3 * i - 0.4) for i in range(n)]).astype(np.float32)
    c2ws[:, :3, 3] += rs.normal(scale=0.2, size=(n, 3)).astype(np.float32)
    focals = (300.0 + 17.0 * np.arange(n) + rs.uniform(size=n)).astype(np.float32)
    out = {"kps": kps, "bones": bones, "init_bones": init_bones, "c2ws": c2ws, "focals": focals,
           "rest_pose": syn.REST_POSE_24.astype(np.float32).astype(np.float64)}
    for v in out.values():
        v.setflags(write=False)
    return out


def call_args(case, name):
    """-> (args, kwargs) of pose_sequence / pose_sequence_reference for a LOADER_ARGS entry."""
    sel, kw = LOADER_ARGS[name]
    kw = dict(kw)
    if name == "correction":
        kw["init_bones"] = case["init_bones"]
    return (kind_of(name), case["kps"], case["bones"], case["c2ws"], case["focals"], case["rest_pose"], sel), kw


def skeleton65():
    """The synthetic 65-joint tree (a-nerf_amd/synthetic.skeleton) as a kinematics.Skeleton -> (skeleton, rest)."""
    kin = importlib.import_module("a-nerf_amd.kinematics")
    parents, rest = syn.skeleton(65, seed=3)[:2]
    parents = np.asarray(parents)
    return kin.Skeleton([f"j{i}" for i in range(65)], parents, 0, list(range(1, 65)), {}, []), \
        np.asarray(rest, np.float32)


@functools.lru_cache(maxsize=None)
def rotations(seed=SEED + 1, n=2000):
    """-> (matrices (n + 3 + 64, 3, 3) float32, angles): n rotations with angle uniform in [0, pi - 1e-3] about random
    axes, the identity, two of angle 1e-8, and 64 within 1e-3 of pi; float32 roundings of float64 matrices, so
    orthogonal only to float32 rounding."""
    from scipy.spatial.transform import Rotation
    rs = np.random.RandomState(seed)

    def rot(angles):
        ax = rs.normal(size=(len(angles), 3))
        ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
        return Rotation.from_rotvec(ax * np.asarray(angles)[:, None]).as_matrix()

    ang = np.concatenate([rs.uniform(0.0, np.pi - 1e-3, size=n), [0.0, 1e-8, 1e-8],
                          np.pi - rs.uniform(0.0, 1e-3, size=64)])
    m = rot(ang).astype(np.float32)
    m.setflags(write=False)
    ang.setflags(write=False)
    return m, ang


@functools.lru_cache(maxsize=None)
def formula_agreement():
    """The float64 agreement of the device kernel's formula (sequences.matrix_to_axis_angle_formula: pytorch3d's
    matrix -> quaternion -> axis-angle) with scipy on the float32 matrices of rotations(), rows with angle
    <= pi - 1e-3: the first term of the GPU bound of matrix_to_axis_angle and slerp.  On exactly orthogonal matrices
    the two agree to 1e-15; on float32 roundings scipy first projects onto the nearest rotation (an SVD) and the
    formula reads the quaternion off the matrix as it is, two estimates from entries that are off by up to 2^-24."""
    seq = importlib.import_module("a-nerf_amd.sequences")
    m, ang = rotations()
    far = ang <= np.pi - 1e-3
    return float(np.abs(seq.matrix_to_axis_angle_formula(m) - seq.matrix_to_axis_angle_reference(m))[far].max())

"""Time the pose-sequence layer: `interpolate` over 31 keys with n_step = 10 (301 frames of 24 joints).

  * device_ms         anerf_sequence_bones + anerf_pose_kinematics on tables and keys already on the device, by events
                      after warm-up
  * pose_sequence_ms  sequences.pose_sequence as a user calls it: the host plan, the upload of keys and tables, both
                      launches; wall clock around a synchronise, after warm-up
  * numpy_ms          the float64 NumPy checker on the host (pose_sequence_reference), one run

Writes the numbers to profiles/sequence_bench.json (--out) and prints the same JSON line.  Not a throughput item (a
512 x 512 frame takes about 0.17 s to render): the point is that the layer exists and the poses stay on the device.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

anerf = importlib.import_module("a-nerf_amd")
_lib = importlib.import_module("a-nerf_amd._lib")
seq = importlib.import_module("a-nerf_amd.sequences")
kin = importlib.import_module("a-nerf_amd.kinematics")
syn = importlib.import_module("a-nerf_amd.synthetic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sequence_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    n_keys, n_step, nj = 31, 10, 24
    rs = np.random.RandomState(31)
    kps = rs.normal(scale=0.5, size=(n_keys, nj, 3)).astype(np.float32)
    bones = (0.4 * rs.normal(size=(n_keys, nj, 3))).astype(np.float32)
    c2ws = np.stack([syn.camera_c2w(distance=5.0, yaw=0.1 * i) for i in range(n_keys)])
    focals = np.full(n_keys, 768.0, np.float32)
    rest = syn.REST_POSE_24
    args = ("interpolate", kps, bones, c2ws, focals, rest, np.arange(n_keys))
    dev = torch.device("cuda", 0)
    o = seq._options(dict(n_step=n_step))
    plan = seq._plan_of(*args[:5], args[6], o)
    frames = plan.n_frames
    kb, kr = torch.from_numpy(plan.key_bones).to(dev), torch.from_numpy(plan.key_root).to(dev)
    keys_d, vals_d = torch.from_numpy(plan.keys).to(dev), torch.from_numpy(plan.vals).to(dev)
    out_b = torch.empty(frames, nj, 3, device=dev)
    out_p = torch.empty(frames, 3, device=dev)
    lib = _lib.load()
    st = _lib.stream_handle(dev)
    ct = _lib.ctypes

    def device():
        _lib.check(lib.anerf_sequence_bones(_lib.ptr(kb), _lib.ptr(kr), n_keys, nj, 0,
                                            plan.keys.ctypes.data_as(_lib.c_i32p),
                                            plan.vals.ctypes.data_as(ct.POINTER(ct.c_double)), _lib.ptr(keys_d),
                                            _lib.ptr(vals_d), None, frames, 0, 0, None, _lib.ptr(out_b),
                                            _lib.ptr(out_p), st), "anerf_sequence_bones")
        return kin.pose_kinematics(out_b, rest, pelvis=out_p, device=dev, outputs=("kps", "skts", "l2ws"))

    for _ in range(5):
        device()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        device()
    e1.record()
    torch.cuda.synchronize()
    device_ms = e0.elapsed_time(e1) / a.reps

    for _ in range(5):
        s = seq.pose_sequence(*args, n_step=n_step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        s = seq.pose_sequence(*args, n_step=n_step)
    torch.cuda.synchronize()
    full_ms = (time.perf_counter() - t0) * 1e3 / a.reps

    t0 = time.perf_counter()
    chk = seq.pose_sequence_reference(*args, n_step=n_step)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    out = {"what": "pose_sequence('interpolate'): 31 keys, n_step 10, 24 joints", "frames": int(frames), "joints": nj,
           "reps": a.reps, "device_ms": round(device_ms, 4), "pose_sequence_ms": round(full_ms, 4),
           "numpy_float64_host_ms": round(numpy_ms, 2),
           "bytes_uploaded": int(plan.key_bones.nbytes + plan.key_root.nbytes + plan.keys.nbytes + plan.vals.nbytes),
           "max_abs_skts_device_vs_numpy": float(np.abs(s.skts.cpu().numpy() - chk.skts).max()),
           "max_abs_kps_device_vs_numpy": float(np.abs(s.kp.cpu().numpy() - chk.kp).max())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

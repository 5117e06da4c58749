"""Training-step benchmark through the product's Trainer: tools/train_bench.py's scene and configuration (N_rand 2048
rays, 64 + 16 samples, 8x256 nets, 128 images, kinematic pose optimisation on 6-D rotations), stepped by
`Trainer.train_batch` on anerf.Adam instead of the step written out inline there.  The Trainer does more per step
than that bare step: every statistic (psnr, MPJPC, alpha, the gradient norms), the learning-rate decay, the tau
schedule, and one device read of the statistics buffer per step.

Prints one JSON line: training rays/s, ms_per_step, host_issue_ms_per_step.  (train_batch ends with its one device
read, so the host's issue time is close to the step time: the host waits there, not in the launches.)
Usage: python tools/trainer_bench.py [--steps K] [--warmup W] [--rays N] [--adam kernel|foreach]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_bench  # noqa: E402  (the scene, the configuration and the defaults are that module's)


def parser():
    ap = argparse.ArgumentParser()
    base = train_bench.parser()
    for name in ("steps", "warmup", "rays", "images", "joints", "samples", "importance", "mlp"):
        action = next(x for x in base._actions if x.dest == name)
        ap.add_argument("--" + name, type=action.type, default=action.default, choices=action.choices)
    ap.add_argument("--adam", default="kernel", choices=["kernel", "foreach"],
                    help="kernel: anerf.Adam (anerf_adam_step); foreach: torch.optim.Adam, the norms by torch ops")
    return ap


def measure(a, dev=None):
    anerf = importlib.import_module("a-nerf_amd")
    syn = importlib.import_module("a-nerf_amd.synthetic")
    train = importlib.import_module("a-nerf_amd.train")
    kin = importlib.import_module("a-nerf_amd.kinematics")
    raycaster = importlib.import_module("a-nerf_amd.raycaster")
    dev = dev or torch.device("cuda:0")
    S, I, n, nj = a.samples, a.importance, a.rays, a.joints
    cfg = anerf.RenderConfig(n_joints=nj, N_samples=S, N_importance=I).validate()
    ck = syn.make_checkpoint(13, n_joints=nj, D=8, W=256, fine=True, tau=20.0)
    sc = syn.make_scene(n_joints=nj, H=512, W=512, seed=13, n_frames=a.images, yaw_step=2 * np.pi / a.images)
    idx, cyls, _ = anerf.rays.valid_pixels(sc["c2ws"], 512, 512, sc["focal"], kps=sc["kps"], ext_scale=0.001)
    rng = np.random.default_rng(0)
    caster = train.TrainRayCaster(cfg, ck, device=dev, mlp=a.mlp).train()
    skel = kin.SMPLSkeleton if nj == 24 else kin.Skeleton(
        [f"j{i}" for i in range(nj)], np.asarray(sc["parents"]), 0, list(range(1, nj)), {}, None)
    layer = kin.PoseOptLayer(sc["kps"], sc["bones"], sc["rest"][None] - sc["rest"][None, :1], skel, use_rot6d=True,
                             device=dev)
    with torch.no_grad():
        kps0, _, _, _, rots0 = layer.calculate_kinematic(np.arange(a.images))
    popt_kwargs = {"popt_layer": layer, "popt_anchors": {"kps": kps0.clone(), "rots": rots0.clone()}}
    # Trainer.train_batch with --opt_pose --opt_rot6d, tol 0.01, coef 2.0 (configs/h36m/h36m_prot2.txt), as train_bench
    args = argparse.Namespace(opt_pose=True, opt_rot6d=True, opt_pose_tol=0.01, opt_pose_coef=2.0, opt_pose_step=1,
                              opt_pose_stop=None, opt_pose_cache=False, use_temp_loss=False, use_background=True,
                              loss_fn="MSE", reg_fn=None, coarse_weight=1.0, lrate=5e-4, lrate_decay=250,
                              lrate_decay_rate=0.1, decay_unit=1000, cutoff_step=250, cutoff_rate=10.0, finetune=False,
                              opt_framecode=False, chunk=1024 * 32, ext_scale=0.001, multires=7)
    common = {"N_importance": I, "N_samples": S, "use_viewdirs": True, "ext_scale": 0.001,
              "preproc_kwargs": {"density_scale": cfg.density_scale}, "lindisp": False, "nerf_type": "nerf"}
    kw_train = {"ray_caster": caster, "perturb": 1.0, "raw_noise_std": 1.0, "ray_noise_std": 0.0, **common}
    kw_test = {"ray_caster": raycaster._EvalView(caster), "perturb": False, "raw_noise_std": 0.0, "ray_noise_std": 0.0,
               **common}
    Adam = anerf.Adam if a.adam == "kernel" else (lambda p, lr: torch.optim.Adam(p, lr=lr, foreach=True))
    trainer = anerf.Trainer(args, {"hwf": (512, 512, sc["focal"])}, Adam(list(caster.parameters()), lr=5e-4),
                            Adam(list(layer.parameters()), lr=5e-4), kw_train, kw_test, popt_kwargs=popt_kwargs)

    def batch():
        img = rng.integers(0, a.images, n)
        o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        for f in np.unique(img):
            sel = np.nonzero(img == f)[0]
            pix = rng.choice(idx[f], len(sel))
            y, x = pix // 512, pix % 512
            c2w = sc["c2ws"][f].astype(np.float64)
            o[sel] = c2w[:3, 3]
            d[sel] = np.stack([(x - 256.0) / sc["focal"], -(y - 256.0) / sc["focal"], -np.ones(len(sel))],
                              -1) @ c2w[:3, :3].T
        return {"rays": torch.from_numpy(np.stack([o, d])).to(dev), "kp_idx": torch.from_numpy(img).to(dev),
                "cyls": torch.from_numpy(cyls[img]).to(dev), "target_s": torch.rand(n, 3, device=dev)}

    batches = [batch() for _ in range(4)]
    for i in range(a.warmup):
        trainer.train_batch(batches[i % 4], i=i, global_step=i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss_dict, stats = trainer.train_batch(batches[i % 4], i=i, global_step=a.warmup + i)
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    return {"metric": "training rays/s (Trainer.train_batch: PoseOptLayer kinematics + render_rays fwd + anerf_train_loss + "
                      "anerf_pose_loss + bwd + anerf_adam_step on both optimizers + every statistic, decay and schedule; "
                      "N_rand 2048, 64+16 samples, 8x256, 128 images)",
            "value": round(n / dt, 1), "unit": "rays/s", "ms_per_step": round(1e3 * dt, 3), "steps": a.steps,
            "host_issue_ms_per_step": round(1e3 * t_issue / a.steps, 3), "mlp": a.mlp, "adam": a.adam, "joints": nj,
            "last_stats": {k: round(float(v), 6) for k, v in stats.items()},
            "data": "synthetic (seeded SMPL-24 poses, 128 cameras on a circle, seeded weights)"}


def main():
    print(json.dumps(measure(parser().parse_args())), flush=True)


if __name__ == "__main__":
    main()

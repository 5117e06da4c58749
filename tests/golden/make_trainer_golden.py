"""Golden fixtures for the TRAINER: K consecutive steps of the reference's own `Trainer.train_batch`
(core/trainer.py:205-517) on the CPU, in the style of make_train_golden.py.

The reference's networks are built by its create_raycaster and loaded with the seeded synthetic checkpoint (checked by
sha256 in the tests); its PoseOptLayer is built the way make_golden.py's kinematics tables build it (`__new__`: its
__init__ needs pytorch3d), on 6-D rotations.  torch.rand / torch.randn are replaced, for the duration of each step, by
a queue of pre-drawn tensors stored in the fixture.  Each fixture holds, per step, the batch and the draws and the
step's loss_dict and stats, and at the end the pose parameters and, per network tensor, a strided sample of the
parameters and the norm of the whole update.

One reference quirk is worked round: in the pose-optimisation branch Trainer.optimize calls get_gradnorm after the
gradients were reset (core/trainer.py:471-473), which with torch >= 2 (set_to_none) divides by zero.  Where that branch
runs, both optimizers' zero_grad is called with set_to_none=False (the norms the reference then reports are 0), and the
norms of the gradients the step used are recorded here, before the step, with the reference's own get_gradnorm.

Runs ONLY where the reference is present.  Usage: python tests/golden/make_trainer_golden.py [NAME ...]
"""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

CONFIGS = {
    # t1's net; pose optimisation on 6-D rotations with the temporal loss, a pose step every second iteration and
    # none from iteration 4 on; lrate and tau both move within the 6 steps
    "tr1_popt_d4w128": dict(H=128, NJ=24, S=32, I=16, D=4, W=128, tau=20.0, seed=61, n_rays=64, n_poses=4, K=6,
                            popt=True,
                            flags=["--loss_fn", "MSE", "--use_background", "--opt_pose", "--opt_rot6d",
                                   "--use_temp_loss", "--temp_coef", "0.05", "--opt_pose_step", "2",
                                   "--opt_pose_stop", "4", "--opt_pose_tol", "0.005", "--opt_pose_coef", "2.0",
                                   "--opt_pose_lrate", "0.0005", "--lrate", "0.0005", "--lrate_decay", "4",
                                   "--decay_unit", "2", "--cutoff_step", "1", "--cutoff_rate", "10.0"]),
    # no pose layer: the batch carries the poses; Huber + the BCE regulariser on fgs, a coarse weight.  The seeded
    # 8 x 256 nets are opaque along most rays of the box, and where acc is within float32 rounding of 1 the
    # regulariser's log(1 - acc + 1e-8) turns that rounding (6e-8 of a transmittance of 1e-6) into percents of reg_loss:
    # such a fixture pins the rounding of acc, not the step (measured: reg_loss0 off by 2 % at step 0, for the
    # product and for torch alike).  So each step's rays are the first 32 of 16 x 32 candidates whose acc stays below
    # max_acc in both passes at the step's weights, and the seed is one whose net leaves enough of them
    "tr2_nopopt_d8w256": dict(H=128, NJ=24, S=32, I=16, D=8, W=256, tau=20.0, seed=66, n_rays=32, n_poses=2, K=3,
                              popt=False, candidates=16, max_acc=0.999,
                              flags=["--loss_fn", "Huber", "--loss_beta", "0.1", "--use_background", "--reg_fn", "BCE",
                                     "--reg_coef", "0.1", "--coarse_weight", "0.5", "--lrate", "0.0005",
                                     "--lrate_decay", "4", "--decay_unit", "2", "--cutoff_step", "1",
                                     "--cutoff_rate", "10.0"]),
}
GLOBAL_STEP = 100  # train_batch(i, global_step = GLOBAL_STEP * i): tau = 20 * 10 ** (0.1 i)
SAMPLE = 2048      # network tensors with more entries are sampled (sample_idx)


def sample_idx(numel):
    return np.arange(0, numel, max(1, numel // SAMPLE))[:SAMPLE]


def rot6d_of(bones):
    """Axis-angle bones (N, NJ, 3) -> the [:3, :2] block of their rotation matrices, row-major (N, NJ, 6)."""
    N, nj = bones.shape[:2]
    out = np.zeros((N, nj, 6), np.float32)
    for f in range(N):
        for j in range(nj):
            out[f, j] = mg.anerf_syn.rotvec_to_matrix(bones[f, j])[:3, :2].reshape(6)
    return out


def reference_layer(mods, bones6, pelvis, rest):
    import torch
    po = importlib.import_module("core.pose_opt")
    L = po.PoseOptLayer.__new__(po.PoseOptLayer)  # (__init__ would call pytorch3d's axis_angle_to_matrix)
    torch.nn.Module.__init__(L)
    L.skel_type, L.use_cache, L.unroll_kinematic_chain, L.use_rot6d = mods[4].SMPLSkeleton, False, True, True
    L.rest_pose_idxs, L.kp_map, L.kp_uidxs, L.root_id, L.N_kps = None, None, None, 0, len(pelvis)
    L.register_buffer("rest_pose", torch.tensor(rest))
    L.register_parameter("pelvis", torch.nn.Parameter(torch.tensor(pelvis)))
    L.register_parameter("bones", torch.nn.Parameter(torch.tensor(bones6)))
    return L


def build(mods, cfg, tmp):
    """The reference's create_raycaster with the fixture's training flags -> (args, kwargs_train, kwargs_test,
    optimizer, checkpoint)."""
    import torch
    run_nerf, _, raycasters, _, sk = mods
    argv = ["--N_samples", str(cfg["S"]), "--N_importance", str(cfg["I"]), "--netdepth", str(cfg["D"]),
            "--netwidth", str(cfg["W"]), "--multires", "7", "--multires_views", "4", "--use_cutoff",
            "--cutoff_viewdir", "--cutoff_inputs", "--use_viewdirs", "--ext_scale", "0.001", "--chunk", "4096",
            "--no_reload", "--basedir", tmp, "--expname", "x", "--raw_noise_std", "1.0", "--perturb", "1.0"]
    args = run_nerf.config_parser().parse_args(argv + cfg.get("model_flags", []) + cfg["flags"])
    os.makedirs(os.path.join(tmp, "x"), exist_ok=True)
    data_attrs = {"skel_type": sk.SMPLSkeleton, "near": 0.0, "far": 1.0, "n_views": 5,
                  "joint_coords": np.zeros((cfg["NJ"], 3, 3), np.float32)}
    kw_train, kw_test, _, _, optimizer, _ = raycasters.create_raycaster(args, data_attrs)
    ck = mg.anerf_syn.make_checkpoint(cfg["seed"], n_joints=cfg["NJ"], D=cfg["D"], W=cfg["W"], fine=True,
                                      tau=cfg["tau"])
    ck_t = {k: {n: torch.from_numpy(np.array(v)) for n, v in d.items()} for k, d in ck.items()}
    kw_test["ray_caster"].load_state_dict(ck_t, strict=True)
    return args, kw_train, kw_test, optimizer, ck


def make(name, cfg, mods, tmp):
    import torch
    _, trainer, _, ray_utils, _ = mods
    args, kw_train, kw_test, optimizer, ck = build(mods, cfg, os.path.join(tmp, name))
    rc = kw_test["ray_caster"]
    rc.train()
    S, I, NJ, P, K, n = cfg["S"], cfg["I"], cfg["NJ"], cfg["n_poses"], cfg["K"], cfg["n_rays"]
    sc = mg.anerf_syn.make_scene(n_joints=NJ, H=cfg["H"], W=cfg["H"], seed=cfg["seed"], n_frames=P, yaw_step=0.5)
    rng = np.random.default_rng(cfg["seed"] + 2000)
    data = {}
    popt_kwargs, pose_optimizer, layer = None, None, None
    if cfg["popt"]:
        rest = (sc["rest"][None] - sc["rest"][None, :1]).astype(np.float32)
        anchor6, pelvis0 = rot6d_of(sc["bones"]), sc["kps"][:, 0].copy()
        with torch.no_grad():  # the anchors: the dataset's poses through the reference's own chain
            a_kps, _, _, _, a_rots = reference_layer(mods, anchor6, pelvis0, rest).calculate_kinematic(np.arange(P))
        # the layer starts away from its anchors (as after a reload), so the anchor loss and its tolerance both act
        bones6 = (anchor6 + rng.normal(scale=0.05, size=anchor6.shape)).astype(np.float32)
        pelvis = (pelvis0 + rng.normal(scale=0.01, size=pelvis0.shape)).astype(np.float32)
        layer = reference_layer(mods, bones6, pelvis, rest)
        pose_optimizer = torch.optim.Adam(params=list(layer.parameters()), lr=args.opt_pose_lrate, betas=(0.9, 0.999))
        popt_kwargs = {"popt_layer": layer, "popt_anchors": {"kps": a_kps.clone(), "rots": a_rots.clone()}}
        data.update(rest=rest, init_bones6=bones6, init_pelvis=pelvis, anchor_kps=a_kps.numpy(),
                    anchor_rots=a_rots.numpy(), scene_kps=sc["kps"], scene_bones=sc["bones"])
    # rays of every pose once; each step draws its own subset
    per_pose = []
    for f in range(P):
        rays, vids, cyls, _ = ray_utils.kp_to_valid_rays(torch.from_numpy(sc["c2ws"][f:f + 1]), sc["H"], sc["W"],
                                                         sc["focal"], kps=torch.from_numpy(sc["kps"][f:f + 1]),
                                                         ext_scale=0.001)
        per_pose.append((rays[0][0].numpy(), rays[0][1].numpy(), cyls.numpy()[0]))
    T = trainer.Trainer(args, {"hwf": (sc["H"], sc["W"], sc["focal"])}, optimizer, pose_optimizer, kw_train, kw_test,
                        popt_kwargs=popt_kwargs, device="cpu")
    nets = (("fn", rc.network), ("fine", rc.network_fine))
    init = {f"{t}__{k}": p.detach().numpy().copy() for t, net in nets for k, p in net.named_parameters()}
    recorded = {}

    def norms_before(opt_step):  # get_gradnorm of the gradients the step uses (module docstring)
        def step(*a, **k):
            recorded["norms"] = trainer.get_gradnorm(kw_train["ray_caster"])
            return opt_step(*a, **k)
        return step
    optimizer.step = norms_before(optimizer.step)
    for opt in (optimizer, pose_optimizer):
        if opt is not None and cfg["popt"]:
            opt.zero_grad = (lambda z: lambda set_to_none=False: z(set_to_none=False))(opt.zero_grad)
    real_rand, real_randn = torch.rand, torch.randn
    keys = {}

    def fake(kind, queue):
        def fn(*shape, **kw):
            k, arr = queue.pop(0)
            shp = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
            assert k == kind and shp == arr.shape, (kind, shp, k, arr.shape)
            return torch.from_numpy(arr.copy())
        return fn
    for i in range(K):
        nc = n * cfg.get("candidates", 1)
        pose = np.sort(rng.integers(0, P, nc)).astype(np.int64)
        if i == 0:
            pose[0], pose[-1] = 0, P - 1  # (both wraps of the temporal neighbours)
        pix = [rng.integers(len(per_pose[f][0])) for f in pose]
        o = np.stack([per_pose[f][0][p] for f, p in zip(pose, pix)]).astype(np.float32)
        d = np.stack([per_pose[f][1][p] for f, p in zip(pose, pix)]).astype(np.float32)
        cyl = np.stack([per_pose[f][2] for f in pose]).astype(np.float32)
        step = dict(rays_o=o, rays_d=d, pose=pose, cyls=cyl, target=rng.random((nc, 3), dtype=np.float32),
                    bg=rng.random((nc, 3), dtype=np.float32),
                    t_rand=rng.random((nc, S), dtype=np.float32), noise0=rng.standard_normal((nc, S), dtype=np.float32),
                    u=rng.random((nc, I), dtype=np.float32), noise1=rng.standard_normal((nc, S + I), dtype=np.float32))
        if nc > n:
            # keep the first n candidates whose accumulated opacity, at the current weights and with their own draws,
            # stays below max_acc in both passes (rays are rendered independently: the batch reproduces these values)
            queue = [("rand", step["t_rand"]), ("randn", step["noise0"]), ("rand", step["u"]), ("randn", step["noise1"])]
            torch.rand, torch.randn = fake("rand", queue), fake("randn", queue)
            try:
                with torch.no_grad():
                    pre = trainer.render(sc["H"], sc["W"], sc["focal"], chunk=args.chunk, verbose=False, retraw=False,
                                         rays=torch.from_numpy(np.stack([o, d])), kp_batch=torch.from_numpy(sc["kps"][pose]),
                                         skts=torch.from_numpy(sc["skts"][pose]), bones=torch.from_numpy(sc["bones"][pose]),
                                         cyls=torch.from_numpy(cyl), cams=None, subject_idxs=None, **kw_train)
            finally:
                torch.rand, torch.randn = real_rand, real_randn
            ok = np.nonzero((torch.maximum(pre["acc_map"], pre["acc0"]) < cfg["max_acc"]).numpy())[0]
            assert len(ok) >= n, f"only {len(ok)} of {nc} candidate rays below acc {cfg['max_acc']}"
            step = {k: np.ascontiguousarray(v[ok[:n]]) for k, v in step.items()}
            o, d, pose, cyl = step["rays_o"], step["rays_d"], step["pose"], step["cyls"]
        batch = {"rays": torch.from_numpy(np.stack([o, d])), "cyls": torch.from_numpy(cyl),
                 "target_s": torch.from_numpy(step["target"]), "bgs": torch.from_numpy(step["bg"])}
        if cfg["popt"]:
            step["temp_val"] = (rng.random(n) < 0.8).astype(np.float32)
            batch.update(kp_idx=torch.from_numpy(pose), temp_val=torch.from_numpy(step["temp_val"]))
        else:
            step["fgs"] = np.where(rng.random(n) < 0.5, 1.0, rng.random(n)).astype(np.float32)
            batch.update(kp3d=torch.from_numpy(sc["kps"][pose]), skts=torch.from_numpy(sc["skts"][pose]),
                         bones=torch.from_numpy(sc["bones"][pose]), fgs=torch.from_numpy(step["fgs"])[:, None])
        queue = [("rand", step["t_rand"]), ("randn", step["noise0"]), ("rand", step["u"]), ("randn", step["noise1"])]
        torch.rand, torch.randn = fake("rand", queue), fake("randn", queue)
        try:
            loss_dict, stats = T.train_batch(batch, i=i, global_step=GLOBAL_STEP * i)
        finally:
            torch.rand, torch.randn = real_rand, real_randn
        assert not queue, "the reference drew fewer random tensors than expected"
        stats["total_norm"], stats["avg_norm"] = recorded["norms"]
        keys[i] = (sorted(loss_dict), sorted(stats))
        for k, v in step.items():
            data[f"s{i}_{k}"] = v
        for k, v in loss_dict.items():
            data[f"s{i}_loss_{k}"] = np.float64(float(v))
        for k, v in stats.items():
            data[f"s{i}_stat_{k}"] = np.float64(float(v))
        print(f"{name} step {i}: " + " ".join(f"{k}={float(v):.6g}" for k, v in {**loss_dict, **stats}.items()))
    if cfg["popt"]:
        data.update(final_bones6=layer.bones.detach().numpy(), final_pelvis=layer.pelvis.detach().numpy())
    for t, net in nets:
        for k, p in net.named_parameters():
            key = f"{t}__{k}"
            v = p.detach().numpy().reshape(-1)
            idx = sample_idx(v.size)
            data["final_" + key] = v[idx]
            data["update_norm_" + key] = np.float64(np.linalg.norm(v.astype(np.float64) -
                                                                   init[key].reshape(-1).astype(np.float64)))
    meta = dict(seed=cfg["seed"], sha256=mg.anerf_syn.checkpoint_sha256(ck), NJ=NJ, S=S, I=I, D=cfg["D"], W=cfg["W"],
                tau=cfg["tau"], H=sc["H"], focal=sc["focal"], ext_scale=0.001, chunk=4096, framecode=0, flags=cfg.get("model_flags", []),
                drop=[], n_poses=P, K=K, n_rays=n, popt=cfg["popt"], train_flags=cfg["flags"], raw_noise_std=1.0,
                global_step=GLOBAL_STEP, sample=SAMPLE, loss_keys={i: k[0] for i, k in keys.items()},
                stat_keys={i: k[1] for i, k in keys.items()}, torch=torch.__version__)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, meta=np.array(repr(meta)), **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB)")


def main():
    import torch
    torch.set_num_threads(8)
    mods = mg.import_reference()
    only = sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        for name, cfg in CONFIGS.items():
            if only and name not in only:
                continue
            make(name, cfg, mods, tmp)


if __name__ == "__main__":
    main()

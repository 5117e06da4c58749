"""GPU: the training-step kernels (anerf_train_loss, anerf_pose_loss, anerf_adam_step) against the float64 checkers
of a-nerf_amd/trainer.py, and the Trainer over several steps.

Bounds.  The loss kernels compute in double and round once, so every loss is within 1e-6 relative of the float64
checker (the issue's bound for a tree sum of <= 2^13 non-negative fp32 terms; a single rounding is 6e-8), every
gradient within 1e-6 relative + 1e-9, psnr within 1e-4 dB.  The Adam kernel is fp32 in torch's operation order: its
error to the float64 checker is at most twice that of torch.optim.Adam(foreach=True) on the same device and inputs
plus one fp32 ulp of the value per step (both are valid roundings of the same formula; a contracted multiply-add may
differ in the last bit); the norms are double sums, within 1e-6 relative.
"""
import importlib

import numpy as np
import pytest
import torch

from _trainer_cases import loss_inputs, pose_case, pose_reference

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")
T = importlib.import_module("a-nerf_amd.trainer")

REL, ABS_G, PSNR_DB = 1e-6, 1e-9, 1e-4


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev32(x):
    return torch.tensor(np.asarray(x), dtype=torch.float32, device="cuda").contiguous()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def close(got, ref, what, rel=REL, abs_=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if np.isnan(ref).any():
        assert np.array_equal(np.isnan(got), np.isnan(ref)), what
        got, ref = np.nan_to_num(got), np.nan_to_num(ref)
    err = np.abs(got - ref) - (rel * np.abs(ref) + abs_)
    assert err.max() <= 0.0, f"{what}: max |got - ref| = {np.abs(got - ref).max():.3e} at |ref| = " \
                             f"{np.abs(ref).reshape(-1)[err.argmax()]:.3e}"


# ---- the loss kernel

#             loss_fn  beta  coarse bgs        reg    fgs
LOSS_CASES = [("MSE", 0.1, True, "per-ray", None, None),
              ("L1", 0.1, True, "base", None, None),
              ("Huber", 0.125, True, "per-ray", "BCE", "mixed"),
              ("Huber", 0.5, False, "off", None, None),
              ("MSE", 0.1, False, "base", "BCE", "mixed"),
              ("L1", 0.1, False, "off", "BCE", "mixed"),
              ("MSE", 0.1, True, "per-ray", "BCE", "all-foreground")]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2051])
@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_loss_kernel(n, case):
    loss_fn, beta, coarse, bgs, reg, fgs_kind = case
    d = loss_inputs(n, 100 + n, f32=True)
    if fgs_kind == "all-foreground":
        d["fgs"] = np.ones(n)
    elif reg:
        d["fgs"][0] = 0.25  # (at least one ray under the regulariser, also at n = 1)
    kw = dict(loss_fn=loss_fn, loss_beta=beta, use_background=bgs != "off", coarse_weight=0.75, reg_fn=reg,
              reg_coef=0.25)
    spec = T.LossSpec(base_bg=1.0, **kw)
    t = {k: dev32(v) for k, v in d.items()}
    args = dict(rgb0=t["rgb0"] if coarse else None, acc0=t["acc0"] if coarse else None,
                bgs=t["bgs"] if bgs == "per-ray" else None, fgs=t["fgs"] if reg else None)
    ref = {u: T.nerf_loss_reference(d["rgb"], d["acc"], d["target"], d["rgb0"] if coarse else None,
                                    d["acc0"] if coarse else None, bgs=d["bgs"] if bgs == "per-ray" else None,
                                    base_bg=1.0, fgs=d["fgs"] if reg else None, upstream=u, **kw) for u in (1.0, 0.5)}
    out, ws = T.train_loss_forward(spec, t["rgb"], t["acc"], t["target"], **args)
    out2, _ = T.train_loss_forward(spec, t["rgb"], t["acc"], t["target"], **args)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), "two calls, different bits"
    got = dict(zip(T.LOSS_STATS, host(out)))
    print(f"\nloss n={n} {case}: " + " ".join(f"{k}={got[k]:.9g}/{ref[1.0][k]:.9g}" for k in T.LOSS_STATS))
    for k in ("rgb_loss", "rgb_loss0", "reg_loss", "reg_loss0", "alpha", "total"):
        close(got[k], ref[1.0][k], k)
    for k in ("psnr",) + (("psnr0",) if coarse else ()):
        assert abs(got[k] - ref[1.0][k]) <= PSNR_DB, (k, got[k], ref[1.0][k])
    if fgs_kind == "all-foreground":
        assert np.isnan(got["reg_loss"]) and np.isnan(got["reg_loss0"]) and np.isnan(got["total"])
    grads = {}
    for u in (1.0, 0.5):
        up = torch.tensor(u, dtype=torch.float32, device="cuda")
        g = T.train_loss_backward(spec, ws, up, t["rgb"], t["acc"], t["target"], **args)
        grads[u] = g
        for name, gt in zip(("g_rgb", "g_acc", "g_rgb0", "g_acc0"), g):
            if gt is None:
                assert name.endswith("0") and not coarse
                continue
            close(host(gt), ref[u][name], f"{name} upstream {u}", REL, ABS_G)
    g_again = T.train_loss_backward(spec, ws, torch.tensor(1.0, device="cuda"), t["rgb"], t["acc"], t["target"], **args)
    for a, b, h in zip(grads[1.0], g_again, grads[0.5]):
        if a is not None:
            assert torch.equal(a, b), "two backward calls, different bits"
            assert torch.equal(a * 0.5, h), "upstream 0.5 does not halve the gradient exactly"


def test_step_loss_is_one_autograd_node():
    """step_loss: total_loss.backward() reaches the render outputs and the pose tensors through one node, with the
    upstream gradient of a scaled loss."""
    n, nj = 65, 24
    d = loss_inputs(n, 7, f32=True)
    c = pose_case(n, nj, True, True, 8, f32=True)
    t = {k: dev32(v).requires_grad_(k in ("rgb", "acc", "rgb0", "acc0")) for k, v in d.items()}
    prev, nxt = T.temporal_neighbours(c["kp_idx"], c["N"])
    cur, kps = dev32(c["cur"]).requires_grad_(True), dev32(c["kps"]).requires_grad_(True)
    pose = T.PoseSpec(dev32(T._cur6(c["anchor_full"], True)), dev32(c["anchor_kps"]),
                      torch.tensor(c["kp_idx"], device="cuda"), True, c["tol"], c["coef"],
                      dev32(c["frames_cur"][prev]), dev32(c["frames_cur"][nxt]), dev32(c["frames_kps"][prev]),
                      dev32(c["frames_kps"][nxt]), dev32(c["temp_val"]), c["temp_coef"], c["ext_scale"])
    spec = T.LossSpec("MSE", use_background=True, coarse_weight=1.0)
    total, stats = T.step_loss(spec, t["rgb"], t["acc"], t["target"], t["rgb0"], t["acc0"], t["bgs"], None, pose, cur,
                               kps)
    assert total.grad_fn is not None and type(total.grad_fn).__name__.startswith("_StepLoss")
    (total * 0.5).backward()
    rl = T.nerf_loss_reference(d["rgb"], d["acc"], d["target"], d["rgb0"], d["acc0"], bgs=d["bgs"], use_background=True,
                               upstream=0.5)
    rp = pose_reference(c, upstream=0.5)
    close(total.item(), rl["total"] + rp["total"], "total", 2e-6)
    s = host(stats)
    close(s[len(T.LOSS_STATS) + 2], rp["MPJPC"], "MPJPC")
    for k in ("rgb", "acc", "rgb0", "acc0"):
        close(host(t[k].grad), rl["g_" + k], k, REL, ABS_G)
    close(host(cur.grad), rp["g_cur"], "g_cur", REL, ABS_G)
    close(host(kps.grad), rp["g_kps"], "g_kps", REL, ABS_G)


# ---- the pose-loss kernel

@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("nj", [2, 24, 65])
@pytest.mark.parametrize("rot6d", [True, False], ids=["rot6d", "axisangle"])
@pytest.mark.parametrize("temporal", [True, False], ids=["temporal", "anchor-only"])
def test_pose_loss_kernel(n, nj, rot6d, temporal):
    c = pose_case(n, nj, rot6d, temporal, 200 + n + nj, f32=True)
    if n >= 2:
        assert 0 in c["kp_idx"] and c["N"] - 1 in c["kp_idx"]  # (both wraps of the neighbours)
    d2 = ((c["anchor_full"][c["kp_idx"]] - c["cur"])[:, 1:, ..., :2 if rot6d else 3]) ** 2
    assert (d2 > c["tol"]).any() and (d2 <= c["tol"]).any(), "the tolerance must cut through the case"
    prev, nxt = T.temporal_neighbours(c["kp_idx"], c["N"])
    tk = {}
    if temporal:
        tk = dict(prev_cur=dev32(c["frames_cur"][prev]), next_cur=dev32(c["frames_cur"][nxt]),
                  prev_kps=dev32(c["frames_kps"][prev]), next_kps=dev32(c["frames_kps"][nxt]),
                  temp_val=dev32(c["temp_val"]), temp_coef=c["temp_coef"])
    spec = T.PoseSpec(dev32(T._cur6(c["anchor_full"], rot6d)), dev32(c["anchor_kps"]),
                      torch.tensor(c["kp_idx"], device="cuda"), rot6d, c["tol"], c["coef"], ext_scale=c["ext_scale"],
                      **tk)
    cur, kps = dev32(c["cur"]), dev32(c["kps"])
    out, out2 = T.pose_loss_forward(spec, cur, kps), T.pose_loss_forward(spec, cur, kps)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), "two calls, different bits"
    got = dict(zip(T.POSE_STATS, host(out)))
    ref = {u: pose_reference(c, upstream=u) for u in (1.0, 0.5)}
    print(f"\npose n={n} nj={nj} rot6d={rot6d} temporal={temporal}: " +
          " ".join(f"{k}={got[k]:.9g}/{ref[1.0][k]:.9g}" for k in T.POSE_STATS))
    for k in T.POSE_STATS:
        close(got[k], ref[1.0][k], k)
    assert (got["temp_loss"] > 0) == temporal
    g = {}
    for u in (1.0, 0.5):
        g[u] = T.pose_loss_backward(spec, torch.tensor(u, device="cuda"), cur, kps)
        close(host(g[u][0]), ref[u]["g_cur"], f"g_cur upstream {u}", REL, ABS_G)
        if temporal:
            close(host(g[u][1]), ref[u]["g_kps"], f"g_kps upstream {u}", REL, ABS_G)
        else:
            assert g[u][1] is None
    if rot6d:
        assert torch.count_nonzero(g[1.0][0][..., 2]).item() == 0, "the third column of g_rots must be exactly 0"
    assert torch.count_nonzero(g[1.0][0]).item() > 0
    assert torch.equal(g[1.0][0] * 0.5, g[0.5][0])


def test_pose_loss_index_outside_the_table_reads_nothing():
    c = pose_case(3, 4, True, False, 5, f32=True)
    idx = torch.tensor([0, 7, -1], device="cuda")
    spec = T.PoseSpec(dev32(T._cur6(c["anchor_full"], True)), dev32(c["anchor_kps"]), idx, True, c["tol"], c["coef"])
    out = host(T.pose_loss_forward(spec, dev32(c["cur"]), dev32(c["kps"])))
    assert np.isnan(out[0]) and np.isnan(out[2])


# ---- the Adam kernel

def _adam_case(sizes, view_at=None, skip_at=None, steps=5, wd=0.0, seed=0):
    """`steps` updates of tensors of `sizes` elements by anerf.Adam, torch.optim.Adam(foreach=True) and the float64
    checker on the same seeded gradients, the learning rate changed between steps; gradient `view_at` is a view one
    element into a larger buffer (4-byte aligned only), parameter `skip_at` never has a gradient."""
    rs = np.random.RandomState(seed)
    betas, eps = (0.9, 0.99), 1e-8
    init = [rs.normal(size=s).astype(np.float32) for s in sizes]
    ours = [torch.nn.Parameter(torch.tensor(x, device="cuda")) for x in init]
    theirs = [torch.nn.Parameter(torch.tensor(x, device="cuda")) for x in init]
    opt = anerf.Adam(ours, lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
    topt = torch.optim.Adam(theirs, lr=1e-3, betas=betas, eps=eps, weight_decay=wd, foreach=True)
    ref = [(x.astype(np.float64), np.zeros(s), np.zeros(s)) for x, s in zip(init, sizes)]
    worst = {"ours": 0.0, "torch": 0.0}
    for step in range(1, steps + 1):
        lr = 1e-3 * 0.7 ** (step - 1)
        for o in (opt, topt):
            for g in o.param_groups:
                g["lr"] = lr
        grads = [rs.normal(scale=10.0 ** rs.uniform(-3, 0), size=s).astype(np.float32) for s in sizes]
        sq, cnt = 0.0, 0
        for k, g in enumerate(grads):
            if k == skip_at:
                ours[k].grad = theirs[k].grad = None
                continue
            if k == view_at:
                buf = torch.zeros(sizes[k] + 1, device="cuda")
                buf[1:] = torch.tensor(g, device="cuda")
                ours[k].grad = buf[1:]
                assert ours[k].grad.data_ptr() % 16 == 4
            else:
                ours[k].grad = torch.tensor(g, device="cuda")
            theirs[k].grad = torch.tensor(g, device="cuda")
            ref[k] = T.adam_reference(*ref[k][:1], g, *ref[k][1:], step, lr, betas, eps, wd)
            sq += float((g.astype(np.float64) ** 2).sum())
            cnt += 1
        opt.step()
        topt.step()
        norms = host(opt.last_grad_norm())
        close(norms[0], np.sqrt(sq), "total_norm")
        close(norms[1], np.sqrt(sq / cnt), "avg_norm")
        for k in range(len(sizes)):
            if k == skip_at:
                continue
            assert float(opt.state[ours[k]]["step"]) == float(topt.state[theirs[k]]["step"]) == step
            for name, r, a, b in (("param", ref[k][0], ours[k], theirs[k]),
                                  ("exp_avg", ref[k][1], opt.state[ours[k]]["exp_avg"], topt.state[theirs[k]]["exp_avg"]),
                                  ("exp_avg_sq", ref[k][2], opt.state[ours[k]]["exp_avg_sq"],
                                   topt.state[theirs[k]]["exp_avg_sq"])):
                e_ours, e_torch = np.abs(host(a) - r), np.abs(host(b) - r)
                ulp = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
                if name == "param":
                    worst["ours"], worst["torch"] = max(worst["ours"], e_ours.max()), max(worst["torch"], e_torch.max())
                assert (e_ours <= 2.0 * e_torch.max() + step * ulp).all(), \
                    f"{name} of tensor {k} ({sizes[k]}) at step {step}: {e_ours.max():.3e} vs torch {e_torch.max():.3e}"
    return ours, theirs, opt, topt, init, worst


def test_adam_kernel_sizes_view_and_skipped_tensor():
    sizes = [1, 3, 255, 256, 257, 65537, 2048, 5]
    ours, theirs, opt, topt, init, worst = _adam_case(sizes, view_at=4, skip_at=7)
    print(f"\nadam max |param - float64| after 5 steps: kernel {worst['ours']:.3e}, torch foreach {worst['torch']:.3e}")
    assert torch.equal(ours[7].detach().cpu(), torch.tensor(init[7])), "the skipped parameter moved"
    assert ours[7] not in opt.state and theirs[7] not in topt.state  # (no state for it, as in torch)
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and 7 not in sd["state"]


@pytest.mark.parametrize("count", [1, 70])
def test_adam_kernel_table_sizes(count):
    """One tensor, and 70: more than the 64 a launch's table holds."""
    sizes = [257] if count == 1 else [(1, 3, 255, 256, 257, 2049, 4097)[k % 7] for k in range(count)]
    _, _, _, _, _, worst = _adam_case(sizes, view_at=count // 2, seed=count)
    print(f"\nadam x{count}: kernel {worst['ours']:.3e}, torch foreach {worst['torch']:.3e}")


def test_adam_kernel_weight_decay_and_hook():
    calls = []
    ours, theirs, opt, topt, init, worst = _adam_case([300, 7], wd=0.01, seed=3)
    opt.on_step = lambda: calls.append(1)
    v = ours[0]._version
    ours[0].grad = torch.ones_like(ours[0])
    opt.step()
    assert calls == [1]
    assert ours[0]._version == v  # (why the hook exists: the kernel does not advance the version counter)


def test_adam_two_runs_give_the_same_bits():
    a = _adam_case([65537, 257, 3], view_at=1, seed=9)[0]
    b = _adam_case([65537, 257, 3], view_at=1, seed=9)[0]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_grad_norms_on_the_device():
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in (5, 300, 7)]
    ps[0].grad, ps[1].grad = torch.randn(5, device="cuda"), torch.randn(300, device="cuda")
    got = host(T.grad_norms(ps))
    sq = sum(float((host(p.grad) ** 2).sum()) for p in ps[:2])
    close(got, [np.sqrt(sq), np.sqrt(sq / 2)], "grad_norms", 1e-6)


# ---- the Trainer over several steps, against the reference's own Trainer.train_batch (tests/golden/tr*.npz)

import argparse  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402

from _golden import Golden  # noqa: E402
from _trainer_cases import torch_kp_loss  # noqa: E402

train = importlib.import_module("a-nerf_amd.train")
kin = importlib.import_module("a-nerf_amd.kinematics")
raycaster = importlib.import_module("a-nerf_amd.raycaster")

GRAD_REL = 2e-3  # tests/test_gpu_train.py: the training gradients' bound; here the sanity bound of the fixtures' losses
DEFAULTS = dict(loss_fn="MSE", loss_beta=0.1, use_background=False, reg_fn=None, reg_coef=0.1, coarse_weight=1.0,
                opt_pose=False, opt_rot6d=False, use_temp_loss=False, temp_coef=0.05, opt_pose_step=1,
                opt_pose_stop=None, opt_pose_tol=0.0, opt_pose_coef=0.0, opt_pose_lrate=5e-4, opt_pose_cache=False,
                lrate=5e-4, lrate_decay=250, lrate_decay_rate=0.1, decay_unit=1000, cutoff_step=250, cutoff_rate=10.0,
                finetune=False, opt_framecode=False, chunk=4096, ext_scale=0.001, multires=7, freq_schedule_step=5)
INTS = ("opt_pose_step", "opt_pose_stop", "lrate_decay", "decay_unit", "cutoff_step")


def _args(flags):
    a = dict(DEFAULTS)
    k = 0
    while k < len(flags):
        name = flags[k][2:]
        if isinstance(DEFAULTS[name], bool):
            a[name] = True
            k += 1
        else:
            v = flags[k + 1]
            a[name] = int(v) if name in INTS else (v if name in ("loss_fn", "reg_fn") else float(v))
            k += 2
    return argparse.Namespace(**a)


class _Run:
    """One fixture's model, pose layer, optimizers and batches; kind 'A' = the parent's composition (train.nerf_loss,
    the torch pose-loss expression, torch.optim.Adam), 'B' = the Trainer on anerf.Adam."""

    def __init__(self, name, mlp, kind, popt=None):
        g = self.g = Golden(name)
        m, dev = g.meta, torch.device("cuda:0")
        self.args, self.kind, self.dev = _args(m["train_flags"]), kind, dev
        self.popt = m["popt"] if popt is None else popt  # (False: the batch carries the scene's poses, no pose layer)
        if not self.popt:
            self.args.opt_pose = self.args.use_temp_loss = False
        caster = self.caster = train.TrainRayCaster(g.cfg, g.ckpt, mlp=mlp).train()
        common = {"N_importance": m["I"], "N_samples": m["S"], "use_viewdirs": True, "ext_scale": m["ext_scale"],
                  "preproc_kwargs": {"density_scale": 1.0}, "lindisp": False, "nerf_type": "nerf"}
        self.kw_train = {"ray_caster": caster, "perturb": 1.0, "raw_noise_std": 1.0, "ray_noise_std": 0.0, **common}
        self.kw_test = {"ray_caster": raycaster._EvalView(caster), "perturb": False, "raw_noise_std": 0.0,
                        "ray_noise_std": 0.0, **common}
        self.layer = self.popt_kwargs = self.pose_opt = None
        Adam = anerf.Adam if kind == "B" else torch.optim.Adam
        if self.popt:
            layer = self.layer = kin.PoseOptLayer(g["scene_kps"], g["scene_bones"], g["rest"], use_rot6d=True, device=dev)
            with torch.no_grad():
                layer.bones.copy_(torch.from_numpy(g["init_bones6"]))
                layer.pelvis.copy_(torch.from_numpy(g["init_pelvis"]))
            self.anchors = {"kps": torch.from_numpy(g["anchor_kps"]).to(dev),
                            "rots": torch.from_numpy(g["anchor_rots"]).to(dev),
                            "bones": torch.from_numpy(g["scene_bones"]).to(dev), "beta": torch.zeros(1, 10)}
            self.popt_kwargs = {"popt_layer": layer, "popt_anchors": self.anchors}
            self.pose_opt = Adam(list(layer.parameters()), lr=self.args.opt_pose_lrate, betas=(0.9, 0.999))
        self.opt = Adam([p for p in caster.parameters() if p.requires_grad], lr=self.args.lrate, betas=(0.9, 0.999))
        self.hwf = (m["H"], m["H"], m["focal"])
        self.trainer = anerf.Trainer(self.args, {"hwf": self.hwf}, self.opt, self.pose_opt, self.kw_train, self.kw_test,
                                     popt_kwargs=self.popt_kwargs) if kind == "B" else None
        self.init = {k: p.detach().clone() for k, p in self.named()}

    def named(self):
        for t, net in (("fn", self.caster.network_fn), ("fine", self.caster.network_fine)):
            for k, p in net.named_parameters():
                yield f"{t}__{k}", p

    def batch(self, i):
        g, c = self.g, (lambda k: torch.from_numpy(self.g[f"s{i}_{k}"]))
        b = {"rays": torch.stack([c("rays_o"), c("rays_d")]), "cyls": c("cyls"), "target_s": c("target"), "bgs": c("bg")}
        if self.popt:
            b.update(kp_idx=c("pose"), temp_val=c("temp_val"))
        else:
            pose = g[f"s{i}_pose"]
            sc = self.scene()
            b.update(kp3d=torch.from_numpy(sc["kps"][pose]), skts=torch.from_numpy(sc["skts"][pose]),
                     bones=torch.from_numpy(sc["bones"][pose]))
            if g.has(f"s{i}_fgs"):
                b["fgs"] = c("fgs")[:, None]
        rand = {k: c(k).to(self.dev) for k in ("t_rand", "noise0", "u", "noise1")}
        return b, rand

    def scene(self):
        if not hasattr(self, "_scene"):
            m = self.g.meta
            syn = importlib.import_module("a-nerf_amd.synthetic")
            self._scene = syn.make_scene(n_joints=m["NJ"], H=m["H"], W=m["H"], seed=m["seed"], n_frames=m["n_poses"],
                                         yaw_step=0.5)
        return self._scene

    def step(self, i):
        batch, rand = self.batch(i)
        gs = self.g.meta["global_step"] * i
        if self.kind == "B":
            loss_dict, stats = self.trainer.train_batch(batch, i=i, global_step=gs, rand=rand)
            return {k: float(v) for k, v in loss_dict.items()}, stats
        return self.step_a(batch, rand, i, gs)

    def step_a(self, batch, rand, i, gs):
        """The parent's composition of one step (tools/train_bench.py:160-181, all flag combinations)."""
        a, dev = self.args, self.dev
        batch = {k: v.to(dev) for k, v in batch.items()}
        detach = not (a.opt_pose_stop is None or i < a.opt_pose_stop)
        if self.layer is not None:
            kps, bones, skts, _, rots = self.layer(batch["kp_idx"])
            if detach:
                kps, bones, skts, rots = (t.detach() for t in (kps, bones, skts, rots))
        else:
            kps, bones, skts, rots = batch["kp3d"], batch["bones"], batch["skts"], None
        out = anerf.render(*self.hwf, chunk=a.chunk, rays=batch["rays"], kp_batch=kps, skts=skts, bones=bones,
                           cyls=batch["cyls"], rand=rand, **self.kw_train)
        total, loss_dict = train.nerf_loss(out, batch["target_s"], bgs=batch["bgs"], use_background=a.use_background,
                                           coarse_weight=a.coarse_weight, loss_fn=a.loss_fn, loss_beta=a.loss_beta,
                                           reg_fn=a.reg_fn, reg_coef=a.reg_coef, fgs=batch.get("fgs"), return_dict=True)
        stats = {}
        with torch.no_grad():
            for tag, r, ac in (("", out["rgb_map"], out["acc_map"]), ("0", out["rgb0"], out["acc0"])):
                pred = r + (1.0 - ac)[..., None] * batch["bgs"] if a.use_background else r
                stats["psnr" + tag] = float(-10.0 * torch.log(((pred - batch["target_s"]) ** 2).mean()) / np.log(10.0))
        no_pose = detach or not a.opt_pose
        if not no_pose:
            N = self.layer.N_kps
            pose = torch_kp_loss(a, self.anchors, batch["kp_idx"], {"kp_batch": kps, "rots": rots, "bones": bones},
                                 lambda idx: [self.layer(torch.remainder(idx, N))[k] for k in (0, 1, 4)],
                                 batch.get("temp_val"))
            stats["MPJPC"] = float(pose.pop("MPJPC"))
            for k, v in pose.items():
                total = total + v
                loss_dict[k] = v
        loss_dict["total_loss"] = total
        total.backward()
        sq = [float(p.grad.norm(2)) ** 2 for p in self.caster.parameters() if p.grad is not None]
        stats["total_norm"], stats["avg_norm"] = sum(sq) ** 0.5, (sum(sq) / len(sq)) ** 0.5
        self.opt.step()
        self.opt.zero_grad()
        if not no_pose and i % a.opt_pose_step == 0:
            self.pose_opt.step()
            self.pose_opt.zero_grad()
        lr, _ = T.decay_optimizer_lrate(a.lrate, a.lrate_decay, a.lrate_decay_rate, self.opt, decay_unit=a.decay_unit)
        self.caster.update_embed_fns(gs, a)
        stats.update(lrate=lr, alpha=float(out["acc_map"].detach().mean()), cutoff=self.caster.embed_fn.get_tau())
        return {k: float(v) for k, v in loss_dict.items()}, stats


def _trajectory(name, mlp, kind):
    run = _Run(name, mlp, kind)
    g, K = run.g, run.g.meta["K"]
    steps, poses = [], []
    for i in range(K):
        steps.append(run.step(i))
        if run.layer is not None:
            poses.append((run.layer.bones.detach().clone(), run.layer.pelvis.detach().clone()))
    dev = {}
    for i, (loss_dict, stats) in enumerate(steps):
        for tag, d in (("loss", loss_dict), ("stat", stats)):
            for k, v in d.items():
                dev[f"s{i}_{tag}_{k}"] = (abs(v - float(g[f"s{i}_{tag}_{k}"])), abs(float(g[f"s{i}_{tag}_{k}"])))
    if run.layer is not None:
        for k, t in (("final_bones6", run.layer.bones), ("final_pelvis", run.layer.pelvis)):
            dev[k] = (float(np.abs(host(t) - g[k]).max()), float(np.abs(g[k]).max()))
    idx_of = lambda n: np.arange(0, n, max(1, n // g.meta["sample"]))[:g.meta["sample"]]  # noqa: E731
    for k, p in run.named():
        idx = idx_of(p.numel())
        p0 = host(run.init[k]).reshape(-1)[idx]
        upd, upd_ref = host(p).reshape(-1)[idx] - p0, g["final_" + k].astype(np.float64) - p0
        dev["update_" + k] = (float(np.linalg.norm(upd - upd_ref) / np.linalg.norm(upd_ref)), 1.0)
    return run, steps, poses, dev


_CACHE = {}


def trajectory(name, mlp, kind):
    if (name, mlp, kind) not in _CACHE:
        _CACHE[(name, mlp, kind)] = _trajectory(name, mlp, kind)
    return _CACHE[(name, mlp, kind)]


FIXTURES = ["tr1_popt_d4w128", "tr2_nopopt_d8w256"]


@pytest.mark.parametrize("mlp", ["fp32", "bf16x6", "mixed"])
@pytest.mark.parametrize("name", FIXTURES)
def test_trainer_trajectory_against_the_reference(name, mlp):
    """Every step's loss_dict / stats, the final poses and every network tensor's update: the Trainer's deviation from
    the reference's Trainer.train_batch is at most twice that of the parent's composition of the same step (+ 1e-6 of
    the reference value); both are printed and kept in profiles/trainer_parity.json."""
    run_a, steps_a, _, dev_a = trajectory(name, mlp, "A")
    run_b, steps_b, _, dev_b = trajectory(name, mlp, "B")
    g = run_b.g
    report = {k: {"A": dev_a[k][0], "B": dev_b[k][0], "ref": dev_a[k][1]} for k in dev_a}
    print(f"\n{name} {mlp}: deviation from the reference, parent's composition (A) | Trainer (B)")
    for k, r in report.items():
        print(f"  {k:44s} A {r['A']:.3e}  B {r['B']:.3e}  |ref| {r['ref']:.3e}")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trainer_parity.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[f"{name}-{mlp}"] = report
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass  # (a read-only checkout: the figures are in the output above)
    for i, (loss_dict, stats) in enumerate(steps_b):  # exact keys and values
        assert sorted(loss_dict) == g.meta["loss_keys"][i] and sorted(stats) == g.meta["stat_keys"][i], i
        assert stats["lrate"] == float(g[f"s{i}_stat_lrate"]) and stats["cutoff"] == float(g[f"s{i}_stat_cutoff"]), i
    assert dev_a.keys() == dev_b.keys()
    if mlp in ("fp32", "bf16x6"):
        ref0 = float(g["s0_loss_total_loss"])
        assert abs(steps_b[0][0]["total_loss"] - ref0) <= 1e-5 * abs(ref0), (steps_b[0][0]["total_loss"], ref0)
        for dev in (dev_a, dev_b):  # the sanity condition: otherwise the fixture is wrong
            for k, (d, ref) in dev.items():
                if "_loss_" in k:
                    assert d <= GRAD_REL * ref, (k, d, ref)
    bad = {k: report[k] for k in report if report[k]["B"] > 2.0 * report[k]["A"] + 1e-6 * report[k]["ref"]}
    assert not bad, bad


def test_trainer_pose_schedule():
    """opt_pose_step 2: the pose parameters are bit-unchanged after steps 1, 3 and 5; from opt_pose_stop (4) on they
    are bit-unchanged and the loss has no kp_loss."""
    run, steps, poses, _ = trajectory("tr1_popt_d4w128", "fp32", "B")
    init = (torch.from_numpy(run.g["init_bones6"]).cuda(), torch.from_numpy(run.g["init_pelvis"]).cuda())
    before = [init] + poses[:-1]
    for i, (now, prev) in enumerate(zip(poses, before)):
        same = torch.equal(now[0], prev[0]) and torch.equal(now[1], prev[1])
        assert same == (i in (1, 3, 4, 5)), i
    for i, (loss_dict, stats) in enumerate(steps):
        assert ("kp_loss" in loss_dict) == (i < 4) and ("temp_loss" in loss_dict) == (i < 4), i
        assert ("MPJPC" in stats) == (i < 4)


def _eval_render(caster_like, run, i=0):
    g = run.g
    c = lambda k: torch.from_numpy(g[f"s{i}_{k}"]).cuda()  # noqa: E731
    o, d = c("rays_o"), c("rays_d")
    n = o.shape[0]
    rb = torch.cat([o, d, torch.zeros(n, 1).cuda(), torch.ones(n, 1).cuda(), d / d.norm(dim=-1, keepdim=True)], -1)
    sc = run.scene()
    pose = g[f"s{i}_pose"]
    return caster_like.render_rays(rb.contiguous(), g.meta["S"], skts=torch.from_numpy(sc["skts"][pose]).cuda(),
                                   cyls=c("cyls"), N_importance=g.meta["I"])


def test_eval_render_after_train_batch_sees_the_new_weights():
    """The Adam kernel does not advance the version counters; its on_step hook reaches weights_changed, so the eval
    render through render_kwargs_test equals a fresh RayCaster built from checkpoint()."""
    run, steps, _, _ = trajectory("tr1_popt_d4w128", "fp32", "B")
    assert run.opt.on_step is not None
    a = _eval_render(run.kw_test["ray_caster"], run)
    batch, rand = run.batch(0)
    run.trainer.train_batch(batch, i=6, global_step=600, rand=rand)
    b = _eval_render(run.kw_test["ray_caster"], run)
    fresh = anerf.RayCaster(run.g.cfg, run.caster.checkpoint(), device=0)
    c = _eval_render(fresh, run)
    assert not torch.equal(a["rgb_map"], b["rgb_map"]), "the eval caster still renders the old weights"
    for k in ("rgb_map", "acc_map", "disp_map"):
        assert torch.equal(b[k], c[k]), k


def test_save_nerf_and_resume(tmp_path):
    """save_nerf writes the reference's keys; a Trainer rebuilt from that file through create_raycaster continues
    with bit-identical next-step losses (create_raycaster's caster trains in the default "mixed" arithmetic)."""
    run = _Run("tr1_popt_d4w128", "mixed", "B", popt=False)
    for i in range(3):
        batch, rand = run.batch(i)
        run.trainer.train_batch(batch, i=i, global_step=100 * i, rand=rand)
    path = str(tmp_path / "000003.tar")
    run.trainer.save_nerf(path, 3)
    ck = raycaster.load_checkpoint(path)
    assert set(ck) == {"global_step", "optimizer_state_dict", "poseopt_layer_state_dict", "pose_optimizer_state_dict",
                       "poseopt_anchors", "network_fn_state_dict", "network_fine_state_dict", "embed_state_dict",
                       "embedbones_state_dict", "embeddirs_state_dict"}
    assert ck["global_step"] == 3 and set(ck["optimizer_state_dict"]) == {"state", "param_groups"}
    assert ck["poseopt_layer_state_dict"] is None and ck["poseopt_anchors"] is None
    m = run.g.meta
    a = argparse.Namespace(**vars(run.args), N_samples=m["S"], N_importance=m["I"], netdepth=m["D"], netwidth=m["W"],
                           multires_views=4, use_cutoff=True, cutoff_viewdir=True, cutoff_inputs=True,
                           use_viewdirs=True, perturb=1.0, raw_noise_std=1.0, basedir=str(tmp_path), expname="x")
    kw_train, kw_test, start, _, opt, _ = anerf.create_raycaster(a, {"skel_type": kin.SMPLSkeleton}, ckpt=ck)
    assert float(opt.state[opt.param_groups[0]["params"][0]]["step"]) == 3.0
    kw_train["ray_caster"].train()
    again = anerf.Trainer(a, {"hwf": run.hwf}, anerf.Adam.from_torch(opt), None, kw_train, kw_test)
    batch, rand = run.batch(1)
    l1, s1 = run.trainer.train_batch(batch, i=3, global_step=300, rand=rand)
    l2, s2 = again.train_batch(batch, i=3, global_step=300, rand=rand)
    assert l1.keys() == l2.keys()
    for k in l1:
        assert float(l1[k]) == float(l2[k]), k
    assert s1["psnr"] == s2["psnr"] and s1["alpha"] == s2["alpha"] and s1["lrate"] == s2["lrate"]


def test_create_popt_anchors_are_the_initial_poses():
    g = Golden("tr1_popt_d4w128")
    a = _args(g.meta["train_flags"])
    attrs = {"skel_type": kin.SMPLSkeleton, "rest_pose": g["rest"], "betas": np.zeros((1, 10), np.float32),
             "kp3d": g["scene_kps"], "bones": g["scene_bones"]}
    opt, kw = anerf.create_popt(a, attrs, device="cuda:0")
    assert isinstance(opt, anerf.Adam) and set(kw) == {"popt_anchors", "popt_layer", "skel_type"}
    assert set(kw["popt_anchors"]) == {"kps", "bones", "rots", "beta"}
    with torch.no_grad():
        kps, _, _, _, rots = kw["popt_layer"].calculate_kinematic(np.arange(g.meta["n_poses"]))
    close(host(kw["popt_anchors"]["rots"]), host(rots), "anchor rots", 0.0, 1e-6)
    close(host(kw["popt_anchors"]["kps"]), host(kps), "anchor kps", 0.0, 1e-5)
    close(host(rots), g["anchor_rots"], "the reference's anchors", 0.0, 1e-5)


def test_save_nerf_and_resume_with_the_pose_layer(tmp_path):
    """save_nerf with pose optimisation on, then create_raycaster + create_popt from that file: the layer, its
    optimizer and the anchors reload, and the rebuilt Trainer continues below opt_pose_stop with bit-identical losses
    (kp_loss and temp_loss among them) and, after the next pose step, bit-identical pose parameters."""
    run = _Run("tr1_popt_d4w128", "mixed", "B")
    g, m = run.g, run.g.meta
    run.step(0)  # (a pose step: no pose gradient is pending when the file is written)
    path = str(tmp_path / "000001.tar")
    run.trainer.save_nerf(path, 1)
    run.trainer.save_popt(str(tmp_path / "pose_000001.tar"), 1)
    ck = raycaster.load_checkpoint(path)
    assert set(ck["poseopt_layer_state_dict"]) >= {"pelvis", "bones", "rest_pose"}
    assert set(ck["pose_optimizer_state_dict"]) == {"state", "param_groups"}
    assert set(ck["poseopt_anchors"]) == {"kps", "rots", "bones", "beta"}
    assert set(raycaster.load_checkpoint(str(tmp_path / "pose_000001.tar"))) == {"global_step", "poseopt_layer_state_dict",
                                                                                "poseopt_anchors"}
    a = argparse.Namespace(**vars(run.args), N_samples=m["S"], N_importance=m["I"], netdepth=m["D"], netwidth=m["W"],
                           multires_views=4, use_cutoff=True, cutoff_viewdir=True, cutoff_inputs=True,
                           use_viewdirs=True, perturb=1.0, raw_noise_std=1.0, basedir=str(tmp_path), expname="x")
    attrs = {"skel_type": kin.SMPLSkeleton, "rest_pose": g["rest"], "betas": np.zeros((1, 10), np.float32),
             "kp3d": g["scene_kps"], "bones": g["scene_bones"], "hwf": run.hwf}
    kw_train, kw_test, _, _, opt, _ = anerf.create_raycaster(a, attrs, ckpt=ck)
    pose_opt, popt_kwargs = anerf.create_popt(a, attrs, ckpt=ck, device="cuda:0")
    layer = popt_kwargs["popt_layer"]
    assert torch.equal(layer.bones, run.layer.bones) and torch.equal(layer.pelvis, run.layer.pelvis)
    assert not torch.equal(layer.bones.cpu(), torch.from_numpy(g["init_bones6"]))  # (the reloaded, not the initial poses)
    assert torch.equal(popt_kwargs["popt_anchors"]["rots"], run.anchors["rots"].cpu())
    assert float(pose_opt.state[layer.bones]["step"]) == 1.0
    kw_train["ray_caster"].train()
    again = anerf.Trainer(a, attrs, anerf.Adam.from_torch(opt), pose_opt, kw_train, kw_test, popt_kwargs=popt_kwargs)
    for i in (1, 2):
        batch, rand = run.batch(i)
        l1, s1 = run.trainer.train_batch(batch, i=i, global_step=100 * i, rand=rand)
        l2, s2 = again.train_batch(batch, i=i, global_step=100 * i, rand=rand)
        assert set(l1) == set(l2) >= {"kp_loss", "temp_loss", "rgb_loss", "rgb_loss0", "total_loss"}
        for k in l1:
            assert float(l1[k]) == float(l2[k]), (i, k, float(l1[k]), float(l2[k]))
        assert s1 == s2, (i, s1, s2)
        moved = not torch.equal(layer.bones.cpu(), ck["poseopt_layer_state_dict"]["bones"])
        assert moved == (i == 2)  # (opt_pose_step 2: the pose step of iteration 2 uses both iterations' gradients)
        assert torch.equal(layer.bones, run.layer.bones) and torch.equal(layer.pelvis, run.layer.pelvis), i


def test_train_batch_reads_the_device_once():
    """One synchronising device-to-host read per train_batch (the statistics buffer), counted by torch's
    synchronisation debug mode on a warmed-up Trainer with the batch already on the device."""
    import warnings
    run = _Run("tr1_popt_d4w128", "mixed", "B")
    run.step(0)
    batch, rand = run.batch(1)
    batch = {k: v.cuda() for k, v in batch.items()}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            run.trainer.train_batch(batch, i=1, global_step=100, rand=rand)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]
    print("\nsynchronising calls in train_batch:", len(syncs), syncs)
    assert len(syncs) == 1, syncs

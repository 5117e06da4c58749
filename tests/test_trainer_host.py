"""CPU: the training-step entries' argument validation, the float64 checkers of a-nerf_amd/trainer.py against torch,
anerf.Adam's CPU path and state_dict, the refusals, and the trainer fixtures' meta."""
import argparse
import copy
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

anerf = importlib.import_module("a-nerf_amd")
_lib = importlib.import_module("a-nerf_amd._lib")
T = importlib.import_module("a-nerf_amd.trainer")
train = importlib.import_module("a-nerf_amd.train")
from _trainer_cases import loss_inputs, pose_case, pose_reference, torch_kp_loss  # noqa: E402

P = 0x1000  # a non-NULL stand-in pointer: every check below returns before anything is read or launched


# ---- argument validation (before any HIP call)

def _loss_call(lib, **kw):
    a = dict(rgb=P, acc=P, rgb0=None, acc0=None, target=P, bgs=None, base_bg=1.0, fgs=None, n=4, kind=0, beta=0.1,
             use_bg=1, cw=1.0, reg=0, reg_coef=0.1, out=P, ws=P, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.anerf_train_loss(*a.values())


def test_train_loss_rejects_bad_arguments():
    lib = _lib.load()
    for kw, word in ((dict(rgb=None), b"NULL"), (dict(target=None), b"NULL"), (dict(out=None), b"NULL"),
                     (dict(ws=None), b"NULL"), (dict(n=0), b"n must"), (dict(kind=3), b"loss kind"),
                     (dict(kind=-1), b"loss kind"), (dict(reg=2), b"regulariser"), (dict(reg=1), b"fgs"),
                     (dict(rgb0=P), b"rgb0"), (dict(kind=2, beta=-1.0), b"beta")):
        assert _loss_call(lib, **kw) == -1, kw
        msg = lib.anerf_last_error()
        assert b"anerf_train_loss" in msg and word in msg, (kw, msg)
    assert _loss_call(lib, ws_bytes=8) == -3  # ANERF_EWORKSPACE
    assert lib.anerf_train_loss_workspace(0) == 0 and lib.anerf_train_loss_workspace(257) == 8 * (16 + 2 * 10)
    # the backward: the same checks, and its own pointers
    bw = [P, P, None, None, P, None, 1.0, None, 4, 0, 0.1, 1, 1.0, 0, 0.1, P, 1 << 20, P, P, P, None, None, None]
    for at in (0, 4, 15, 17, 18, 19):
        bad = list(bw)
        bad[at] = None
        assert lib.anerf_train_loss_backward(*bad) == -1, at
        assert b"anerf_train_loss_backward" in lib.anerf_last_error()
    bad = list(bw)
    bad[8] = 0
    assert lib.anerf_train_loss_backward(*bad) == -1
    bad = list(bw)
    bad[2] = bad[3] = P  # the coarse pair without its gradient outputs
    assert lib.anerf_train_loss_backward(*bad) == -1 and b"g_rgb0" in lib.anerf_last_error()


def _pose_call(lib, **kw):
    a = dict(cur=P, rot6d=1, anchor=P, kp_idx=P, n=4, nj=24, n_poses=3, kps=P, anchor_kps=P, prev_cur=None,
             next_cur=None, prev_kps=None, next_kps=None, temp_val=None, tol=0.01, coef=2.0, temp_coef=0.05,
             ext_scale=0.001, out=P, ws=P, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.anerf_pose_loss(*a.values())


def test_pose_loss_rejects_bad_arguments():
    lib = _lib.load()
    for kw, word in ((dict(cur=None), b"NULL"), (dict(anchor=None), b"NULL"), (dict(kp_idx=None), b"NULL"),
                     (dict(kps=None), b"NULL"), (dict(anchor_kps=None), b"NULL"), (dict(out=None), b"NULL"),
                     (dict(n=0), b"n and n_poses"), (dict(n_poses=0), b"n and n_poses"), (dict(nj=1), b"n_joints"),
                     (dict(prev_cur=P), b"all or none"), (dict(ext_scale=0.0), b"ext_scale")):
        assert _pose_call(lib, **kw) == -1, kw
        msg = lib.anerf_last_error()
        assert b"anerf_pose_loss" in msg and word in msg, (kw, msg)
    assert _pose_call(lib, ws_bytes=8) == -3
    assert lib.anerf_pose_loss_workspace(4, 1) == 0 and lib.anerf_pose_loss_workspace(0, 24) == 0
    assert lib.anerf_pose_loss_workspace(65, 24) == 8 * 3 * 7  # ceil(65 * 24 / 256) partial rows of 3 doubles
    bw = [P, 1, P, P, 4, 24, 3, P, None, None, None, None, None, 0.01, 2.0, 0.05, P, P, None, None]
    for at, val in ((0, None), (3, None), (16, None), (17, None), (4, 0), (5, 1)):
        bad = list(bw)
        bad[at] = val
        assert lib.anerf_pose_loss_backward(*bad) == -1, at
        assert b"anerf_pose_loss_backward" in lib.anerf_last_error()
    bad = list(bw)
    bad[8:13] = [P] * 5  # the temporal term without g_kps
    assert lib.anerf_pose_loss_backward(*bad) == -1 and b"g_kps" in lib.anerf_last_error()


def test_adam_step_rejects_bad_arguments():
    import ctypes
    lib = _lib.load()
    vp = ctypes.c_void_p

    def call(params=(P,), grads=(P,), m=(P,), v=(P,), numel=(7,), count=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0,
             step=1, base=0, ntens=1, norms=None, ws=P, ws_bytes=1 << 20):
        arr = lambda xs: None if xs is None else (vp * len(xs))(*xs)  # noqa: E731
        nm = None if numel is None else (ctypes.c_int64 * len(numel))(*numel)
        return lib.anerf_adam_step(arr(params), arr(grads), arr(m), arr(v), nm, count, lr, b1, b2, eps, wd, step, base,
                                   ntens, norms, ws, ws_bytes, None)
    for kw, word in ((dict(params=None), b"NULL"), (dict(grads=None), b"NULL"), (dict(numel=None), b"NULL"),
                     (dict(ws=None), b"NULL"), (dict(count=0), b"count"), (dict(step=0), b"step"),
                     (dict(b1=1.0), b"betas"), (dict(lr=-1.0), b"lr"), (dict(grads=(None,)), b"NULL tensor"),
                     (dict(grads=(P + 2,)), b"4-byte"), (dict(numel=(0,)), b"numel"), (dict(base=-1), b"chunk_base"),
                     (dict(norms=P, ntens=0), b"norm_tensors")):
        assert call(**kw) == -1, kw
        msg = lib.anerf_last_error()
        assert b"anerf_adam_step" in msg and word in msg, (kw, msg)
    assert call(ws_bytes=0) == -3
    nm = (ctypes.c_int64 * 3)(1, 2048, 2049)
    assert lib.anerf_adam_step_workspace(nm, 3) == 8 * 4
    assert lib.anerf_adam_step_workspace(None, 3) == 0 and lib.anerf_adam_step_workspace(nm, 0) == 0


# ---- the float64 checkers against torch on the CPU

@pytest.mark.parametrize("loss_fn,beta", [("MSE", 0.1), ("L1", 0.1), ("Huber", 0.1), ("Huber", 0.6)])
@pytest.mark.parametrize("coarse", [True, False])
@pytest.mark.parametrize("bgs", ["per-ray", "base", "off"])
@pytest.mark.parametrize("reg", [None, "BCE"])
def test_nerf_loss_reference_equals_train_nerf_loss(loss_fn, beta, coarse, bgs, reg):
    d = loss_inputs(37, 5)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k in ("rgb", "acc", "rgb0", "acc0"))
         for k, v in d.items()}
    preds = {"rgb_map": t["rgb"], "acc_map": t["acc"]}
    if coarse:
        preds.update(rgb0=t["rgb0"], acc0=t["acc0"])
    kw = dict(use_background=bgs != "off", coarse_weight=0.7, loss_fn=loss_fn, loss_beta=beta, reg_fn=reg, reg_coef=0.3)
    total, parts = train.nerf_loss(preds, t["target"], bgs=t["bgs"] if bgs == "per-ray" else 1.0,
                                   fgs=t["fgs"][:, None], return_dict=True, **kw)
    (total * 0.5).backward()
    ref = T.nerf_loss_reference(d["rgb"], d["acc"], d["target"], d["rgb0"] if coarse else None,
                                d["acc0"] if coarse else None, bgs=d["bgs"] if bgs == "per-ray" else None, base_bg=1.0,
                                fgs=d["fgs"], upstream=0.5, **kw)
    assert abs(ref["total"] - total.item()) <= 1e-13 * abs(total.item())
    for k, v in parts.items():
        assert abs(ref[k] - v.item()) <= 1e-13 * abs(v.item()), k
    for k in ("rgb", "acc") + (("rgb0", "acc0") if coarse else ()):
        got = np.zeros(d[k].shape) if t[k].grad is None else t[k].grad.numpy()  # (acc without background and reg)
        np.testing.assert_allclose(ref["g_" + k], got, rtol=1e-12, atol=1e-16, err_msg=k)
    with torch.no_grad():
        bg = (t["bgs"] if bgs == "per-ray" else 1.0) if bgs != "off" else 0.0
        mse = F.mse_loss(t["rgb"] + (1 - t["acc"])[:, None] * bg, t["target"])
        assert abs(ref["psnr"] - float(-10.0 * torch.log(mse) / np.log(10.0))) <= 1e-12
    assert abs(ref["alpha"] - d["acc"].mean()) <= 1e-15


def test_nerf_loss_reference_without_foreground_rays_is_nan():
    d = loss_inputs(9, 6)
    ref = T.nerf_loss_reference(d["rgb"], d["acc"], d["target"], fgs=np.ones(9), reg_fn="BCE")
    assert np.isnan(ref["reg_loss"]) and np.isnan(ref["total"]) and np.isfinite(ref["g_acc"]).all()
    assert np.all(ref["g_acc"] == 0.0)  # (no background term, no ray under the regulariser)


@pytest.mark.parametrize("rot6d", [True, False])
@pytest.mark.parametrize("temporal", [True, False])
@pytest.mark.parametrize("n,nj", [(1, 2), (5, 24), (7, 3)])
def test_pose_loss_reference_equals_the_torch_expression(rot6d, temporal, n, nj):
    c = pose_case(n, nj, rot6d, temporal, 11)
    a = argparse.Namespace(opt_rot6d=rot6d, opt_pose_tol=c["tol"], opt_pose_coef=c["coef"], use_temp_loss=temporal,
                           temp_coef=c["temp_coef"], ext_scale=c["ext_scale"])
    tt = lambda x, g=False: torch.tensor(x, dtype=torch.float64, requires_grad=g)  # noqa: E731
    cur, kps = tt(c["cur"], True), tt(c["kps"], True)
    anchors = {"kps": tt(c["anchor_kps"]), "rots": tt(c["anchor_full"]), "bones": tt(c["anchor_full"])}
    kp_opts = {"kp_batch": kps, "rots": cur, "bones": cur}
    fk, fc = tt(c["frames_kps"]), tt(c["frames_cur"])
    out = torch_kp_loss(a, anchors, c["kp_idx"], kp_opts, lambda i: (fk[i], fc[i], fc[i]), tt(c["temp_val"]))
    total = out["kp_loss"] + out.get("temp_loss", 0.0)
    (total * 0.5).backward()
    ref = pose_reference(c, upstream=0.5)
    assert (c["cur"] - c["anchor_full"][c["kp_idx"]])[..., :2 if rot6d else 3].__pow__(2).max() > c["tol"]
    for k in ("kp_loss", "MPJPC") + (("temp_loss",) if temporal else ()):
        assert abs(ref[k] - out[k].item()) <= 1e-12 * abs(out[k].item()), k
    assert ref["kp_loss"] > 0 and abs(ref["total"] - total.item()) <= 1e-12 * abs(total.item())
    np.testing.assert_allclose(ref["g_cur"], cur.grad.numpy(), rtol=1e-11, atol=1e-16)
    if rot6d:
        assert np.all(ref["g_cur"][..., 2] == 0.0)
    np.testing.assert_allclose(ref["g_kps"], np.zeros_like(c["kps"]) if kps.grad is None else kps.grad.numpy(),
                               rtol=1e-11, atol=1e-16)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_reference_equals_torch_adam_in_float64(wd):
    rs = np.random.RandomState(3)
    shapes = [(1,), (3,), (17, 5), (257,)]
    ps = [torch.tensor(rs.normal(size=s), dtype=torch.float64, requires_grad=True) for s in shapes]
    opt = torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    mine = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for p in ps]
    for step in range(1, 6):
        lr = 1e-3 * 0.8 ** step
        for g in opt.param_groups:
            g["lr"] = lr
        grads = [rs.normal(size=s) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g)
        opt.step()
        mine = [T.adam_reference(p, g, m, v, step, lr, (0.9, 0.99), 1e-8, wd) for (p, m, v), g in zip(mine, grads)]
        for (p, m, v), tp in zip(mine, ps):
            assert np.abs(p - tp.detach().numpy()).max() <= 1e-12
            assert np.abs(m - opt.state[tp]["exp_avg"].numpy()).max() <= 1e-12
            assert np.abs(v - opt.state[tp]["exp_avg_sq"].numpy()).max() <= 1e-12


# ---- anerf.Adam on the CPU: torch's own step

def _cpu_run(cls, steps=4, **kw):
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in ((5, 3), (7,), (1,))]
    opt = cls(ps, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01, **kw)
    g = torch.Generator().manual_seed(1)
    for _ in range(steps):
        for p in ps[:2]:  # (the third parameter never has a gradient: skipped, no state)
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return ps, opt


def test_anerf_adam_on_cpu_parameters_is_torch_adam():
    ps_a, opt_a = _cpu_run(anerf.Adam)
    ps_b, opt_b = _cpu_run(torch.optim.Adam)
    for a, b in zip(ps_a, ps_b):
        assert torch.equal(a, b)
    sa, sb = opt_a.state_dict(), opt_b.state_dict()
    assert sa["state"].keys() == sb["state"].keys() == {0, 1}
    for k in sa["state"]:
        assert set(sa["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        for name in sa["state"][k]:
            assert torch.equal(sa["state"][k][name], sb["state"][k][name])
    assert opt_a.last_grad_norm() is None  # (only the kernel path writes norms)


def test_anerf_adam_state_dict_round_trips_through_torch_adam():
    ps_a, opt_a = _cpu_run(anerf.Adam)
    ps_t = [torch.nn.Parameter(p.detach().clone()) for p in ps_a]
    opt_t = torch.optim.Adam(ps_t, lr=1.0)
    # (a copy: torch's load_state_dict shares the CPU `step` tensors with the dict it is given)
    opt_t.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    assert opt_t.param_groups[0]["lr"] == 2e-3 and opt_t.param_groups[0]["betas"] == (0.9, 0.99)
    back = anerf.Adam.from_torch(opt_t)
    assert isinstance(back, anerf.Adam) and back.param_groups[0]["weight_decay"] == 0.01
    g = torch.Generator().manual_seed(2)
    grads = [torch.randn(p.shape, generator=g) for p in ps_a[:2]]
    for opt, ps in ((opt_a, ps_a), (back, ps_t)):
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
    for a, b in zip(ps_a, ps_t):
        assert torch.equal(a, b)
    assert float(back.state[ps_t[0]]["step"]) == 5.0


def test_anerf_adam_calls_on_step_only_for_kernel_updates():
    calls = []
    ps, opt = _cpu_run(anerf.Adam, steps=1, on_step=lambda: calls.append(1))
    assert calls == []  # (CPU parameters: torch's step, nothing the version counters miss)


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "capturable", "differentiable", "fused"])
def test_anerf_adam_refuses_unsupported_modes(flag):
    with pytest.raises(NotImplementedError, match=flag):
        anerf.Adam([torch.nn.Parameter(torch.zeros(3))], **{flag: True})


# ---- refusals

@pytest.mark.parametrize("reg", ["L1", "MSE"])
def test_unreduced_regularisers_are_refused(reg):
    with pytest.raises(NotImplementedError, match="unreduced") as e:
        T.LossSpec(reg_fn=reg)
    assert "backward() raises" in str(e.value)
    with pytest.raises(NotImplementedError):
        T.nerf_loss_reference(np.zeros((2, 3)), np.zeros(2), np.zeros((2, 3)), reg_fn=reg)


def test_unknown_loss_is_refused():
    with pytest.raises(NotImplementedError, match="loss_fn"):
        T.LossSpec(loss_fn="SSIM")


def test_temporal_neighbours_wrap_like_the_reference():
    idx = np.array([0, 1, 2, 0])
    prev, nxt = T.temporal_neighbours(idx, 3)
    table = np.arange(3) * 10
    assert np.array_equal(table[prev], table[idx - 1])  # (NumPy's -1: the last pose)
    assert np.array_equal(nxt, (idx + 1) % 3)
    tp, tn = T.temporal_neighbours(torch.tensor(idx), 3)
    assert tp.tolist() == prev.tolist() and tn.tolist() == nxt.tolist()


def test_decay_follows_the_reference_expression():
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.Adam([p], lr=5e-4)
    p.grad = torch.ones(2)
    for _ in range(7):
        opt.step()
    lr, _ = T.decay_optimizer_lrate(5e-4, 2, 0.1, opt, decay_unit=3)
    step = opt.state[p]["step"]
    assert isinstance(lr, float) and lr == float(5e-4 * (0.1 ** ((step // 3) / 2)))
    assert opt.param_groups[0]["lr"] == lr and lr < 5e-4


def test_trainer_fixture_meta():
    """tests/golden/tr1_popt_d4w128.npz loads, its seeded checkpoint's sha256 matches (Golden asserts it), and it holds
    what the GPU trajectory test reads."""
    from _golden import Golden
    g = Golden("tr1_popt_d4w128")
    m = g.meta
    assert (m["D"], m["W"], m["NJ"], m["S"], m["I"], m["K"], m["n_rays"], m["n_poses"]) == (4, 128, 24, 32, 16, 6, 64, 4)
    for flag in ("--use_background", "--opt_pose", "--opt_rot6d", "--use_temp_loss", "--opt_pose_step", "--opt_pose_stop"):
        assert flag in m["train_flags"]
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                        "tr1_popt_d4w128.npz")) <= 650 * 1024
    for i in range(m["K"]):
        assert g[f"s{i}_rays_o"].shape == (64, 3) and g[f"s{i}_t_rand"].shape == (64, 32)
        assert ("kp_loss" in m["loss_keys"][i]) == (i < 4) and "total_norm" in m["stat_keys"][i]
    lr = [float(g[f"s{i}_stat_lrate"]) for i in range(m["K"])]
    tau = [float(g[f"s{i}_stat_cutoff"]) for i in range(m["K"])]
    assert lr[0] > lr[1] > lr[3] > lr[5] and tau == sorted(tau) and tau[0] < tau[-1]  # (both schedules move)
    assert {0, m["n_poses"] - 1} <= set(g["s0_pose"].tolist())  # (both wraps of the temporal neighbours)


def test_trainer_fixture_meta_tr2():
    """tests/golden/tr2_nopopt_d8w256.npz: 8 x 256, 32 rays, 3 steps, no pose layer, Huber + the BCE regulariser."""
    from _golden import Golden
    g = Golden("tr2_nopopt_d8w256")
    m = g.meta
    assert (m["D"], m["W"], m["K"], m["n_rays"], m["popt"]) == (8, 256, 3, 32, False)
    assert m["train_flags"][m["train_flags"].index("--loss_fn") + 1] == "Huber" and "BCE" in m["train_flags"]
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                        "tr2_nopopt_d8w256.npz")) <= 650 * 1024
    for i in range(3):
        assert m["loss_keys"][i] == ["reg_loss", "reg_loss0", "rgb_loss", "rgb_loss0", "total_loss"]
        fgs = g[f"s{i}_fgs"]
        assert fgs.shape == (32,) and (fgs < 1).any() and (fgs == 1).any()

"""The reference's training step as a product class: `Trainer` (core/trainer.py:205-517), `create_popt`
(core/pose_opt.py:14-83) and an `Adam` whose update is one kernel over every parameter tensor.

`Trainer.train_batch` is what run_nerf.py's loop hands its batches to.  Its tail -- the image loss, the pose loss,
the optimizer update and the gradient norms -- runs on three hand-written kernels (csrc/anerf_step.hip):

* `anerf_train_loss` / `_backward`: Trainer._compute_nerf_loss for the fine and the coarse outputs;
* `anerf_pose_loss` / `_backward`: Trainer._compute_kp_loss with the temporal term;
* `anerf_adam_step`: torch.optim.Adam's update over a table of tensors, with get_gradnorm's sums in the same pass.

The step issues without waiting for the device: the pose indices stay on the device, every statistic lands in one
buffer, and `train_batch` reads that buffer once, after the whole step has been issued.  (The reference's step reads
one value per statistic and per parameter tensor, about 50 waits.)

Two deliberate differences from the reference:

* `optimize` reports the norm of the gradients the step used in both of its branches.  The reference's pose branch
  calls get_gradnorm after `_optim_step` has reset the gradients (core/trainer.py:471-473): with torch >= 2
  (set_to_none) it divides by zero, with torch 1.x it reports 0.
* `reg_fn` 'L1' / 'MSE' are refused: with reduction='off' the reference's img2l1 / img2mse return the unreduced tensor
  (core/trainer.py:20-25, 37-42), the total loss is then not a scalar and its backward() raises.

`nerf_loss_reference`, `pose_loss_reference` and `adam_reference` are float64 NumPy statements of what the kernels
compute (values and gradients), for the tests.
"""
import copy
import ctypes

import numpy as np
import torch

from . import _lib
from .kinematics import PoseOptLayer, pose_kinematics
from .render import render

LOSS_STATS = ("rgb_loss", "rgb_loss0", "reg_loss", "reg_loss0", "psnr", "psnr0", "alpha", "total")  # anerf_train_loss
POSE_STATS = ("kp_loss", "temp_loss", "MPJPC", "total")  # anerf_pose_loss
# the Trainer's one statistics buffer: the two kernels' outputs, then the network's and the pose layer's
# (total_norm, avg_norm)
N_STATS = len(LOSS_STATS) + len(POSE_STATS) + 4
_NORM_AT = len(LOSS_STATS) + len(POSE_STATS)


# ----------------------------------------------------------------------------------------------------------------------
# float64 checkers

def _elem_loss(kind, beta, d):
    if kind == "MSE":
        return d * d, 2.0 * d
    if kind == "L1" or (kind == "Huber" and beta == 0.0):
        return np.abs(d), np.sign(d)
    if kind == "Huber":
        small = np.abs(d) < beta
        return (np.where(small, 0.5 * d * d / beta, np.abs(d) - 0.5 * beta),
                np.where(small, d / beta, np.sign(d)))
    raise NotImplementedError(f"loss {kind!r}")


def nerf_loss_reference(rgb, acc, target, rgb0=None, acc0=None, bgs=None, base_bg=1.0, fgs=None, loss_fn="MSE",
                        loss_beta=0.1, use_background=False, coarse_weight=1.0, reg_fn=None, reg_coef=0.1,
                        upstream=1.0):
    """Trainer._compute_nerf_loss + compute_loss's sum (core/trainer.py:319-380) in float64 NumPy: a dict with
    anerf_train_loss's eight values (LOSS_STATS) and the gradients g_rgb, g_acc (g_rgb0, g_acc0) of `total`
    times `upstream`.  fgs: [n] (the batch's fgs[..., 0])."""
    if reg_fn not in (None, "BCE"):
        raise NotImplementedError(f"reg_fn {reg_fn!r}")
    f8 = lambda x: None if x is None else np.asarray(x, np.float64)  # noqa: E731
    target, bgs, fgs = f8(target), f8(bgs), f8(fgs)
    n = target.shape[0]
    out = {k: 0.0 for k in LOSS_STATS}

    def one(rgb, acc, tag, w):
        rgb, acc = f8(rgb), f8(acc)
        bg = (bgs if bgs is not None else np.full((n, 3), float(base_bg))) if use_background else np.zeros((n, 3))
        d = rgb + (1.0 - acc)[:, None] * bg - target
        l, g = _elem_loss(loss_fn, float(loss_beta), d)
        out["rgb_loss" + tag] = l.mean() * w
        out["psnr" + tag] = -10.0 * np.log((d * d).mean()) / np.log(10.0)
        g_rgb = g * (w * upstream / (3.0 * n))
        g_acc = -(g_rgb * bg).sum(-1)
        if reg_fn == "BCE":
            m = fgs < 1.0
            eps = 1e-8
            with np.errstate(invalid="ignore", divide="ignore"):
                bce = -(fgs * np.log(acc + eps) + (1.0 - fgs) * np.log(1.0 - acc + eps))
                out["reg_loss" + tag] = (bce[m].sum() / m.sum() if m.any() else np.nan) * reg_coef
                gb = -(fgs / (acc + eps) - (1.0 - fgs) / (1.0 - acc + eps))
                g_acc = g_acc + np.where(m, gb * (reg_coef * upstream / max(m.sum(), 1)), 0.0)
        return g_rgb, g_acc

    out["g_rgb"], out["g_acc"] = one(rgb, acc, "", 1.0)
    out["alpha"] = f8(acc).mean()
    if rgb0 is not None:
        out["g_rgb0"], out["g_acc0"] = one(rgb0, acc0, "0", float(coarse_weight))
    out["total"] = out["rgb_loss"] + out["reg_loss"] + out["rgb_loss0"] + out["reg_loss0"]
    return out


def temporal_neighbours(kp_idx, n_poses):
    """The previous and the next pose of every index, as the reference takes them (core/trainer.py:410-411): kp_idx - 1,
    where -1 names the last pose (NumPy's negative index), and (kp_idx + 1) % n_poses."""
    if isinstance(kp_idx, torch.Tensor):
        return torch.remainder(kp_idx - 1, n_poses), torch.remainder(kp_idx + 1, n_poses)
    kp_idx = np.asarray(kp_idx)
    return (kp_idx - 1) % n_poses, (kp_idx + 1) % n_poses


def _cur6(cur, rot6d):
    cur = np.asarray(cur, np.float64)
    return cur[..., :3, :2].reshape(*cur.shape[:-2], 6) if rot6d else cur


def pose_loss_reference(cur, anchor, kp_idx, kps, anchor_kps, rot6d=True, tol=0.0, coef=1.0, prev_cur=None,
                        next_cur=None, prev_kps=None, next_kps=None, temp_val=None, temp_coef=0.05, ext_scale=0.001,
                        upstream=1.0):
    """Trainer._compute_kp_loss (core/trainer.py:382-441) in float64 NumPy: a dict with anerf_pose_loss's four values
    (POSE_STATS) and the gradients g_cur (in cur's layout: [n, NJ, 3, 3] with a zero third column when rot6d) and g_kps
    of `total` times `upstream`.  cur / prev_cur / next_cur: rotations [n, NJ, 3, 3] (rot6d) or bones [n, NJ, 3]."""
    b = _cur6(cur, rot6d)
    kp_idx = np.asarray(kp_idx)
    kps = np.asarray(kps, np.float64)
    n, nj = b.shape[:2]
    reg = np.asarray(anchor, np.float64)[kp_idx]
    diff = (reg - b)[:, 1:]
    d = diff ** 2
    mask = d > tol
    out = {"kp_loss": np.where(mask, d - tol, 0.0).sum(-1).mean() * coef, "temp_loss": 0.0}
    g = np.zeros_like(b)
    g[:, 1:] = np.where(mask, -2.0 * diff, 0.0) * (coef * upstream / (n * (nj - 1)))
    g_kps = np.zeros_like(kps)
    if prev_cur is not None:
        tv = np.asarray(temp_val, np.float64)[:, None]
        v = (b - _cur6(prev_cur, rot6d)) - (_cur6(next_cur, rot6d) - b)
        u = (kps - np.asarray(prev_kps, np.float64)) - (np.asarray(next_kps, np.float64) - kps)
        out["temp_loss"] = (((v ** 2).sum(-1) + (u ** 2).sum(-1)) * tv).mean() * temp_coef
        s = temp_coef * upstream / (n * nj)
        g += 4.0 * v * tv[..., None] * s
        g_kps = 4.0 * u * tv[..., None] * s
    pjpc = np.sqrt(((np.asarray(anchor_kps, np.float64)[kp_idx] - kps) ** 2).sum(-1))
    out["MPJPC"] = pjpc.mean() / ext_scale
    out["total"] = out["kp_loss"] + out["temp_loss"]
    if rot6d:
        g9 = np.zeros(b.shape[:2] + (3, 3))
        g9[..., :2] = g.reshape(n, nj, 3, 2)
        g = g9
    out["g_cur"], out["g_kps"] = g, g_kps
    return out


def adam_reference(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """One torch.optim.Adam update (number `step`, from 1) of one tensor in float64 NumPy -> (param, exp_avg,
    exp_avg_sq)."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (param, grad, exp_avg, exp_avg_sq))
    b1, b2 = betas
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


# ----------------------------------------------------------------------------------------------------------------------
# the kernels

def _f32(t, dev=None):
    """float32, contiguous, on the device (None passes)."""
    if t is None:
        return None
    return t.to(device=dev or t.device, dtype=torch.float32).contiguous()


def _reg_kind(reg_fn):
    if reg_fn is None:
        return _lib.ANERF_REG_NONE
    if reg_fn == "BCE":
        return _lib.ANERF_REG_BCE
    if reg_fn in ("L1", "MSE"):
        raise NotImplementedError(
            f"reg_fn {reg_fn!r}: with reduction='off' the reference's img2l1 / img2mse return the unreduced tensor "
            "(core/trainer.py:20-25, 37-42), so its total loss is not a scalar and backward() raises; only 'BCE' "
            "is a usable regulariser")
    raise NotImplementedError(f"reg_fn {reg_fn!r}")


def _loss_kind(loss_fn):
    if loss_fn not in _lib.ANERF_LOSS_KINDS:
        raise NotImplementedError(f"loss_fn {loss_fn!r}: 'MSE', 'L1' or 'Huber'")
    return _lib.ANERF_LOSS_KINDS[loss_fn]


class LossSpec:
    """The options of anerf_train_loss (the reference's args.loss_fn, loss_beta, use_background, coarse_weight, reg_fn,
    reg_coef and _compute_nerf_loss's base_bg)."""

    def __init__(self, loss_fn="MSE", loss_beta=0.1, use_background=False, coarse_weight=1.0, reg_fn=None,
                 reg_coef=0.1, base_bg=1.0):
        self.kind, self.reg = _loss_kind(loss_fn), _reg_kind(reg_fn)
        self.beta, self.use_background = float(loss_beta), bool(use_background)
        self.coarse_weight, self.reg_coef, self.base_bg = float(coarse_weight), float(reg_coef), float(base_bg)


def _loss_args(spec, rgb, acc, rgb0, acc0, target, bgs, fgs):
    n = int(rgb.shape[0])
    if rgb.shape != (n, 3) or acc.shape != (n,) or target.shape != (n, 3):
        raise ValueError("rgb [n, 3], acc [n], target [n, 3]")
    if (rgb0 is None) != (acc0 is None) or (rgb0 is not None and (rgb0.shape != (n, 3) or acc0.shape != (n,))):
        raise ValueError("rgb0 [n, 3] and acc0 [n]: both or neither")
    if bgs is not None and bgs.shape != (n, 3):
        raise ValueError("bgs [n, 3]")
    if spec.reg != _lib.ANERF_REG_NONE and (fgs is None or fgs.shape != (n,)):
        raise ValueError("reg_fn needs the batch's fgs [n]")
    return (_lib.ptr(rgb), _lib.ptr(acc), _lib.ptr(rgb0), _lib.ptr(acc0), _lib.ptr(target), _lib.ptr(bgs),
            spec.base_bg, _lib.ptr(fgs), n, spec.kind, spec.beta, int(spec.use_background), spec.coarse_weight,
            spec.reg, spec.reg_coef)


def train_loss_forward(spec, rgb, acc, target, rgb0=None, acc0=None, bgs=None, fgs=None, out=None):
    """anerf_train_loss on float32 contiguous device tensors -> (out [8] (LOSS_STATS), workspace for the backward)."""
    dev = rgb.device
    args = _loss_args(spec, rgb, acc, rgb0, acc0, target, bgs, fgs)
    need = _lib.workspace("anerf_train_loss_workspace", args[8])
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(len(LOSS_STATS), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().anerf_train_loss(*args, _lib.ptr(out), _lib.ptr(ws), need, _lib.stream_handle(dev)),
                   "anerf_train_loss")
    return out, ws


def train_loss_backward(spec, ws, upstream, rgb, acc, target, rgb0=None, acc0=None, bgs=None, fgs=None):
    """anerf_train_loss_backward -> (g_rgb, g_acc, g_rgb0, g_acc0); upstream: a float32 device scalar."""
    dev = rgb.device
    args = _loss_args(spec, rgb, acc, rgb0, acc0, target, bgs, fgs)
    g_rgb, g_acc = torch.empty_like(rgb), torch.empty_like(acc)
    g_rgb0 = None if rgb0 is None else torch.empty_like(rgb0)
    g_acc0 = None if acc0 is None else torch.empty_like(acc0)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().anerf_train_loss_backward(*args, _lib.ptr(ws), ws.numel() * 8, _lib.ptr(upstream),
                                                         _lib.ptr(g_rgb), _lib.ptr(g_acc), _lib.ptr(g_rgb0),
                                                         _lib.ptr(g_acc0), _lib.stream_handle(dev)),
                   "anerf_train_loss_backward")
    return g_rgb, g_acc, g_rgb0, g_acc0


class PoseSpec:
    """The constants of anerf_pose_loss: the anchor tables, the batch's pose indices, the (detached) neighbours of the
    temporal term and the reference's args.opt_rot6d, opt_pose_tol, opt_pose_coef, temp_coef, ext_scale."""

    def __init__(self, anchor, anchor_kps, kp_idx, rot6d=True, tol=0.0, coef=0.0, prev_cur=None, next_cur=None,
                 prev_kps=None, next_kps=None, temp_val=None, temp_coef=0.05, ext_scale=0.001):
        self.anchor, self.anchor_kps, self.kp_idx = anchor, anchor_kps, kp_idx
        self.rot6d, self.tol, self.coef = bool(rot6d), float(tol), float(coef)
        self.temporal = (prev_cur, next_cur, prev_kps, next_kps, temp_val)
        if any(t is None for t in self.temporal) != all(t is None for t in self.temporal):
            raise ValueError("the temporal term takes prev / next cur and kps and temp_val: all or none")
        self.temp_coef, self.ext_scale = float(temp_coef), float(ext_scale)

    @property
    def has_temporal(self):
        return self.temporal[0] is not None


def _pose_shapes(spec, cur, kps):
    n, nj = int(kps.shape[0]), int(kps.shape[1])
    nc = 6 if spec.rot6d else 3
    want = (n, nj, 3, 3) if spec.rot6d else (n, nj, 3)
    if cur.shape != want or kps.shape != (n, nj, 3):
        raise ValueError(f"cur {want} and kps [n, NJ, 3]")
    N = int(spec.anchor.shape[0])
    if spec.anchor.shape != (N, nj, nc) or spec.anchor_kps.shape != (N, nj, 3):
        raise ValueError(f"anchor [N, NJ, {nc}] and anchor_kps [N, NJ, 3]")
    if spec.kp_idx.shape != (n,) or spec.kp_idx.dtype != torch.int64:
        raise ValueError("kp_idx [n] int64")
    if spec.has_temporal:
        pc, nx, pk, nk, tv = spec.temporal
        if pc.shape != want or nx.shape != want or pk.shape != (n, nj, 3) or nk.shape != (n, nj, 3) or tv.shape != (n,):
            raise ValueError("prev / next cur as cur, prev / next kps as kps, temp_val [n]")
    return n, nj, N


def pose_loss_forward(spec, cur, kps, out=None):
    """anerf_pose_loss on float32 contiguous device tensors -> out [4] (POSE_STATS)."""
    dev = cur.device
    n, nj, N = _pose_shapes(spec, cur, kps)
    need = _lib.workspace("anerf_pose_loss_workspace", n, nj)
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(len(POSE_STATS), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().anerf_pose_loss(
            _lib.ptr(cur), int(spec.rot6d), _lib.ptr(spec.anchor), _lib.ptr(spec.kp_idx), n, nj, N, _lib.ptr(kps),
            _lib.ptr(spec.anchor_kps), *(_lib.ptr(t) for t in spec.temporal), spec.tol, spec.coef, spec.temp_coef,
            spec.ext_scale, _lib.ptr(out), _lib.ptr(ws), need, _lib.stream_handle(dev)), "anerf_pose_loss")
    return out


def pose_loss_backward(spec, upstream, cur, kps):
    """anerf_pose_loss_backward -> (g_cur, g_kps or None without the temporal term)."""
    dev = cur.device
    n, nj, N = _pose_shapes(spec, cur, kps)
    g_cur = torch.empty_like(cur)
    g_kps = torch.empty_like(kps) if spec.has_temporal else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().anerf_pose_loss_backward(
            _lib.ptr(cur), int(spec.rot6d), _lib.ptr(spec.anchor), _lib.ptr(spec.kp_idx), n, nj, N, _lib.ptr(kps),
            *(_lib.ptr(t) for t in spec.temporal), spec.tol, spec.coef, spec.temp_coef, _lib.ptr(upstream),
            _lib.ptr(g_cur), _lib.ptr(g_kps), _lib.stream_handle(dev)), "anerf_pose_loss_backward")
    return g_cur, g_kps


class _StepLoss(torch.autograd.Function):
    """The step's total loss as ONE autograd node over both loss kernels: forward fills `stats` (LOSS_STATS, then
    POSE_STATS when there is a pose term) and returns the total; backward runs the two backward kernels on the
    upstream gradient where it is, on the device."""

    @staticmethod
    def forward(ctx, spec, pose, stats, target, bgs, fgs, rgb, acc, rgb0, acc0, cur, kps):
        nl = len(LOSS_STATS)
        _, ws = train_loss_forward(spec, rgb, acc, target, rgb0, acc0, bgs, fgs, out=stats[:nl])
        if pose is not None:
            pose_loss_forward(pose, cur, kps, out=stats[nl:nl + len(POSE_STATS)])
            total = stats[nl - 1] + stats[nl + len(POSE_STATS) - 1]
        else:
            total = stats[nl - 1].clone()
        ctx.spec, ctx.pose, ctx.consts = spec, pose, (target, bgs, fgs)
        ctx.save_for_backward(ws, rgb, acc, rgb0, acc0, cur, kps)
        return total

    @staticmethod
    def backward(ctx, g):
        ws, rgb, acc, rgb0, acc0, cur, kps = ctx.saved_tensors
        target, bgs, fgs = ctx.consts
        g = g.to(torch.float32).contiguous()
        g_rgb, g_acc, g_rgb0, g_acc0 = train_loss_backward(ctx.spec, ws, g, rgb, acc, target, rgb0, acc0, bgs, fgs)
        g_cur = g_kps = None
        if ctx.pose is not None and (ctx.needs_input_grad[10] or ctx.needs_input_grad[11]):
            g_cur, g_kps = pose_loss_backward(ctx.pose, g, cur, kps)
        return None, None, None, None, None, None, g_rgb, g_acc, g_rgb0, g_acc0, g_cur, g_kps


def step_loss(spec, rgb, acc, target, rgb0=None, acc0=None, bgs=None, fgs=None, pose=None, cur=None, kps=None,
              stats=None):
    """total loss (a 0-d tensor whose backward() reaches rgb, acc, rgb0, acc0, cur and kps) and the statistics buffer
    (float32, device: LOSS_STATS then POSE_STATS; the pose entries are written only with `pose`, a PoseSpec)."""
    dev = rgb.device
    if stats is None:
        stats = torch.empty(N_STATS, dtype=torch.float32, device=dev)
    det = lambda t: None if t is None else _f32(t.detach(), dev)  # noqa: E731
    grad = lambda t: None if t is None else _f32(t, dev)  # noqa: E731
    total = _StepLoss.apply(spec, pose, stats, det(target), det(bgs), det(fgs), grad(rgb), grad(acc), grad(rgb0),
                            grad(acc0), grad(cur), grad(kps))
    return total, stats


# ----------------------------------------------------------------------------------------------------------------------
# Adam

def _kernel_param(p):
    return p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and not p.grad.is_sparse and p.numel() > 0


class Adam(torch.optim.Adam):
    """torch.optim.Adam whose step() updates every CUDA float32 parameter in one launch sequence (anerf_adam_step:
    64 tensors per launch, the gradients' norms in the same pass, no host synchronisation).  State and state_dict()
    are torch's own (`step`, `exp_avg`, `exp_avg_sq`), so checkpoints move between the two freely.

    * parameters without a gradient are skipped; CPU (or non-float32) parameters go to torch's own step();
    * `on_step`: called after a step that wrote CUDA parameters.  The kernel writes them without advancing their
      version counters, so whoever caches by version (TrainRayCaster's eval caster) needs the call: the Trainer
      sets it to `TrainRayCaster.weights_changed`;
    * `last_grad_norm()`: the device buffer [total_norm, avg_norm] (get_gradnorm, core/trainer.py:191-203) of the
      gradients the last step used; `norm_buffer` may be pointed at a caller's two floats;
    * amsgrad, maximize, capturable, differentiable and fused are refused."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 maximize=False, capturable=False, differentiable=False, fused=None, foreach=None, on_step=None):
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable),
                         ("differentiable", differentiable), ("fused", fused)):
            if on:
                raise NotImplementedError(f"anerf Adam: {name} is not supported")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=foreach)
        self.on_step = on_step
        self.norm_buffer = None
        self._norms = None

    @classmethod
    def from_torch(cls, optimizer, on_step=None):
        """This Adam over a torch.optim.Adam's parameter groups and a copy of its state (what create_raycaster
        returns).  (A copy: load_state_dict shares the CPU `step` tensors with the dict it is given, and two
        optimizers stepping one counter would both skip update numbers.)"""
        g0 = optimizer.param_groups[0]
        new = cls([{k: v for k, v in g.items() if k in ("params", "lr", "betas", "eps", "weight_decay")}
                   for g in optimizer.param_groups], lr=g0["lr"], betas=g0["betas"], eps=g0["eps"],
                  weight_decay=g0["weight_decay"], on_step=on_step)
        new.load_state_dict(copy.deepcopy(optimizer.state_dict()))
        return new

    def last_grad_norm(self):
        return self._norms

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._norms = None  # (written by the kernel path only: None after a step that did not take it)
        jobs, rest = {}, []  # (device, step, lr, betas, eps, weight_decay) -> [(p, grad, state)]
        for group in self.param_groups:
            for flag in ("amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
                if group.get(flag):
                    raise NotImplementedError(f"anerf Adam: {flag} is not supported")
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not _kernel_param(p):
                    rest.append(p)
                    continue
                state = self.state[p]
                if len(state) == 0:  # (torch's _init_group)
                    state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() ==
                                                 torch.float64 else torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():  # (a view with a 4-byte offset passes as it is)
                    g = g.to(torch.float32).contiguous()
                b1, b2 = group["betas"]
                key = (p.device, int(state["step"]) + 1, float(group["lr"]), float(b1), float(b2),
                       float(group["eps"]), float(group["weight_decay"]))
                jobs.setdefault(key, []).append((p, g, state))
        if jobs:
            self._launch(jobs)
        if rest:
            # torch's own step for what the kernel does not take: hide the gradients of what it did
            done = [(p, p.grad) for job in jobs.values() for p, _, _ in job]
            for p, _ in done:
                p.grad = None
            try:
                super().step()
            finally:
                for p, g in done:
                    p.grad = g
        if jobs and self.on_step is not None:
            self.on_step()
        return loss

    def _launch(self, jobs):
        lib = _lib.load()
        devices = {k[0] for k in jobs}
        if len(devices) != 1:
            raise NotImplementedError("anerf Adam: parameters on more than one CUDA device")
        dev = devices.pop()
        every = [e for job in jobs.values() for e in job]
        numel_all = (ctypes.c_int64 * len(every))(*[p.numel() for p, _, _ in every])
        need = _lib.workspace("anerf_adam_step_workspace", numel_all, len(every))
        ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
        norms = self.norm_buffer if self.norm_buffer is not None else torch.empty(2, dtype=torch.float32, device=dev)
        vp = ctypes.c_void_p
        base, left = 0, len(jobs)
        with torch.cuda.device(dev):
            stream = _lib.stream_handle(dev)
            for (_, step, lr, b1, b2, eps, wd), job in jobs.items():
                k = len(job)
                left -= 1
                numel = (ctypes.c_int64 * k)(*[p.numel() for p, _, _ in job])
                rc = lib.anerf_adam_step((vp * k)(*[p.data_ptr() for p, _, _ in job]),
                                         (vp * k)(*[g.data_ptr() for _, g, _ in job]),
                                         (vp * k)(*[s["exp_avg"].data_ptr() for _, _, s in job]),
                                         (vp * k)(*[s["exp_avg_sq"].data_ptr() for _, _, s in job]), numel, k, lr, b1,
                                         b2, eps, wd, step, base, len(every), _lib.ptr(norms) if left == 0 else None,
                                         _lib.ptr(ws), need, stream)
                _lib.check(rc, "anerf_adam_step")
                base += _lib.workspace("anerf_adam_step_workspace", numel, k) // 8  # (one double per chunk)
                for _, _, s in job:
                    s["step"] += 1
        self._norms = norms


@torch.no_grad()
def grad_norms(params, out=None):
    """get_gradnorm (core/trainer.py:191-203) on the device: [total_norm, avg_norm] over the parameters that have a
    gradient, without a host read per tensor (for optimizers other than this module's Adam)."""
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:  # (the reference divides by zero here; a step without gradients has norm 0)
        return torch.zeros(2) if out is None else out.zero_()
    sq = torch.stack([n.to(grads[0].device) for n in torch._foreach_norm(grads)]).double().square().sum()
    both = torch.stack([sq.sqrt(), (sq / len(grads)).sqrt()]).float()
    if out is None:
        return both
    out.copy_(both)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the Trainer

def decay_optimizer_lrate(lrate, lrate_decay, decay_rate, optimizer, global_step=None, decay_unit=1000):
    """The reference's exponential decay (core/trainer.py:173-183): lrate * decay_rate ** (k / lrate_decay), k the
    number of whole `decay_unit`s in the first parameter's Adam update count (not in global_step, which is unused).
    torch >= 2 keeps that count as a float32 CPU tensor, so the reference's rate is float32 arithmetic; the same
    float32 operations run here, and the rate is set and returned as a Python float -> (rate, None)."""
    state = optimizer.state.get(optimizer.param_groups[0]["params"][0], {})
    count = torch.as_tensor(state.get("step", 0.0), dtype=torch.float32).cpu()
    units = torch.div(count, decay_unit, rounding_mode="floor")
    rate = float(torch.mul(torch.pow(decay_rate, torch.div(units, lrate_decay)), lrate))
    for group in optimizer.param_groups:
        group["lr"] = rate
    return rate, None


def dict_to_device(d, device):
    return {k: (d[k].to(device) if torch.is_tensor(d[k]) else d[k]) for k in d}


class Trainer:
    """The reference's Trainer (core/trainer.py:205-517): same constructor, same methods (train_batch, get_fwd_args,
    get_kp_args, compute_loss, optimize, save_nerf, save_popt), same loss_dict / stats keys.

    args: the reference's parsed arguments (attributes missing from it take run_nerf.py's defaults).
    render_kwargs_train / _test: create_raycaster's; popt_kwargs: create_popt's, or None without pose optimisation.
    `optimizer` / `pose_optimizer` may be this module's Adam (the step then runs on anerf_adam_step and yields the
    gradient norms; its on_step hook is set to the caster's weights_changed) or stock torch optimizers.

    What differs from the reference, besides the two points of the module docstring:
    * `train_batch` reads the device once per call (one statistics buffer, after the whole step has been issued) and
      returns Python floats in `stats`; `loss_dict` holds device tensors, `loss_dict['total_loss']` with its graph;
    * `compute_loss` and `optimize`, called on their own, return their statistics as 0-d device tensors;
    * `train_batch(..., rand=)` passes recorded random draws to TrainRayCaster.render_rays (tests)."""

    def __init__(self, args, data_attrs, optimizer, pose_optimizer, render_kwargs_train, render_kwargs_test,
                 popt_kwargs=None, device=None):
        self.args = args
        self.optimizer = optimizer
        self.pose_optimizer = pose_optimizer
        self.render_kwargs_train = render_kwargs_train
        self.render_kwargs_test = render_kwargs_test
        self.popt_kwargs = popt_kwargs
        caster = render_kwargs_train["ray_caster"]
        self.device = torch.device(device) if device is not None else caster._dev
        self.hwf = data_attrs["hwf"]
        self.data_attrs = data_attrs
        self.loss_spec = LossSpec(self._arg("loss_fn", "MSE"), self._arg("loss_beta", 0.1),
                                  self._arg("use_background", False), self._arg("coarse_weight", 1.0),
                                  self._arg("reg_fn", None), self._arg("reg_coef", 0.1))
        if isinstance(optimizer, Adam) and optimizer.on_step is None:
            optimizer.on_step = caster.module.weights_changed
        self._stats = None
        self._stat_views = {}
        self._anchor_dev = None

    def _arg(self, name, default):
        return getattr(self.args, name, default)

    # -- the step
    def train_batch(self, batch, i=0, global_step=0, rand=None):
        """One training step on `batch` (core/trainer.py:230-273) -> (loss_dict, stats)."""
        args = self.args
        H, W, focal = self.hwf
        batch = dict_to_device(batch, self.device)
        self._stats = torch.empty(N_STATS, dtype=torch.float32, device=self.device)
        stop = self._arg("opt_pose_stop", None)
        popt_detach = not (stop is None or i < stop)
        kp_args, extra_args = self.get_kp_args(batch, detach=popt_detach)
        fwd_args = self.get_fwd_args(batch)
        extra_render = {} if rand is None else {"rand": rand}
        preds = render(H, W, focal, chunk=self._arg("chunk", 1024 * 32), verbose=i < 10, retraw=False, **kp_args,
                       **fwd_args, **extra_render, **self.render_kwargs_train)
        no_pose = popt_detach or not self._arg("opt_pose", False)
        loss_dict, stats = self.compute_loss(batch, preds, kp_opts={**kp_args, **extra_args}, popt_detach=no_pose)
        optim_stats = self.optimize(loss_dict["total_loss"], i, no_pose)
        new_lrate, _ = decay_optimizer_lrate(self._arg("lrate", 5e-4), self._arg("lrate_decay", 250),
                                             decay_rate=self._arg("lrate_decay_rate", 0.1), optimizer=self.optimizer,
                                             global_step=global_step, decay_unit=self._arg("decay_unit", 1000))
        ray_caster = self.render_kwargs_train["ray_caster"]
        if not self._arg("finetune", False):
            ray_caster.module.update_embed_fns(global_step, args)
        # the step's one device read: every statistic of it
        host = self._stats.cpu()
        at = {id(t): k for k, t in self._stat_views.items()}
        value = lambda t: float(host[at[id(t)]]) if id(t) in at else float(t)  # noqa: E731
        stats = {"lrate": new_lrate, "alpha": float(host[LOSS_STATS.index("alpha")]),
                 "cutoff": ray_caster.module.embed_fn.get_tau(), **{k: value(v) for k, v in stats.items()},
                 **{k: value(v) for k, v in optim_stats.items()}}
        return loss_dict, stats

    def get_fwd_args(self, batch):
        return {"rays": batch["rays"], "cams": batch["cam_idxs"] if self._arg("opt_framecode", False) else None,
                "subject_idxs": batch.get("subject_idxs", None)}

    def get_kp_args(self, batch, detach=False):
        """Human pose data from the batch or from the pose layer (core/trainer.py:285-312).  The pose indices go to the
        layer as a device tensor.  With the temporal loss, where the layer evaluates every frame at once
        (PoseOptLayer.all_frames), that one evaluation also serves both neighbours of the batch (extras['_frames'])."""
        extras = {}
        if self.popt_kwargs is None or self.popt_kwargs["popt_layer"] is None:
            return self._create_kp_args_dict(kps=batch["kp3d"], skts=batch["skts"], bones=batch["bones"],
                                             cyls=batch["cyls"]), extras
        layer = self.popt_kwargs["popt_layer"]
        kp_idx = torch.as_tensor(batch["kp_idx"]).to(self.device, torch.long).reshape(-1)
        from .kinematics import ALL_FRAMES_MAX
        if (self._arg("use_temp_loss", False) and not detach and self._arg("opt_pose", False) and not layer.use_cache
                and layer.N_kps <= ALL_FRAMES_MAX):
            frames = layer.all_frames()
            kps, bones, skts, _, rots = (t[kp_idx] for t in frames)
            extras["_frames"] = (frames[0].detach(), frames[1].detach(), frames[4].detach())
        else:
            kps, bones, skts, _, rots = layer(kp_idx)
        kp_args = self._create_kp_args_dict(kps=kps, skts=skts, bones=bones, cyls=batch["cyls"])
        extras["rots"] = rots
        if detach:
            kp_args = {k: kp_args[k].detach() for k in kp_args if kp_args[k] is not None}
            extras = {k: extras[k].detach() for k in extras if torch.is_tensor(extras[k])}
        return kp_args, extras

    def _create_kp_args_dict(self, kps, skts, bones=None, cyls=None, rots=None):
        return {"kp_batch": kps, "skts": skts, "bones": bones, "cyls": cyls}

    def _anchors(self):
        """The anchors of create_popt on the device, in the kernel's layout (rot6d: the [:3, :2] blocks, flattened)."""
        a = self.popt_kwargs["popt_anchors"]
        key = (id(a["kps"]), id(a.get("rots")), id(a.get("bones")))
        if self._anchor_dev is None or self._anchor_dev[0] != key:
            if self._arg("opt_rot6d", False):
                r = torch.as_tensor(a["rots"])
                table = r[..., :3, :2].reshape(r.shape[0], r.shape[1], 6)
            else:
                table = torch.as_tensor(a["bones"])
            self._anchor_dev = (key, _f32(table, self.device), _f32(torch.as_tensor(a["kps"]), self.device))
        return self._anchor_dev[1], self._anchor_dev[2]

    def _pose_spec(self, batch, kp_opts):
        """Trainer._compute_kp_loss's inputs (core/trainer.py:382-433) as anerf_pose_loss's constants."""
        rot6d = self._arg("opt_rot6d", False)
        anchor, anchor_kps = self._anchors()
        kp_idx = torch.as_tensor(batch["kp_idx"]).to(self.device, torch.long).reshape(-1)
        temporal = {}
        if self._arg("use_temp_loss", False):
            layer = self.popt_kwargs["popt_layer"]
            prev, nxt = temporal_neighbours(kp_idx, layer.N_kps)
            if "_frames" in kp_opts:
                kps_all, bones_all, rots_all = kp_opts["_frames"]
                cur_all = rots_all if rot6d else bones_all
                pk, pc, nk, nc = kps_all[prev], cur_all[prev], kps_all[nxt], cur_all[nxt]
            else:
                with torch.no_grad():
                    o_prev, o_next = layer(prev), layer(nxt)
                at = 4 if rot6d else 1
                pk, pc, nk, nc = o_prev[0], o_prev[at], o_next[0], o_next[at]
            temporal = dict(prev_cur=_f32(pc), next_cur=_f32(nc), prev_kps=_f32(pk), next_kps=_f32(nk),
                            temp_val=_f32(batch["temp_val"].reshape(-1), self.device),
                            temp_coef=self._arg("temp_coef", 0.05))
        return PoseSpec(anchor, anchor_kps, kp_idx, rot6d, self._arg("opt_pose_tol", 0.0),
                        self._arg("opt_pose_coef", 0.0), ext_scale=self._arg("ext_scale", 0.001), **temporal)

    def compute_loss(self, batch, preds, kp_opts=None, popt_detach=False):
        """core/trainer.py:319-351 on anerf_train_loss and anerf_pose_loss -> (loss_dict, stats): the reference's keys,
        0-d device tensors (views of the step's statistics buffer; total_loss carries the graph)."""
        if self._stats is None:
            self._stats = torch.empty(N_STATS, dtype=torch.float32, device=self.device)
        coarse = "rgb0" in preds
        reg = self.loss_spec.reg != _lib.ANERF_REG_NONE
        fgs = batch["fgs"][..., 0] if reg else None
        pose = cur = kps = None
        if not popt_detach:
            pose = self._pose_spec(batch, kp_opts)
            cur = kp_opts["rots"] if pose.rot6d else kp_opts["bones"]
            kps = kp_opts["kp_batch"]
        total, stats_buf = step_loss(self.loss_spec, preds["rgb_map"], preds["acc_map"], batch["target_s"],
                                     preds.get("rgb0"), preds.get("acc0"), batch.get("bgs"), fgs, pose, cur, kps,
                                     stats=self._stats)
        views = {}

        def stat(names, name, offset=0):
            k = offset + names.index(name)
            views[k] = stats_buf[k]
            return views[k]
        loss_dict, stats = {"rgb_loss": stat(LOSS_STATS, "rgb_loss")}, {"psnr": stat(LOSS_STATS, "psnr")}
        if reg:
            loss_dict["reg_loss"] = stat(LOSS_STATS, "reg_loss")
        if coarse:
            loss_dict["rgb_loss0"] = stat(LOSS_STATS, "rgb_loss0")
            stats["psnr0"] = stat(LOSS_STATS, "psnr0")
            if reg:
                loss_dict["reg_loss0"] = stat(LOSS_STATS, "reg_loss0")
        if pose is not None:
            nl = len(LOSS_STATS)
            loss_dict["kp_loss"] = stat(POSE_STATS, "kp_loss", nl)
            if pose.has_temporal:
                loss_dict["temp_loss"] = stat(POSE_STATS, "temp_loss", nl)
            stats["MPJPC"] = stat(POSE_STATS, "MPJPC", nl)
        loss_dict["total_loss"] = total
        self._stat_views = views
        return loss_dict, stats

    def _optim_step(self):
        """optimizer.step() + zero_grad() (set_to_none: mlp.py's deferred weight-gradient guard tests `grad is None`),
        -> the [total_norm, avg_norm] device view of the gradients the step used."""
        norms = self._stats[_NORM_AT:_NORM_AT + 2]
        if isinstance(self.optimizer, Adam):
            self.optimizer.norm_buffer = norms
            self.optimizer.step()
            if self.optimizer.last_grad_norm() is None:
                # no parameter took the kernel path (CPU parameters, or no gradient at all): nothing wrote the two
                # floats; the gradients are still there, the norms come from torch ops
                grad_norms([p for g in self.optimizer.param_groups for p in g["params"]], out=norms)
        else:
            grad_norms(self.render_kwargs_train["ray_caster"].parameters(), out=norms)
            self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)
        return norms

    def optimize(self, loss, i, popt_detach=False):
        """core/trainer.py:451-483: backward, the network's step, and every opt_pose_step-th call the pose layer's.
        Both branches report the norm of the gradients the step used (module docstring)."""
        if self._stats is None:
            self._stats = torch.empty(N_STATS, dtype=torch.float32, device=self.device)
        if popt_detach:
            loss.backward()
        else:
            cache = self._arg("opt_pose_cache", False)
            step = self._arg("opt_pose_step", 1)
            loss.backward(retain_graph=bool(cache and step > 1))
        norms = self._optim_step()
        if not popt_detach and i % self._arg("opt_pose_step", 1) == 0:
            if isinstance(self.pose_optimizer, Adam):
                self.pose_optimizer.norm_buffer = self._stats[_NORM_AT + 2:_NORM_AT + 4]
            self.pose_optimizer.step()
            self.pose_optimizer.zero_grad(set_to_none=True)
            if self._arg("opt_pose_cache", False):
                self.popt_kwargs["popt_layer"].update_cache()
        out = {}
        for k, name in enumerate(("total_norm", "avg_norm")):
            self._stat_views[_NORM_AT + k] = norms[k]
            out[name] = self._stat_views[_NORM_AT + k]
        return out

    # -- checkpoints
    def save_nerf(self, path, global_step):
        """core/trainer.py:485-506: the reference's checkpoint keys, CPU tensors."""
        ray_caster = self.render_kwargs_train["ray_caster"]
        popt_sd, poptim_sd, popt_anchors = None, None, None
        if self.popt_kwargs is not None:
            popt_sd = _cpu(self.popt_kwargs["popt_layer"].state_dict())
            poptim_sd = _cpu(self.pose_optimizer.state_dict())
            popt_anchors = _cpu(self.popt_kwargs["popt_anchors"])
        torch.save({"global_step": global_step, "optimizer_state_dict": _cpu(self.optimizer.state_dict()),
                    "poseopt_layer_state_dict": popt_sd, "pose_optimizer_state_dict": poptim_sd,
                    "poseopt_anchors": popt_anchors, **ray_caster.module.checkpoint()}, path)
        print("Saved checkpoints at", path)

    def evaluate_poses(self, gt_kps, idxs=None, **kw):
        """Score the pose layer's current joints against gt_kps [N_kps][J][3] on the device (posescore.
        evaluate_pose_layer: MPJPE, PA-MPJPE, PCK, AUC) -> PoseScores."""
        from .posescore import evaluate_pose_layer
        if self.popt_kwargs is None:
            raise ValueError("this Trainer optimises no poses (popt_kwargs is None)")
        return evaluate_pose_layer(self.popt_kwargs["popt_layer"], gt_kps, idxs=idxs, **kw)

    def save_popt(self, path, global_step):
        """core/trainer.py:508-516."""
        torch.save({"global_step": global_step,
                    "poseopt_layer_state_dict": _cpu(self.popt_kwargs["popt_layer"].state_dict()),
                    "poseopt_anchors": _cpu(self.popt_kwargs["popt_anchors"])}, path)
        print("Saved pose at", path)


def _cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu(v) for v in x)
    return x


def create_popt(args, data_attrs, ckpt=None, device=None):
    """core/pose_opt.py:14-83 without smplx -> (pose_optimizer, popt_kwargs): a kinematics.PoseOptLayer over the
    dataset's poses (kp3d, bones, rest_pose, betas; kp_map / kp_uidxs / rest_pose_idxs when present), this module's
    Adam over it (lr args.opt_pose_lrate) and the anchors of the pose loss {kps, bones, rots, beta}: the initial poses,
    a checkpoint's `poseopt_anchors`, or with --use_ckpt_anchor the checkpoint's optimised poses.  The layer and the
    optimizer reload from `ckpt` (or args.init_poseopt) unless args.no_poseopt_reload.  anchors['rots'] are the
    rotation matrices of the anchor bones (axisang_to_rot); with --use_ckpt_anchor on a --opt_rot6d layer, whose
    parameters are not axis-angle, they are the layer's own matrices."""
    skel_type = data_attrs["skel_type"]
    nj = len(skel_type.joint_names)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    rest_pose = torch.as_tensor(np.asarray(data_attrs["rest_pose"], np.float32)).reshape(-1, nj, 3)
    beta = torch.as_tensor(np.asarray(data_attrs["betas"])) if data_attrs.get("betas") is not None else None
    init_kps = torch.as_tensor(np.asarray(data_attrs["kp3d"], np.float32))
    init_bones = torch.as_tensor(np.asarray(data_attrs["bones"], np.float32))
    rot6d = bool(getattr(args, "opt_rot6d", False))
    layer = PoseOptLayer(init_kps.clone(), init_bones.clone(), rest_pose, skel_type=skel_type,
                         kp_map=data_attrs.get("kp_map"), kp_uidxs=data_attrs.get("kp_uidxs"),
                         rest_pose_idxs=data_attrs.get("rest_pose_idxs"),
                         use_cache=bool(getattr(args, "opt_pose_cache", False)), use_rot6d=rot6d, beta=beta, device=dev)
    params = list(layer.parameters())
    lr = getattr(args, "opt_pose_lrate", 5e-4)
    if dev.type == "cuda":
        pose_optimizer = Adam(params, lr=lr, betas=(0.9, 0.999))
    else:
        pose_optimizer = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999))
    anchor_kps, anchor_bones, anchor_beta, anchor_rots = init_kps, init_bones, beta, None
    init = getattr(args, "init_poseopt", None)
    if (ckpt is not None or init is not None) and not getattr(args, "no_poseopt_reload", False):
        pose_ckpt = torch.load(init, map_location="cpu", weights_only=True) if init is not None else ckpt
        layer.load_state_dict(pose_ckpt["poseopt_layer_state_dict"])
        pose_optimizer.load_state_dict(pose_ckpt["pose_optimizer_state_dict"])
        if pose_ckpt.get("poseopt_anchors") is not None:
            a = pose_ckpt["poseopt_anchors"]
            anchor_kps, anchor_bones, anchor_beta = a["kps"], a["bones"], a.get("beta")
            # (the matrices the checkpointed run regularised against, where it saved them: a resumed run then continues
            # on the same anchors bit for bit; the reference always recomputes them from the bones)
            anchor_rots = a.get("rots")
        if getattr(args, "use_ckpt_anchor", False):
            with torch.no_grad():
                kps, bones, _, _, rots = layer.calculate_kinematic(np.arange(layer.N_kps))
            anchor_kps, anchor_bones = kps.cpu().clone(), bones.cpu().clone()
            anchor_rots = rots.cpu().clone() if rot6d else None
            anchor_beta = layer.beta
    if anchor_rots is None:
        with torch.no_grad():  # (axisang_to_rot of the anchor bones: the chain's own rotations)
            anchor_rots = pose_kinematics(torch.as_tensor(anchor_bones).float(), rest_pose[:1], skel_type, device=dev,
                                          outputs=("rots",))["rots"].cpu()
    popt_anchors = {"kps": torch.as_tensor(anchor_kps), "bones": torch.as_tensor(anchor_bones),
                    "rots": anchor_rots, "beta": anchor_beta}
    if layer.use_cache:
        layer.update_cache()
    pose_optimizer.zero_grad()
    return pose_optimizer, {"popt_anchors": popt_anchors, "popt_layer": layer, "skel_type": skel_type}


__all__ = ["Adam", "Trainer", "create_popt", "LossSpec", "PoseSpec", "step_loss", "train_loss_forward",
           "train_loss_backward", "pose_loss_forward", "pose_loss_backward", "grad_norms", "decay_optimizer_lrate",
           "temporal_neighbours", "nerf_loss_reference", "pose_loss_reference", "adam_reference", "LOSS_STATS",
           "POSE_STATS"]

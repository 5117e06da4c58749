"""The training stages' kernels (csrc/anerf_train.hpp) one by one against float64 restatements
(tests/_stage_ref.py, pinned on the CPU by tests/test_train_stages_host.py): train_z_kernel, train_encode_kernel,
train_encode_backward_kernel (its eight instances and encode_row_grad_joint_staged), train_composite_kernel and
train_composite_backward_kernel (all five upstream gradients, alone and together), through train._Encode,
train._Composite and the C entry points.  Inputs, normalisations and bounds: tests/_stage_cases.py.

Normalised errors and their bounds.  Every bound is 8 x the largest error of the SAME restatement run in float32 on the
CPU against the float64 one, over the same cases (the formulas' own float32 rounding; the factor is for another, equally
valid order of float32 operations: fma contraction, the slot-order reduction, the atomics), floor 1e-6:

  family              float32 restatement   bound     normalised by
  samples             8.5e-8                1.0e-6    max |z| (the floor)
  encode forward      1.55e-6               1.3e-5    the column's gain 2^k (2 / c) + tau / 4 (d feature / d argument)
  encode backward     3.75e-7               3.0e-6    per (pose, joint): sum over samples and features of
                                                      |g dfeature / dskts| x the feature's gain
  composite forward   3.70e-7               3.0e-6    max |output|
  composite backward  1.62e-6               1.3e-5    per ray: sum_k |G|_k |dw_k / dx_s| + |g_alpha dalpha / dx| (max over s)

Measured on the device (MI355X; every test prints its figure): samples 8.5e-8, encode forward 1.38e-6, encode
backward 3.3e-7 (accumulating into a filled buffer 4.2e-8; the dist = 0 joint's own block 4.2e-8 of its maximum,
1.5e12), composite forward 5.1e-7, composite backward 1.62e-6: all within the restatement's own float32 error or a
small multiple of it, none above 1e-4.

Why the encoder's scales carry a gain (a finding of writing this test, _stage_cases.enc_reference): normalised by the
plain per-sample absolute sum the float32 restatement itself is off by 2.3e-3 on these cases (multires 10 with
--cutoff_shift: cancellation among a sample's twenty terms of size 2^k |g|, and the distance's float32 rounding, 5e-7,
times the top frequency 2300; the host test prints the figure), and by the unweighted per-feature sum still by 2.5e-4.  Both are
properties of float32, not of a kernel; with the gain in the scale a normalised error is in units of the argument's
rounding for every configuration.  One kernel defect showed up: ray_angle's fminf / fmaxf clamp turned the NaN of an
out-of-range pose index into a finite angle (test_encode_forward_and_backward[s_relpos_angle_mrb2_cb-N5-S12-pmixed]
caught the finite column in a NaN row; torch.clamp keeps NaN, and so does the kernel now).  With querypts the kp columns are
written from the world point alone and stayed finite in such a row; anerf.h promises NaN features, so
train_encode_kernel now makes the point NaN too (the s_query_shift mixed-pose case holds it).  test_train_stages_host shows that severing any single
term of the backward moves the reference by at least 100 x these bounds on batches this module runs.
"""
import importlib

import numpy as np
import pytest
import torch

import _stage_cases as sc
import _stage_ref as ref

pytestmark = pytest.mark.gpu

train = importlib.import_module("a-nerf_amd.train")
model_mod = importlib.import_module("a-nerf_amd.model")
_lib = importlib.import_module("a-nerf_amd._lib")

EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_MODELS = {}


def _enc_model(name, n_joints=24):
    """The encoder constants as TrainRayCaster._constants() builds them (cached per configuration)."""
    key = ("enc", name, n_joints)
    if key not in _MODELS:
        cfg, ckpt, _, vw = sc.enc_config(name, n_joints)
        _MODELS[key] = model_mod.DeviceModel(cfg, ckpt, device=0, view_windows=vw)
    return _MODELS[key]


def _comp_model(model):
    key = ("comp", model)
    if key not in _MODELS:
        cfg, ckpt = sc.comp_config(model)
        _MODELS[key] = model_mod.DeviceModel(cfg, ckpt, device=0)
    return _MODELS[key]


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(x, dtype=dtype).cuda().contiguous()


def _report(what, fam, err):
    bound = sc.BOUNDS[fam]
    print(f"{what}: {fam} error {err:.3e}; the float32 restatement's {sc.F32_ERR[fam]:.2e}; bound {bound:.1e}")
    assert err <= bound, f"{what}: {fam} {err:.3e} > {bound:.1e}"


# ----------------------------------------------------------------------------- samples
def _samples(near, far, S, t, lindisp):
    n = len(near)
    nr, fr, tr = _dev(near), _dev(far), _dev(t)
    z = torch.full((n, S), -7.0, device="cuda")
    _lib.check(_lib.load().anerf_train_samples(_lib.ptr(nr), _lib.ptr(fr), n, S, _lib.ptr(tr),
                                               _lib.ANERF_FLAG_LINDISP if lindisp else 0, _lib.ptr(z),
                                               _lib.stream_handle()), "anerf_train_samples")
    torch.cuda.synchronize()
    return z.cpu()


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("S", sc.SAMPLE_S)
def test_samples(S, lindisp):
    got = {}
    for kind in sc.SAMPLE_T:
        near, far, t = sc.sample_case(S, kind)
        got[kind] = _samples(near, far, S, t, lindisp)
        _report(f"S {S} lindisp {lindisp} t_rand {kind}", "samples",
                sc.rel_error(got[kind], ref.samples(near, far, S, t, lindisp)))
    det = got["none"]
    mids = 0.5 * (det[:, 1:] + det[:, :-1])
    # the first interval's lower end is z_0, the last one's upper end z_{S-1}
    assert torch.equal(got["zeros"][:, 0], det[:, 0])
    assert bool((got["ones"][:, -1] <= det[:, -1]).all())
    tol = 1e-6 * float(det.abs().max())
    assert float((got["ones"][:, -1] - det[:, -1]).abs().max()) <= tol
    assert float((got["zeros"][:, 1:] - mids).abs().max()) <= tol
    assert float((got["ones"][:, :-1] - mids).abs().max()) <= tol
    r = got["random"]
    assert bool((r[:, 0] >= det[:, 0]).all()) and bool((r[:, -1] <= det[:, -1]).all())


# ----------------------------------------------------------------------------- encoder
def _encode(b, start=None):
    """Features [N, S, F] and dL/dskts for the batch's g_feat through train._Encode (start None), or through the C
    entry with grad_skts pre-filled with `start` (the documented accumulation)."""
    m = _enc_model(b["name"], b["cfg"].n_joints)
    N, S = b["z"].shape
    rb, z, g = _dev(b["rb"]), _dev(b["z"]), _dev(b["g_feat"])
    pose, pn = _dev(b["ray_pose"], torch.int32), _dev(b["pts_noise"])
    skts = _dev(b["skts"]).requires_grad_(True)
    feat = train._Encode.apply(skts, m, rb, z, pose, pn)
    assert feat.shape == (N * S, sc.feat_dim(b["cfg"], b["vw"]))
    if start is None:
        feat.backward(g.reshape(N * S, -1))
        grad = skts.grad
    else:
        grad = torch.full_like(skts, start)
        _lib.check(_lib.load().anerf_train_encode_backward(
            m.handle, _lib.ptr(rb), rb.shape[1], N, _lib.ptr(z), S, _lib.ptr(skts), skts.shape[0], _lib.ptr(pose),
            _lib.ptr(pn), _lib.ptr(g), _lib.ptr(grad), _lib.stream_handle()), "anerf_train_encode_backward")
    torch.cuda.synchronize()
    return feat.detach().reshape(N, S, -1).cpu(), grad.detach().cpu()


def _check_encode(b, what):
    f64, g64, scale = sc.enc_reference(b)
    feat, grad = _encode(b)
    _report(what, "encode_forward", sc.feature_error(feat, f64, sc.column_gain(b["cfg"], b["st"], b["vw"])))
    _report(what, "encode_backward", sc.block_error(grad, g64, scale))
    assert bool((grad[:, :, 3, :] == 0).all()), "row 3 of a transform has a gradient"
    return feat, grad, (f64, g64, scale)


@pytest.mark.parametrize("kw", sc.encode_cases(), ids=sc.case_id)
def test_encode_forward_and_backward(kw):
    """Every instance of the backward kernel, the staged function, every option, the layout edges
    (spb = 256 // nj sample slots against ns), the pose forms, pts_noise and the ray angle's clamp."""
    b = sc.enc_batch(**kw)
    feat, grad, _ = _check_encode(b, sc.case_id(kw))
    if b["ray_pose"] is not None:
        bad = (b["ray_pose"] < 0) | (b["ray_pose"] >= b["n_poses"])
        assert bool(torch.isnan(feat[bad]).all()) and bool(torch.isfinite(feat[~bad]).all())


def test_out_of_range_pose_indices_contribute_nothing():
    """Rays with index -1 and n_poses: NaN rows, every other row and the gradients as in the run without them (two
    rays share pose 0: a + b is the same in either order, so bit for bit)."""
    b = sc.enc_batch("i7_4", 5, 12, pose_form="mixed")
    feat, grad = _encode(b)
    keep = np.flatnonzero((b["ray_pose"] >= 0) & (b["ray_pose"] < b["n_poses"]))
    assert keep.tolist() == [0, 2, 4]
    sub = dict(b, rb=b["rb"][keep], z=b["z"][keep], ray_pose=b["ray_pose"][keep], g_feat=b["g_feat"][keep])
    feat_s, grad_s = _encode(sub)
    assert torch.equal(feat[keep], feat_s)
    assert torch.equal(grad, grad_s)
    assert bool((grad[1] == 0).all()), "the pose no ray uses has a gradient"


def test_encode_backward_accumulates_into_grad_skts():
    b = sc.enc_batch("i7_4", 5, 12, pose_form="mixed")
    _, g64, scale = sc.enc_reference(b)
    start = 0.25
    _, grad = _encode(b, start=start)
    assert bool((grad[:, :, 3, :] == start).all()) and bool((grad[1] == start).all())
    # (the sum start + v rounds once more: half an ulp of the larger of the two, against the block's scale)
    extra = float((2.0 ** -24 * (start + g64.abs().amax((-1, -2))) / scale.clamp_min(1e-30))[scale > 0].max())
    err = sc.block_error(grad - start, g64, scale)
    print(f"accumulate: encode_backward error {err:.3e} (bound {sc.BOUNDS['encode_backward']:.1e} + {extra:.1e})")
    assert err <= sc.BOUNDS["encode_backward"] + extra


def test_sample_exactly_on_a_joint():
    """dist = 0: the eps branches give g / 1e-12; compared on its own, block by block."""
    b = sc.dist0_batch()
    feat, grad, (f64, g64, scale) = _check_encode(b, "dist0")
    blk = g64[0, 0, :3]
    assert float(blk.abs().max()) > 1e11 and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(feat).all())
    rel = float(((grad[0, 0, :3].double() - blk).abs() / blk.abs().max()).max())
    print(f"dist0: the joint's own block, max |device - reference| / max |reference| = {rel:.3e}")
    assert rel <= sc.BOUNDS["encode_backward"]


# ----------------------------------------------------------------------------- composite
def _composite(b):
    m = _comp_model(b["model"])
    raw = _dev(b["raw"]).requires_grad_(True)
    outs = train._Composite.apply(raw, m, _dev(b["z"]), _dev(b["rb"]), _dev(b["noise"]))
    return raw, dict(zip(ref.COMPOSITE_OUTPUTS, outs))


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("ns", sc.COMP_NS)
@pytest.mark.parametrize("model", list(sc.COMP_MODELS))
def test_composite_forward_and_backward(model, ns, noise):
    b = sc.comp_batch(model, ns, noise)
    raw, outs = _composite(b)
    what = f"{model} ns {ns} noise {noise}"
    o64 = None
    for which in sc.WHICH:
        o64, g64, scale = sc.comp_reference(b, which)
        g, = torch.autograd.grad([outs[k] for k in which], raw, [_dev(b["g"][k]) for k in which], retain_graph=True)
        torch.cuda.synchronize()
        g = g.cpu()
        assert bool(torch.isfinite(g).all())
        _report(f"{what} g on {'+'.join(which)}", "composite_backward", sc.ray_error(g, g64, scale))
        if b["cfg"].density_type == "relu":
            assert bool((g[sc.EMPTY, :, 3] == 0).all()), "the empty ray's density gradient is not exactly 0"
    for k in ref.COMPOSITE_OUTPUTS:
        _report(f"{what} {k}", "composite_forward", sc.rel_error(outs[k].detach().cpu(), o64[k]))
    if b["cfg"].density_type == "relu":
        assert float(outs["acc"][sc.EMPTY].detach()) == 0 and float(outs["disp"][sc.EMPTY].detach()) == 0
    assert float(outs["acc"][sc.OPAQUE].detach()) == 1 and float(outs["acc"][sc.LAST].detach()) == 1
    assert float(outs["weights"][sc.LAST, -1].detach()) == 1


def _composite_direct(m, b, ns, which, fill=None):
    """The C entries with NULL for the upstream gradients not in `which`."""
    lib = _lib.load()
    N = b["z"].shape[0]
    raw, z, rb, nz = _dev(b["raw"]), _dev(b["z"]), _dev(b["rb"]), _dev(b["noise"])
    f = lambda *s: torch.full(s, -7.0, device="cuda")  # noqa: E731
    rgb, disp, acc, w, a, tr, g_raw = f(N, 3), f(N), f(N), f(N, ns), f(N, ns), f(N, ns), f(N, ns, 4)
    rc_f = lib.anerf_train_composite(m.handle, _lib.ptr(raw), _lib.ptr(z), _lib.ptr(rb), rb.shape[1], N, ns,
                                     _lib.ptr(nz), _lib.ptr(rgb), _lib.ptr(disp), _lib.ptr(acc), _lib.ptr(w),
                                     _lib.ptr(a), _lib.ptr(tr), _lib.stream_handle())
    msg_f = lib.anerf_last_error().decode() if rc_f else ""
    gs = [_dev(b["g"][k]) if k in which else None for k in ref.COMPOSITE_OUTPUTS]
    rc_b = lib.anerf_train_composite_backward(m.handle, _lib.ptr(raw), _lib.ptr(z), _lib.ptr(rb), rb.shape[1], N, ns,
                                              _lib.ptr(nz), _lib.ptr(w), _lib.ptr(a), _lib.ptr(tr),
                                              *[_lib.ptr(x) for x in gs], _lib.ptr(g_raw), _lib.stream_handle())
    msg_b = lib.anerf_last_error().decode() if rc_b else ""
    torch.cuda.synchronize()
    return (rc_f, msg_f, [rgb, disp, acc, w, a, tr]), (rc_b, msg_b, g_raw)


def test_composite_backward_null_gradients_equal_zero_gradients():
    """Autograd hands the kernel zero tensors for the outputs without a gradient; the C entry also takes NULL."""
    b = sc.comp_batch("relu", 65, noise=True)
    raw, outs = _composite(b)
    for which in sc.WHICH:
        g, = torch.autograd.grad([outs[k] for k in which], raw, [_dev(b["g"][k]) for k in which], retain_graph=True)
        (rc_f, _, fw), (rc_b, _, g_raw) = _composite_direct(_comp_model("relu"), b, 65, which)
        assert rc_f == 0 and rc_b == 0
        assert torch.equal(g_raw, g), which
        for x, k in zip(fw, ref.COMPOSITE_OUTPUTS):
            assert torch.equal(x, outs[k].detach()), k


@pytest.mark.parametrize("ns,why", [(1025, "more than 1024 samples"), (1821, "bytes of LDS"), (2341, "bytes of LDS")])
def test_composite_refuses_a_sample_count_the_backward_cannot_hold(ns, why):
    """Both entries, before any launch: the return code, the message, and the sentinel-filled outputs untouched."""
    rng = np.random.default_rng(ns)
    b = dict(raw=rng.normal(size=(1, ns, 4)), z=np.sort(rng.uniform(1, 3, (1, ns))), rb=sc.comp_batch("relu", 2)["rb"][:1],
             noise=None, g={k: rng.normal(size=s) for k, s in zip(ref.COMPOSITE_OUTPUTS,
                                                                  ((1, 3), (1,), (1,), (1, ns), (1, ns)))})
    (rc_f, msg_f, fw), (rc_b, msg_b, g_raw) = _composite_direct(_comp_model("relu"), b, ns, ref.COMPOSITE_OUTPUTS)
    assert rc_f == EINVAL and "anerf_train_composite:" in msg_f and why in msg_f, (rc_f, msg_f)
    assert rc_b == EINVAL and "anerf_train_composite_backward:" in msg_b and why in msg_b, (rc_b, msg_b)
    assert all(bool((x == -7.0).all()) for x in fw + [g_raw]), "written before the check"


def test_composite_largest_accepted_sample_count_runs_both_ways():
    ns = 1024
    rng = np.random.default_rng(ns)
    b = dict(raw=rng.normal(size=(2, ns, 4)), z=np.sort(rng.uniform(1, 3, (2, ns))), rb=sc.comp_batch("relu", 2)["rb"][:2],
             noise=None, g={k: rng.normal(size=s) for k, s in zip(ref.COMPOSITE_OUTPUTS,
                                                                  ((2, 3), (2,), (2,), (2, ns), (2, ns)))})
    (rc_f, _, fw), (rc_b, _, g_raw) = _composite_direct(_comp_model("relu"), b, ns, ref.COMPOSITE_OUTPUTS)
    assert rc_f == 0 and rc_b == 0
    assert all(bool(torch.isfinite(x).all()) and bool((x != -7.0).all()) for x in fw + [g_raw])

"""GPU: the render kernels' MLP (mlp_trunk, mlp_layer, mlp_layer_x3, mlp_layer_x6, mlp_layer_h3 of csrc/anerf_mlp.hpp)
held to a float64 reference in every precision mode, through each kernel that runs it:

  radiance_kernel      RayCaster.render_pts_radiance, all four raw columns, coarse and fine net
  density_kernel       RayCaster.render_pts_density (the alpha head in its own k-order), coarse and fine net; sigma also
                       equals the radiance entry's column 3 under test_gpu_mesh_attrs' raw bar (1e-4 + 1e-5 |ref|)
  render_kernel        render_rays(debug=True, near_far_given=True): 12 rays through the body (12: no multiple of the 4
                       rays a workgroup takes), S = 33, I = 31; last_debug's raw_coarse at z_coarse and raw_fine at the
                       device's own z_fine, which is fed to the reference as input (so hazard H11 does not enter).  The
                       only path through compute_view_factor / view_dir_part; the dead-block skip is off under debug
                       (test_gpu_dead_blocks ties it to this path bit for bit)
  render_fused_kernel  the same for one single_net model

Criterion (tests/_mlp_ref.py check(); tests/test_render_mlp_host.py shows what it can see): per case, output column and
point class, E = RMS(out - ref64) <= 4 max(E32, Eemu(mode)) for fp32, bf16x6, fp16x4, fp16x3 and <= 4 Eemu for bf16x3,
and every element within 16 x that bound.  E32: the float32 restatement's error on the same inputs; Eemu: that of the
float64 emulation of the mode's documented operand formats.  The factor 4 pays for summation order and is not tuned;
every single-layer plane-loss mutant sits at >= 32 x the bound on the `he` checkpoints.  The reference and the
emulations are computed once per case and shared by the modes.  Every test prints E_gpu / E32 per class and column.

The `w256_init` case (torch's default init, the weights of every other checkpoint in the suite) is printed and not
asserted: its layers contract, so it cannot see an early layer's error (test_render_mlp_host.py pins that), and its
bounds say nothing about what the `he` cases do not already say.

`w256_he_negbias`: the "far" class (86 points beyond every cutoff: every window exactly zero, the bone directions the
only live inputs) is judged on its own like every class, and every output is finite.  The bone directions are not
windowed, so no hidden row is all zero there; `w256_he_dead` (the same with the bone-direction weight columns zeroed)
has exactly-zero hidden rows beyond the cutoffs -- the fp16 modes' per-sample scale of a zero maximum -- next to rows
whose maxima span 7e-7 .. 1.8 in the same blocks; its reference there is the biases' alone (_dead_far).

Measured on an MI355X: largest E_gpu / E32 over classes, columns and both nets, (largest E_gpu / bound; < 1 passes).
The full table, every case, is in DESIGN §5.
                              fp32          bf16x3        bf16x6        fp16x3        fp16x4
  radiance w256_he            2.15 (0.54)   26.3 (0.29)   2.05 (0.51)   1.96 (0.49)   1.86 (0.46)
  radiance w256_he_tails      2.26 (0.57)   24.8 (0.27)   2.21 (0.55)   2.13 (0.53)   2.25 (0.56)
  radiance w256_j65 (worst)   2.52 (0.63)   30.7 (0.29)   2.50 (0.62)   2.47 (0.62)   2.43 (0.61)
  radiance w256_he_dead       1.84 (0.46)   11.3 (0.45)   1.83 (0.46)   2.30 (0.57)   2.27 (0.57)
  density  w256_he            1.54 (0.38)   26.3 (0.29)   1.59 (0.40)   1.25 (0.31)   1.32 (0.33)
  render   w256_he            1.81 (0.45)   24.5 (0.27)   1.74 (0.44)   1.57 (0.39)   1.61 (0.40)
  render   w64_d4             1.51 (0.38)   32.8 (0.27)   1.56 (0.39)   1.59 (0.40)   1.66 (0.41)
  fused    w256_single        1.46 (0.36)   23.8 (0.28)   1.44 (0.36)   1.26 (0.32)   1.28 (0.32)
Every other case lies between these; the largest single element is 0.22 of its 16 x guard; density's sigma equals the
radiance entry's column 3 bit for bit.  A library built with the low fp16 plane of one hidden layer's weights zeroed
(layer 2, coarse net) measured 42-51 x the bound here, where the host emulation of that mutant predicts 40-80 x.
"""
import importlib

import numpy as np
import pytest
import torch

import _mlp_cases as C
import _mlp_ref as M

pytestmark = pytest.mark.gpu

anerf = importlib.import_module("a-nerf_amd")

NETS = [("coarse", False), ("fine", True)]


@pytest.fixture(scope="module", autouse=True)
def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


_casters = {}


def _caster(c, mode):
    """One RayCaster per (case, mode), shared by the tests of this module."""
    k = (c.name, mode)
    if k not in _casters:
        _casters[k] = anerf.RayCaster(c.with_precision(mode), c.ckpt)
    return _casters[k]


def _pose(c):
    return _t(c.kps[None]), _t(c.skts[None]), None


def _dead_far(c, ev, mode, out, cols, what):
    """`w256_he_dead`, the points beyond every cutoff: every hidden row is exactly zero and the output is the biases'
    alone, one row for all 86 points.  The RMS over such a class is the rounding of a single number and carries no
    statistics, so the class is judged element by element instead: the same row at every point, sigma the alpha bias
    exactly, rgb within the bound on E of the class "all" (16 x tighter than that class's element guard)."""
    far = ev["classes"] == "far"
    cols = list(cols)
    assert far.sum() == 86 and np.isfinite(out[far]).all()
    assert (out[far] == out[far][0]).all(), what
    b = M.bounds(mode, ev["ref"], ev["y32"], c.emu(ev, mode), ev["classes"])["all"][cols]
    d = np.abs(out[far][0].astype(np.float64) - ev["ref"][far][0][cols])
    print(f"{what} [far: one bias-only row] |gpu - ref64| " + " ".join(f"{x:.1e}" for x in d) + " | bound of all "
          + " ".join(f"{x:.1e}" for x in b))
    assert (d <= b).all(), what
    if 3 in cols:
        assert out[far][0][cols.index(3)] == np.float32(ev["net"].p["alpha_linear.bias"][0]), what


def _radiance(c, mode, net):
    raw = _caster(c, mode).render_pts_radiance(_t(c.pts), _t(c.dirs), *_pose(c), cams=c.cam, network=net)
    assert tuple(raw.shape) == (C.N_POINTS, 4) and raw.dtype == torch.float32
    return raw.cpu().numpy()


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", C.POINT_CASES)
def test_radiance_kernel(name, mode):
    c = C.case(name)
    for net, fine in NETS:
        ev = c.evaluate(fine=fine)
        raw = _radiance(c, mode, net)
        assert np.isfinite(raw).all()
        dead = c.kind == "he_dead"
        M.check(raw, mode, ev["ref"], ev["y32"], c.emu(ev, mode), ev["classes"], f"radiance {name} {mode} {net}",
                assert_it=c.asserted, skip=("far",) if dead else ())
        if dead:
            _dead_far(c, ev, mode, raw, (0, 1, 2, 3), f"radiance {name} {mode} {net}")


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", C.POINT_CASES)
def test_density_kernel(name, mode):
    c = C.case(name)
    for net, fine in NETS:
        ev = c.evaluate(fine=fine)
        sig = _caster(c, mode).render_pts_density(_t(c.pts), *_pose(c), network=net)
        assert tuple(sig.shape) == (C.N_POINTS, 1)
        sig = sig.cpu().numpy().astype(np.float64)
        dead = c.kind == "he_dead"
        M.check(sig, mode, ev["ref"], ev["y32"], c.emu(ev, mode), ev["classes"], f"density {name} {mode} {net}",
                assert_it=c.asserted, cols=(3,), skip=("far",) if dead else ())
        if dead:
            _dead_far(c, ev, mode, sig.astype(np.float32), (3,), f"density {name} {mode} {net}")
        rad = _radiance(c, mode, net)[:, 3:].astype(np.float64)
        d = np.abs(sig - rad)
        print(f"density {name} {mode} {net}: max |density - radiance sigma| {d.max():.3e}")
        assert (d - (1e-4 + 1e-5 * np.abs(rad))).max() <= 0


def _render_debug(c, mode):
    rb = c.rays()
    n = rb.shape[0]
    cyls = anerf.rays.valid_pixels(c.scene["c2ws"], 128, 128, c.scene["focal"], kps=c.scene["kps"], ext_scale=0.001)[1]
    rc = _caster(c, mode)
    rc.render_rays(_t(rb).cuda(), 33, skts=_t(c.skts[None]).cuda().expand(n, -1, -1, -1),
                   cyls=_t(cyls[0:1]).cuda().expand(n, -1), N_importance=31, chunk=4096, debug=True,
                   near_far_given=True)
    torch.cuda.synchronize()
    return rb, {k: v.cpu().numpy() for k, v in rc.last_debug.items()}


def _check_rays(c, mode):
    rb, dbg = _render_debug(c, mode)
    assert dbg["raw_coarse"].shape == (12, 33, 4) and dbg["raw_fine"].shape == (12, 64, 4)
    np.testing.assert_array_equal(dbg["near"], rb[:, 6])
    np.testing.assert_array_equal(dbg["far"], rb[:, 7])
    zf = dbg["z_fine"]
    assert np.isfinite(zf).all() and (np.diff(zf, axis=1) >= 0).all()
    # coarse: z_coarse does not depend on the mode, so its reference is shared; fine: the device's own z_fine
    for what, z, raw, fine, key in (("coarse", dbg["z_coarse"], dbg["raw_coarse"], False, "rays_coarse"),
                                    ("fine", zf, dbg["raw_fine"], True, f"rays_fine_{mode}")):
        if key == "rays_coarse" and (key, fine) in c._ev:
            np.testing.assert_array_equal(z, c._ev[(key, fine)]["z"])
        p, d = C.sample_points(rb, z)
        ev = c.evaluate(p, d, fine=fine, key=key)
        ev["z"] = z
        M.check(raw.reshape(-1, 4), mode, ev["ref"], ev["y32"], c.emu(ev, mode), ev["classes"],
                f"render {c.name} {mode} {what}")


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", C.RAY_CASES)
def test_render_kernel(name, mode):
    _check_rays(C.case(name), mode)


@pytest.mark.parametrize("mode", M.MODES)
def test_render_fused_kernel(mode):
    c = C.case("w256_single")
    assert c.cfg.single_net
    _check_rays(c, mode)

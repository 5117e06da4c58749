"""Host side of the render MLP's float64 criterion (tests/_mlp_ref.py, tests/_mlp_cases.py; the GPU side is
tests/test_gpu_render_mlp.py).  No device code runs here.

Why the criterion exists.  Every raw-output check of the suite is 1e-4 absolute, and every checkpoint it renders has
torch's default init, whose layers contract: on the `w256_init` case an operand that loses its low fp16 plane (11 of
22 bits) in any of trunk layers 0-4 moves the outputs by 0.3-1.1 x the bound below (fp16x3 / fp16x4; the bound is ~4
float32 evaluation errors, ~6e-8 absolute), the skip layer's h part by 2.2-2.4 x; only the x part of the skip layer and
layers 6-7 show (31-49 x).  A render kernel that silently drops half the operand bits of an early hidden layer
passes a suite built on such weights.  test_init_hides_the_early_layers pins that finding: of the 68 trunk-layer
mutants of the four split modes, 25 reach 10 x the bound.

What the tests use instead: the same checkpoints with the variance-preserving gain (x sqrt(6): `he`, `he_tails`,
`he_negbias`, _mlp_cases.py).  Measured here, float32 features and float32 torch CPU evaluation against float64:
  E32 (RMS over 515 points)      1.1e-7 .. 1.3e-7 per output column on `w256_he` (outputs of order 1)
  Eemu / E32, fp32-accurate modes 0.11 .. 1.00 over every case, class and column (asserted <= 2): the emulation rounds
                                 operands and sums exactly, so it sits below a float32 evaluation
  Eemu(bf16x3) / E32             7 .. 15 over all points of the W 256 `he` cases, 0.6 .. 44 over every case and class
                                 (reported)
  mutants, `he` and `he_tails`   fp16x4 / fp16x3: 49 .. 165 x the bound (smallest: layer 4); bf16x3: 32 .. 132 x;
                                 bf16x6 (see below): 434 .. 2,900 x.  Every (layer, operand) pair of every mode is
                                 >= 10 x the bound (asserted); the alpha head's on sigma, the view layer's on rgb.
                                 No pair is listed as invisible.
  element guard                  the float32 restatement's largest element error is at most 0.16 of 16 x 4 E32 (asserted
                                 <= 1)

The criterion (M.check): per case, output column and point class, E = RMS(out - ref64) <= 4 max(E32, Eemu(mode))
(bf16x3: 4 Eemu), every element within 16 x that bound.  The smallest mutant ratio is 32.6 x the bound, i.e. 130 x
max(E32, Eemu), so the factor 4 is below 1/8 of it (16.3); test_mutants_are_visible asserts that.

bf16x6's mutant.  Its operands have three planes.  Losing the third alone leaves 16 bits -- what bf16x3 computes with,
"within 1e-4 but not fp32-accurate"  -- and moves the outputs by 0.4-1.6 x the bound (weights) and 1.7-4.8 x
(activations): 2^-17 per operand against a bound of 4 float32 errors cannot reach 10 x by any choice of inputs.  So
the asserted bf16x6 mutant loses both planes below the first (8 bits remain: half the operand bits and more, the
analogue of the two-plane modes' mutant); the third-plane figures are printed by test_mutants_are_visible, not
asserted.

mlp.nerf_forward (the training MLP) runs on the device's GEMMs only, so the float32 restatement is not compared with
it here.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import oracle  # noqa: E402
import _mlp_cases as C  # noqa: E402
import _mlp_ref as M  # noqa: E402
from _golden import Golden  # noqa: E402

SPLIT = M.MODES[1:]


def _raw_close(a, ref, what):
    """test_gpu_parity._raw_close: 1e-4 absolute plus 1e-5 of the element."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    d = np.abs(a - ref)
    print(f"{what}: max |float64 restatement - reference| {d.max():.3e}")
    assert (d - (1e-4 + 1e-5 * np.abs(ref))).max() <= 0, what


@pytest.mark.parametrize("name,fine", [("c3_512_s64i128_d8w256", False), ("c3_512_s64i128_d8w256", True),
                                       ("v1_mr10_w64_d4", False), ("fc_64_s32i32_d4w128", False)])
def test_reference_matches_the_goldens_and_the_oracle(name, fine):
    """The float64 feature rows and MLP against the reference's own stage dump (stage_raw: D 8 with the skip layer,
    coarse and fine; D 4; the framecode model, one code per ray) and against the C oracle on the same points."""
    g = Golden(name)
    z = g["stage_z_all"] if fine else g["stage_z"]
    want = g["stage_raw_f"] if fine else g["stage_raw"]
    rb = g.ray_batch()[:4]
    om = oracle.OracleModel(g.cfg, g.ckpt)
    codes = g.ckpt["network_fn_state_dict"].get("framecodes.codes.weight")
    for r in range(4):
        p, d = C.sample_points(rb[r:r + 1], z[r:r + 1])
        cam = int(g["cams"][r]) if g.has("cams") else None
        net = M.Net(g.cfg, g.ckpt, fine=fine, cam=cam)
        with torch.no_grad():
            raw = net.forward(M.features(g.cfg, g.ckpt, g["skts"][0], p, d)).numpy()
        _raw_close(raw, want[r], f"{name} fine={fine} ray {r} vs stage dump")
        code = None if cam is None else np.tile(np.asarray(codes, np.float32)[cam], (len(p), 1))
        _raw_close(raw, om.network(om.encode(g["skts"][0], p, d), fine=fine, code=code),
                   f"{name} fine={fine} ray {r} vs oracle")


@pytest.mark.parametrize("name", list(C.INSTANCES))
def test_emulations_are_fp32_accurate(name):
    """Eemu(mode) <= 2 E32 for the four fp32-accurate modes, per class and column; Eemu(bf16x3) reported; the float32
    restatement itself meets the criterion's element guard."""
    c = C.case(name)
    for fine in (False, True):
        ev = c.evaluate(fine=fine)
        ref, y32 = ev["ref"], ev["y32"]
        assert np.isfinite(ref).all() and np.isfinite(y32).all()
        for cl, m in M.class_masks(ev["classes"]).items():
            e32 = M.rms(y32 - ref, m)
            el = np.abs(y32 - ref)[m].max(0)
            print(f"{name} fine={fine} [{cl}, {int(m.sum())}] E32 " + " ".join(f"{x:.2e}" for x in e32)
                  + " | max element / (16 x 4 E32) " + " ".join(f"{x:.3f}" for x in el / np.maximum(64 * e32, 1e-300)))
            assert (el <= M.ELEMENT * M.FACTOR * e32).all(), (name, cl)
            for mode in M.MODES:
                eemu = M.rms(c.emu(ev, mode) - ref, m)
                r = np.where(e32 > 0, eemu / np.where(e32 > 0, e32, 1), 0)  # (E32 exactly 0: Eemu must be 0 too)
                print(f"    Eemu({mode}) / E32 " + " ".join(f"{x:.2f}" for x in r))
                if mode in M.ACCURATE:
                    assert (eemu <= 2.0 * e32).all(), (name, fine, cl, mode, r)


def _sweep(name, mode, layers=None):
    c = C.case(name)
    ev = c.evaluate()
    out = {}
    for drop in ev["net"].mutants(mode):
        if layers is None or drop[0] in layers:
            out[drop] = M.mutant_ratio(c.emu(ev, mode, drop), mode, ev["ref"], ev["y32"], c.emu(ev, mode),
                                       ev["classes"])
    return out


@pytest.mark.parametrize("mode", SPLIT)
@pytest.mark.parametrize("name", C.MUTANT_CASES)
def test_mutants_are_visible(name, mode):
    """Every (layer, operand) pair that has a low plane in the mode: some output column's E is >= 10 x the bound; the
    alpha head's on sigma, the view layer's on rgb."""
    sweep = _sweep(name, mode)
    net = C.case(name).evaluate()["net"]
    assert {d[0] for d in sweep} >= set(net.layers() if mode != "bf16x3" else ["L1", "skip_h", "alpha"])
    for (layer, op), r in sweep.items():
        print(f"{name} {mode} {layer:7s} {op}: E / bound  r {r[0]:7.1f}  g {r[1]:7.1f}  b {r[2]:7.1f}  sigma {r[3]:7.1f}")
    for (layer, op), r in sweep.items():
        shown = r[3] if layer == "alpha" else (r[:3].max() if layer in ("view_h", "feature") else r.max())
        assert shown >= 10.0, (name, mode, layer, op, r)
    smallest = min(float(r.max()) for r in sweep.values())
    print(f"{name} {mode}: smallest mutant ratio {smallest:.1f} x the bound")
    assert M.FACTOR <= smallest * M.FACTOR / 8, "the factor must stay within 1/8 of the smallest mutant ratio"
    if mode == "bf16x6":  # the third plane alone: reported (module docstring)
        c = C.case(name)
        ev = c.evaluate()
        for layer, op in sweep:
            r = M.mutant_ratio(c.emu(ev, mode, (layer, op + "2")), mode, ev["ref"], ev["y32"], c.emu(ev, mode),
                               ev["classes"])
            print(f"{name} bf16x6 third plane only, {layer:7s} {op}: E / bound " + " ".join(f"{x:5.1f}" for x in r))


def test_init_hides_the_early_layers():
    """The same sweep on the unscaled checkpoint, asserted the other way: fewer than half of the trunk-layer mutants
    reach 10 x the bound (torch's default init contracts, module docstring).  This is why the `he` checkpoints exist."""
    net = C.case("w256_init").evaluate()["net"]
    reach = total = 0
    for mode in SPLIT:
        sweep = _sweep("w256_init", mode, layers=net.trunk_layers())
        n = sum(1 for r in sweep.values() if r.max() >= 10.0)
        print(f"w256_init {mode}: {n} of {len(sweep)} trunk-layer mutants reach 10 x the bound: "
              + " ".join(f"{d[0]}{d[1]}:{r.max():.1f}" for d, r in sweep.items()))
        reach, total = reach + n, total + len(sweep)
    assert 2 * reach < total, (reach, total)


def test_points_and_classes():
    """The point mix: 515 points, whole blocks and a ragged one, every class in most 32-point blocks, three points
    exactly on a joint, far points with exactly-zero windows (asserted in Case.evaluate)."""
    c = C.case("w256_he")
    ev = c.evaluate()
    cl = ev["classes"]
    assert len(c.pts) == C.N_POINTS == 16 * 32 + 3
    counts = {k: int((cl == k).sum()) for k in ("near", "mid", "far")}
    print(counts)
    assert counts["far"] == 86 and counts["near"] >= 150 and counts["mid"] >= 100
    mixed = sum(1 for b in range(16) if {"near", "far"} <= set(cl[32 * b:32 * b + 32].tolist()))
    assert mixed >= 14, mixed
    on = (c.pts == 0).all(1)
    assert on.sum() == 3
    nj = c.cfg.n_joints
    dist = ev["feat64"][on][:, :nj]  # (slot 0 of the kp part: dist w)
    assert (dist[:, 0] == 0).all()
    assert (ev["feat64"][on][:, ev["net"].n_kp:ev["net"].n_kp + 3] == 0).all()  # joint 0's bone direction: 0 / eps


def test_dead_rows_case():
    """`w256_he_dead`: beyond every cutoff no input is live, every hidden row is exactly zero from layer 0 on (the fp16
    modes scale a zero maximum there), and the output is the biases' alone: sigma is the alpha bias exactly, in the
    float64 reference and in the float32 restatement, and every such point has the same output row."""
    c = C.case("w256_he_dead")
    for fine in (False, True):
        ev = c.evaluate(fine=fine)
        net, far = ev["net"], ev["classes"] == "far"
        assert far.sum() == 86
        x = ev["feat64"][torch.as_tensor(far)][:, :net.nx]
        h0 = torch.relu(x @ net.p["pts_linears.0.weight"].T + net.p["pts_linears.0.bias"])
        assert (h0 == 0).all()
        ba = float(net.p["alpha_linear.bias"][0])
        assert (ev["ref"][far, 3] == ba).all() and (ev["y32"][far, 3] == ba).all()
        assert (ev["ref"][far] == ev["ref"][far][0]).all()
        live = torch.relu(ev["feat64"][~torch.as_tensor(far)][:, :net.nx] @ net.p["pts_linears.0.weight"].T
                          + net.p["pts_linears.0.bias"]).max(1).values
        print(f"fine={fine}: rows with a live layer 0 among the other points: {int((live > 0).sum())} of {len(live)}, "
              f"their maxima {float(live[live > 0].min()):.2e} .. {float(live.max()):.2e}")
        assert (live > 0).sum() >= 300

"""The mesh path of run_render.render_mesh at its defaults (res=255 -> 256^3 grid, radius 1.8) on the config-3
model (fine net, 8x256, 24 joints), a synthetic pose: the density grid (fwd_type='mesh') and the iso-surface
extraction (isosurface.isosurface, relu on load) timed separately, HIP events on the launch stream.

The extraction's time includes its one host read of the totals between the count and the emit launches.  The
threshold is the grid's 99th percentile (the synthetic checkpoint's densities do not reach the reference's default
of 10), so the surface has a realistic share of active cells.

Prints one JSON line.  Usage: python tools/mesh_bench.py [res] [precision]"""
import importlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
anerf = importlib.import_module("a-nerf_amd")
syn = importlib.import_module("a-nerf_amd.synthetic")
iso = importlib.import_module("a-nerf_amd.isosurface")


def _time(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), out


def main():
    res = int(sys.argv[1]) if len(sys.argv) > 1 else 255
    prec = sys.argv[2] if len(sys.argv) > 2 else "fp16x4"
    cfg = anerf.RenderConfig(N_samples=64, N_importance=128, precision=prec).validate()
    ck = syn.make_checkpoint(13, n_joints=24, D=8, W=256, fine=True, tau=79.6)
    sc = syn.make_scene(n_joints=24, H=512, W=512, seed=13)
    rc = anerf.RayCaster(cfg, ck)
    kps, skts = torch.from_numpy(sc["kps"][0:1]), torch.from_numpy(sc["skts"][0:1])
    grid_ms, grid = _time(lambda: rc.render_mesh_density(kps, skts, None, radius=1.8, res=res))
    thr = float(torch.quantile(grid.flatten()[:: max(1, grid.numel() // 1000000)].clamp_min(0), 0.99))
    iso_ms, (v, t) = _time(lambda: iso.isosurface(grid, thr, relu=True))
    both_ms, _ = _time(lambda: rc.extract_mesh(kps, skts, None, radius=1.8, res=res, threshold=thr))
    n = (res + 1) ** 3
    print(json.dumps({"metric": "mesh path, res=%d, config3 fine net" % res, "precision": prec, "points": n,
                      "grid_ms": round(grid_ms, 3), "isosurface_ms": round(iso_ms, 3),
                      "extract_mesh_ms": round(both_ms, 3), "isosurface_over_grid": round(iso_ms / grid_ms, 4),
                      "threshold": round(thr, 5), "vertices": int(v.shape[0]), "triangles": int(t.shape[0]),
                      "isosurface_points_per_s": round(n / (iso_ms * 1e-3), 1),
                      "isosurface_grid_read_GBps": round(4 * n / (iso_ms * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()

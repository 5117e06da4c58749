"""Render a small ragged slice of the config-3 frame with debug arrays and alphas, with the library that
ANERF_LIB_PATH names, and save every array: the bit-identity check of the per-ray stages (near / far, z, raws,
weights, alphas, maps) between two builds on one box.  Also the 8 + 4 and 7 + 5 sample counts and I = 0.
Usage: python tools/ab_debug_outputs.py OUT.npz [precision ...]"""
import importlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ablib  # noqa: E402,F401  (ANERF_LIB_PATH: an experiment build, A/B tooling only)

N_RAYS = 261  # (no multiple of the 4 rays of a workgroup)


def main():
    out = sys.argv[1]
    precs = sys.argv[2:] or ["fp16x4", "fp16x3", "bf16x6", "bf16x3", "fp32"]
    anerf = importlib.import_module("a-nerf_amd")
    syn = importlib.import_module("a-nerf_amd.synthetic")
    _lib = importlib.import_module("a-nerf_amd._lib")
    sc = syn.make_scene(n_joints=24, H=512, W=512, seed=13)
    idx, cyls, _ = anerf.rays.valid_pixels(sc["c2ws"], 512, 512, sc["focal"], kps=sc["kps"], ext_scale=0.001)
    dev = torch.device("cuda:0")
    # every 97th traced pixel: rays from all over the box, hits and misses of the cylinder
    pix = torch.from_numpy(np.asarray(idx[0], np.int64)[::97][:N_RAYS].copy()).to(dev)
    c2w = torch.from_numpy(np.ascontiguousarray(sc["c2ws"][0][:3, :4], np.float32)).to(dev)
    rb = torch.empty(pix.shape[0], 11, device=dev)
    _lib.check(_lib.load().anerf_gen_rays(_lib.ptr(c2w), 512, 512, sc["focal"], sc["focal"], 0.0, 0.0, 0,
                                          _lib.ptr(pix), pix.shape[0], 0.0, 1.0, _lib.ptr(rb),
                                          _lib.stream_handle(dev)), "gen_rays")
    sk = torch.from_numpy(sc["skts"][0:1]).to(dev)
    cy = torch.from_numpy(cyls[0:1]).to(dev)
    n = rb.shape[0]
    res = {}
    for S, I in ((64, 128), (8, 4), (7, 5), (33, 0)):
        ck = syn.make_checkpoint(13, n_joints=24, D=8, W=256, fine=I > 0, tau=79.6)
        for p in precs:
            cfg = anerf.RenderConfig(n_joints=24, N_samples=S, N_importance=I, precision=p).validate()
            rc = anerf.RayCaster(cfg, ck)
            o = rc.render_rays(rb, S, skts=sk.expand(n, -1, -1, -1), cyls=cy.expand(n, -1), N_importance=I,
                               chunk=100, ret_alpha=True, debug=True)
            torch.cuda.synchronize()
            for k, v in list(o.items()) + list(rc.last_debug.items()):
                if v is not None:
                    res[f"{p}_{S}+{I}_{k}"] = v.cpu().numpy()
            del rc
    np.savez_compressed(out, **res)
    print(f"{out}: {len(res)} arrays, {n} rays")


if __name__ == "__main__":
    main()

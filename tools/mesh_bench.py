"""The mesh path of run_render.render_mesh at its defaults (res=255 -> 256^3 grid, radius 1.8) on the config-3
model (fine net, 8x256, 24 joints), a synthetic pose: the density grid (fwd_type='mesh') and the iso-surface
extraction (isosurface.isosurface, relu on load) timed separately, HIP events on the launch stream.

The extraction's time includes its one host read of the totals between the count and the emit launches.  The
threshold is the grid's 99th percentile (the synthetic checkpoint's densities do not reach the reference's default
of 10), so the surface has a realistic share of active cells.

The mesh attributes are two more legs: normals_ms, the normals pass alone (anerf_isosurface_normals after a count
pass, no host read), and colors_ms, RayCaster.render_pts_radiance at the mesh's world vertices, each looked at
against its own normal (colors_points of them) -- what extract_mesh(normals=True, colors=True) adds to the grid
and the extraction.  Both are short, so they are timed over 20 repetitions.

The component filter (meshops.py) is four more: components_kernels_ms, the launches of anerf_mesh_components alone (no
host read); components_ms, meshops.mesh_components whole (the id range check, the kernels, the host read of the
count, ranking with torch); compact_ms, meshops.compact_mesh under keep_largest=1's mask (count, one host read,
emit); filter_mesh_ms, filter_mesh(keep_largest=1) on positions and normals -- what extract_mesh(keep_largest=1) adds
(extract_mesh_keep_largest_ms is that call).  components_reference_host_ms is mesh_components_reference (NumPy) on
the same mesh, once, for scale.

Adjacency and smoothing (meshops.py), on the body that keep_largest=1 leaves: adjacency_ms, meshops.vertex_adjacency
whole (the id range check, the kernels, the host read of E); adjacency_kernels_ms, the launches of
anerf_mesh_adjacency_count and _emit back to back into preallocated outputs; smooth_ms, smooth_mesh at its defaults
(10 Taubin iterations: 20 launches) on a precomputed adjacency; smooth_step_us, one launch of the step kernel, from the
difference to a 100-iteration call; extract_mesh_smooth_ms, extract_mesh(keep_largest=1, smooth=10), to put next to
extract_mesh_keep_largest_ms.  smooth_reference_host_ms is smooth_mesh_reference (NumPy) on the same mesh, once, for
scale; the device result is checked against it bit for bit.

Looking at the body (meshops.py; csrc/anerf_raster.hip), on the same filtered mesh: vertex_normals_ms,
meshops.vertex_normals (the id range check and three launches); raster_frame_ms, one 512 x 512 rasterize_mesh of the
body coloured by those normals under frame 7 of turntable_transforms; raster_large_frame_ms, the same image size for a
cube's twelve triangles (the workgroups' path: the body's triangles are a pixel or two each and take the thread's);
turntable_ms, mesh_turntable at its defaults (91 frames of 512 x 512, normals included); raster_reference_host_ms,
rasterize_mesh_reference (NumPy) on the body's frame, once, for scale; the device frame is checked against it bit for
bit.  raster_persp_frame_ms is the same body in world coordinates (extract_mesh(coords="world", keep_largest=1)), 512 x
512, coloured by its normals, through the camera of the benchmark's config-3 path (synthetic.make_scene's c2ws[0],
focal 1.5 H) with near and far given: one rasterize_mesh_camera, next to raster_frame_ms of the same run;
raster_persp_covered_pixels what it covers, raster_persp_reference_host_ms rasterize_mesh_camera_reference on that
frame, once; the device frame is checked against it bit for bit.

Simplification (meshops.simplify_mesh; csrc/anerf_simplify.hip), on the same filtered body in index coordinates from
the origin (0, 0, 0), as extract_mesh(simplify=) runs it, at cell = 2 voxels and (the simplify4_* keys) cell = 4:
simplify_ms, simplify_mesh whole (the bounding box and id range read, the kernels, the host read of the totals);
simplify_kernels_ms, anerf_mesh_simplify_count and _emit back to back into preallocated outputs, no host read between
them; simplify_vertices / simplify_triangles, what is left; extract_mesh_simplify_ms, extract_mesh(keep_largest=1,
smooth=10, simplify=2.0, colors=True), next to extract_mesh_smooth_colors_ms, the same call without simplify;
simplify_reference_host_ms, simplify_mesh_reference (NumPy) at cell 2, once, for scale; the device results are checked
against the checker bit for bit.

Prints one JSON line, and appends it to the file given with --append (the record: profiles/mesh_bench.jsonl).
Usage: python tools/mesh_bench.py [res] [precision] [--append FILE]"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
anerf = importlib.import_module("a-nerf_amd")
syn = importlib.import_module("a-nerf_amd.synthetic")
iso = importlib.import_module("a-nerf_amd.isosurface")
meshops = importlib.import_module("a-nerf_amd.meshops")


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


def _normals_leg(grid, thr):
    """The normals pass alone: a count pass, then anerf_isosurface_normals into a buffer of the counted size."""
    _lib = importlib.import_module("a-nerf_amd._lib")
    lib = _lib.load()
    n0, n1, n2 = grid.shape
    need = lib.anerf_isosurface_workspace(n0, n1, n2)
    ws = torch.empty(need, device=grid.device, dtype=torch.uint8)
    totals = torch.empty(2, device=grid.device, dtype=torch.int64)
    flags = iso.ANERF_ISO_RELU
    _lib.check(lib.anerf_isosurface_count(_lib.ptr(grid), n0, n1, n2, thr, flags, _lib.ptr(ws), need, _lib.ptr(totals),
                                          _lib.stream_handle(grid.device)), "anerf_isosurface_count")
    nv = int(totals[0])
    out = torch.empty((nv, 3), device=grid.device, dtype=torch.float32)
    ms, _ = _time(lambda: _lib.check(lib.anerf_isosurface_normals(
        _lib.ptr(grid), n0, n1, n2, thr, flags, _lib.ptr(ws), need, _lib.ptr(out), nv, _lib.stream_handle(grid.device)),
        "anerf_isosurface_normals"), reps=20)
    return ms


def _components_leg(t, nv):
    """The launches of anerf_mesh_components alone, into preallocated outputs."""
    _lib = importlib.import_module("a-nerf_amd._lib")
    lib = _lib.load()
    nt = int(t.shape[0])
    root, tc, vc = (torch.empty(nv, device=t.device, dtype=torch.int32) for _ in range(3))
    n_comp = torch.empty(1, device=t.device, dtype=torch.int64)
    need = lib.anerf_mesh_components_workspace(nv, nt)
    ws = torch.empty(need, device=t.device, dtype=torch.uint8)
    ms, _ = _time(lambda: _lib.check(lib.anerf_mesh_components(
        _lib.ptr(t), nt, nv, _lib.ptr(root), _lib.ptr(tc), _lib.ptr(vc), _lib.ptr(n_comp), _lib.ptr(ws), need,
        _lib.stream_handle(t.device)), "anerf_mesh_components"), reps=20)
    return ms


def _filter_legs(rc, kps, skts, res, thr, v, t, nrm):
    nv = int(v.shape[0])
    kernels_ms = _components_leg(t, nv)
    comp_ms, comp = _time(lambda: meshops.mesh_components(t, nv), reps=20)
    keep = (comp.labels == 0).to(torch.uint8)
    compact_ms, (_, kept, kt) = _time(lambda: meshops.compact_mesh(keep, t), reps=20)
    filter_ms, _ = _time(lambda: meshops.filter_mesh(v, t, [nrm], keep_largest=1), reps=20)
    keep_ms, _ = _time(lambda: rc.extract_mesh(kps, skts, None, radius=1.8, res=res, threshold=thr, keep_largest=1))
    t_host = t.cpu().numpy()
    t0 = time.perf_counter()
    ref = meshops.mesh_components_reference(t_host, nv)
    ref_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(ref.labels, comp.labels.cpu().numpy())
    return {"components": int(comp.roots.shape[0]), "largest_component_triangles": int(comp.triangle_counts[0]),
            "kept_vertices": int(kept.shape[0]), "kept_triangles": int(kt.shape[0]),
            "components_kernels_ms": round(kernels_ms, 3), "components_ms": round(comp_ms, 3),
            "compact_ms": round(compact_ms, 3), "filter_mesh_ms": round(filter_ms, 3),
            "extract_mesh_keep_largest_ms": round(keep_ms, 3), "components_reference_host_ms": round(ref_ms, 1)}


def _smooth_legs(rc, kps, skts, res, thr, v, t):
    """Adjacency and smoothing on the body (the mesh keep_largest=1 leaves), in index coordinates."""
    _lib = importlib.import_module("a-nerf_amd._lib")
    lib = _lib.load()
    v, t = meshops.filter_mesh(v, t, keep_largest=1)
    nv, nt = int(v.shape[0]), int(t.shape[0])
    adj_ms, adj = _time(lambda: meshops.vertex_adjacency(t, nv), reps=20)
    ne = int(adj.neighbors.shape[0])
    need = lib.anerf_mesh_adjacency_workspace(nv, nt)
    ws = torch.empty(need, device=t.device, dtype=torch.uint8)
    offsets = torch.empty(nv + 1, device=t.device, dtype=torch.int32)
    boundary = torch.empty(nv, device=t.device, dtype=torch.uint8)
    neighbors = torch.empty(ne, device=t.device, dtype=torch.int32)
    totals = torch.empty(2, device=t.device, dtype=torch.int64)

    def kernels():  # both entries back to back, no host read
        s = _lib.stream_handle(t.device)
        _lib.check(lib.anerf_mesh_adjacency_count(_lib.ptr(t), nt, nv, _lib.ptr(ws), need, _lib.ptr(offsets),
                                                  _lib.ptr(boundary), _lib.ptr(totals), s), "anerf_mesh_adjacency_count")
        _lib.check(lib.anerf_mesh_adjacency_emit(nv, _lib.ptr(ws), need, _lib.ptr(offsets), _lib.ptr(neighbors), ne, s),
                   "anerf_mesh_adjacency_emit")
    adj_kernels_ms, _ = _time(kernels, reps=20)
    assert torch.equal(neighbors, adj.neighbors) and torch.equal(offsets, adj.offsets)
    smooth_ms, sm = _time(lambda: meshops.smooth_mesh(v, t, adjacency=adj), reps=20)  # 10 Taubin iterations
    long_ms, _ = _time(lambda: meshops.smooth_mesh(v, t, iterations=100, adjacency=adj), reps=5)
    step_us = (long_ms - smooth_ms) / 180.0 * 1e3  # (the calls differ by 180 launches of the step kernel)
    extract_ms, _ = _time(lambda: rc.extract_mesh(kps, skts, None, radius=1.8, res=res, threshold=thr, keep_largest=1,
                                                  smooth=10))
    v_host, t_host = v.cpu().numpy(), t.cpu().numpy()
    t0 = time.perf_counter()
    ref = meshops.smooth_mesh_reference(v_host, t_host)
    ref_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(ref.view(np.int32), sm.cpu().numpy().view(np.int32))
    return {"adjacency_entries": ne, "largest_degree": int(totals[1]), "boundary_vertices": int(adj.boundary.sum()),
            "adjacency_ms": round(adj_ms, 3), "adjacency_kernels_ms": round(adj_kernels_ms, 3),
            "smooth_ms": round(smooth_ms, 3), "smooth_step_us": round(step_us, 2),
            "extract_mesh_smooth_ms": round(extract_ms, 3), "smooth_reference_host_ms": round(ref_ms, 1)}


def _raster_legs(v, t):
    """Normals, one frame and the turntable on the body (the mesh keep_largest=1 leaves)."""
    v, t = meshops.filter_mesh(v, t, keep_largest=1)
    normals_ms, nrm = _time(lambda: meshops.vertex_normals(v, t), reps=20)
    colors = (nrm * 0.5 + 0.5).contiguous()
    A = meshops.turntable_transforms(v, 91, 4.0, 512, 512)[7]
    frame_ms, frame = _time(lambda: meshops.rasterize_mesh(v, t, A, 512, 512, colors), reps=20)
    cube = torch.tensor([[x, y, z] for x in (-1., 1.) for y in (-1., 1.) for z in (-1., 1.)], device=v.device)
    ct = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                       [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], device=v.device, dtype=torch.int32)
    CA = meshops.turntable_transforms(cube, 91, 4.0, 512, 512, up=(0.2, 0.3, 1.0))[7]
    large_ms, _ = _time(lambda: meshops.rasterize_mesh(cube, ct, CA, 512, 512, cube * 0.5 + 0.5), reps=20)
    turntable_ms, frames = _time(lambda: meshops.mesh_turntable(v, t), reps=3)
    v_host, t_host, c_host = v.cpu().numpy(), t.cpu().numpy(), colors.cpu().numpy()
    t0 = time.perf_counter()
    ref = meshops.rasterize_mesh_reference(v_host, t_host, A, 512, 512, c_host)
    ref_ms = (time.perf_counter() - t0) * 1e3
    for name in ("face_ids", "depth", "bary", "image"):
        g, r = getattr(frame, name).cpu().numpy(), getattr(ref, name)
        assert np.array_equal(g.view(np.int32), r.view(np.int32)), name
    nref = meshops.vertex_normals_reference(v_host, t_host)
    assert np.array_equal(nrm.cpu().numpy().view(np.int32), nref.view(np.int32))
    return {"vertex_normals_ms": round(normals_ms, 3), "raster_frame_ms": round(frame_ms, 3),
            "raster_covered_pixels": int((frame.face_ids >= 0).sum()), "raster_large_frame_ms": round(large_ms, 3),
            "turntable_ms": round(turntable_ms, 3), "turntable_frames": int(frames.shape[0]),
            "raster_reference_host_ms": round(ref_ms, 1)}


def _raster_persp_leg(rc, kps, skts, res, thr, sc):
    """One frame of the body through the render path's perspective camera."""
    v, t = rc.extract_mesh(kps, skts, None, radius=1.8, res=res, threshold=thr, coords="world", keep_largest=1)
    colors = (meshops.vertex_normals(v, t) * 0.5 + 0.5).contiguous()
    c2w, H, W, focal = sc["c2ws"][0], sc["H"], sc["W"], sc["focal"]
    lo, hi = (x.double().cpu().numpy() for x in (v.amin(0), v.amax(0)))
    D, rho = float(np.linalg.norm(c2w[:3, 3] - 0.5 * (lo + hi))), 0.5 * float(np.linalg.norm(hi - lo))
    kw = dict(near=max(D - rho, 1e-3 * rho), far=D + rho, attrs=colors)  # (rasterize_mesh_camera's own defaults)
    frame_ms, frame = _time(lambda: meshops.rasterize_mesh_camera(v, t, c2w, H, W, focal, **kw), reps=20)
    t0 = time.perf_counter()
    ref = meshops.rasterize_mesh_camera_reference(v.cpu().numpy(), t.cpu().numpy(), c2w, H, W, focal,
                                                  **{**kw, "attrs": colors.cpu().numpy()})
    ref_ms = (time.perf_counter() - t0) * 1e3
    for name in ("face_ids", "depth", "bary", "image"):
        g, r = getattr(frame, name).cpu().numpy(), getattr(ref, name)
        assert np.array_equal(g.view(np.int32), r.view(np.int32)), name
    return {"raster_persp_frame_ms": round(frame_ms, 3),
            "raster_persp_covered_pixels": int((frame.face_ids >= 0).sum()),
            "raster_persp_reference_host_ms": round(ref_ms, 1)}


def _simplify_legs(rc, kps, skts, res, thr, v, t):
    """Vertex clustering of the body (the mesh keep_largest=1 leaves), in index coordinates from the origin."""
    v, t = meshops.filter_mesh(v, t, keep_largest=1)
    nv = int(v.shape[0])
    v_host, t_host = v.cpu().numpy(), t.cpu().numpy()
    origin = (0.0, 0.0, 0.0)
    out = {}
    for cell, key in ((2.0, "simplify"), (4.0, "simplify4")):
        whole_ms, got = _time(lambda: meshops.simplify_mesh(v, t, cell, origin=origin), reps=20)
        kv, kt = int(got.vertices.shape[0]), int(got.triangles.shape[0])
        c32 = np.float32(cell)
        o = np.zeros(3, np.float32)
        dims = (np.floor(v.amax(0).cpu().numpy() / c32).astype(np.int32) + 1)
        ws = meshops._simplify_workspace(nv, int(t.shape[0]), dims, v.device)
        totals = torch.empty(2, device=v.device, dtype=torch.int64)
        out_v, out_t = torch.empty_like(got.vertices), torch.empty_like(got.triangles)
        vmap, reps = torch.empty_like(got.vertex_map), torch.empty_like(got.representatives)

        def kernels():  # both entries back to back, no host read
            meshops._simplify_count(v, t, o, c32, dims, ws, totals)
            meshops._simplify_emit(v, t, o, c32, dims, ws, out_v, out_t, vmap, reps)
        kernels_ms, _ = _time(kernels, reps=20)
        assert totals.tolist() == [kv, kt]
        t0 = time.perf_counter()
        ref = meshops.simplify_mesh_reference(v_host, t_host, cell, origin=origin)
        ref_ms = (time.perf_counter() - t0) * 1e3
        for mine in (got, (out_v, out_t, vmap, reps)):
            for g, r in zip(mine, ref[:4]):
                g = g.cpu().numpy()
                assert g.shape == r.shape and np.array_equal(g.view(np.int32), r.view(np.int32))
        out.update({key + "_ms": round(whole_ms, 3), key + "_kernels_ms": round(kernels_ms, 3),
                    key + "_vertices": kv, key + "_triangles": kt})
        if cell == 2.0:
            out["simplify_reference_host_ms"] = round(ref_ms, 1)
    kw = dict(radius=1.8, res=res, threshold=thr, keep_largest=1, smooth=10, colors=True)
    plain_ms, _ = _time(lambda: rc.extract_mesh(kps, skts, None, **kw))
    simple_ms, _ = _time(lambda: rc.extract_mesh(kps, skts, None, simplify=2.0, **kw))
    out.update({"extract_mesh_smooth_colors_ms": round(plain_ms, 3), "extract_mesh_simplify_ms": round(simple_ms, 3)})
    return out


def main():
    argv = list(sys.argv[1:])
    append = None
    if "--append" in argv:
        i = argv.index("--append")
        append = argv[i + 1]
        del argv[i:i + 2]
    res = int(argv[0]) if len(argv) > 0 else 255
    prec = argv[1] if len(argv) > 1 else "fp16x4"
    cfg = anerf.RenderConfig(N_samples=64, N_importance=128, precision=prec).validate()
    ck = syn.make_checkpoint(13, n_joints=24, D=8, W=256, fine=True, tau=79.6)
    sc = syn.make_scene(n_joints=24, H=512, W=512, seed=13)
    rc = anerf.RayCaster(cfg, ck)
    kps, skts = torch.from_numpy(sc["kps"][0:1]), torch.from_numpy(sc["skts"][0:1])
    grid_ms, grid = _time(lambda: rc.render_mesh_density(kps, skts, None, radius=1.8, res=res))
    thr = float(torch.quantile(grid.flatten()[:: max(1, grid.numel() // 1000000)].clamp_min(0), 0.99))
    iso_ms, (v, t) = _time(lambda: iso.isosurface(grid, thr, relu=True))
    both_ms, _ = _time(lambda: rc.extract_mesh(kps, skts, None, radius=1.8, res=res, threshold=thr))
    normals_ms = _normals_leg(grid, thr)
    vw, _, attrs = rc.extract_mesh(kps, skts, None, radius=1.8, res=res, threshold=thr, coords="world", normals=True)
    dirs = (0.0 - attrs["normals"]).contiguous()
    colors_ms, raw = _time(lambda: rc.render_pts_radiance(vw, dirs, kps, skts, None), reps=20)
    attrs_ms, _ = _time(lambda: rc.extract_mesh(kps, skts, None, radius=1.8, res=res, threshold=thr, normals=True,
                                                colors=True))
    _, ti, ni = iso.isosurface(grid, thr, relu=True, normals=True)
    legs = _filter_legs(rc, kps, skts, res, thr, v, ti, ni)
    legs.update(_smooth_legs(rc, kps, skts, res, thr, v, ti))
    legs.update(_raster_legs(v, ti))
    legs.update(_raster_persp_leg(rc, kps, skts, res, thr, sc))
    legs.update(_simplify_legs(rc, kps, skts, res, thr, v, ti))
    n = (res + 1) ** 3
    line = json.dumps({"metric": "mesh path, res=%d, config3 fine net" % res, "precision": prec, "points": n,
                      "grid_ms": round(grid_ms, 3), "isosurface_ms": round(iso_ms, 3),
                      "extract_mesh_ms": round(both_ms, 3), "isosurface_over_grid": round(iso_ms / grid_ms, 4),
                      "threshold": round(thr, 5), "vertices": int(v.shape[0]), "triangles": int(t.shape[0]),
                      "isosurface_points_per_s": round(n / (iso_ms * 1e-3), 1),
                      "isosurface_grid_read_GBps": round(4 * n / (iso_ms * 1e-3) / 1e9, 1),
                      "normals_ms": round(normals_ms, 3), "colors_ms": round(colors_ms, 3),
                      "colors_points": int(raw.shape[0]), "normals_over_grid": round(normals_ms / grid_ms, 4),
                      "colors_over_grid": round(colors_ms / grid_ms, 4),
                      "extract_mesh_normals_colors_ms": round(attrs_ms, 3), **legs,
                      "filter_over_grid": round(legs["filter_mesh_ms"] / grid_ms, 4)})
    print(line, flush=True)
    if append:
        with open(append, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

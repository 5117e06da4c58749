"""Iso-surface of a density grid as an indexed triangle mesh, extracted on the device (marching cubes).

`run_render.render_mesh` (run_render.py:970-986) takes the `fwd_type='mesh'` grid to the host and runs
`mcubes.marching_cubes` over it.  Here the grid stays in HBM: `isosurface` runs the count / scan / emit kernels of
csrc/anerf_iso.hip (anerf_isosurface_count, anerf_isosurface_emit; include/anerf.h) and returns device tensors.

The contract, shared by the kernels and by `isosurface_reference` (a NumPy implementation kept as the checker,
reached only by that name -- nothing falls back to it):
  * a sample is inside when value >= threshold (a NaN is outside); `relu` clamps the samples at 0 as they are
    read (the reference's np.maximum(raw_d, 0)), which moves vertices, not only the classification;
  * one vertex per sign-changing grid edge, owned by the edge's lower grid point p and its axis, at
    p + t e_axis with t = (threshold - a) / (b - a) in fp32 (a: the value at p), in array-index coordinates
    (axis 0, 1, 2) as mcubes.marching_cubes returns them; vertices sorted by (p's linear index, axis);
  * triangles from the case table csrc/anerf_iso_table.inc (tools/gen_iso_table.py), int32 vertex ids, sorted by
    (cell's linear index, table order).  A grid with a dimension of 1 has no cells: an empty mesh.  Normals point from dense to empty; `flip` reverses the winding.
    mcubes is not installed where this was developed: its triangle order and winding were not compared.
"""
import os
import re

import numpy as np
import torch

from . import _lib

ANERF_ISO_RELU = 1
ANERF_ISO_FLIP = 2
TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "anerf_iso_table.inc")
_table = None


def load_table():
    """The case table of csrc/anerf_iso_table.inc (the file the kernels compile in) as NumPy arrays:
    dict(edge_corner [12], edge_axis [12], ntri [256], tri [256, 15])."""
    global _table
    if _table is None:
        with open(TABLE_PATH) as f:
            src = re.sub(r"//[^\n]*", "", f.read())
        out = {}
        for name, shape in (("EDGE_CORNER", (12,)), ("EDGE_AXIS", (12,)), ("NTRI", (256,)), ("TRI", (256, 15))):
            m = re.search(r"ANERF_ISO_%s(?:\[\d+\])+\s*=\s*\{(.*?)\};" % name, src, flags=re.S)
            if m is None:
                raise RuntimeError(f"{TABLE_PATH}: ANERF_ISO_{name} not found")
            out[name.lower()] = np.array([int(v) for v in re.findall(r"-?\d+", m.group(1))], np.int64).reshape(shape)
        _table = out
    return _table


def _flags(relu, flip):
    return (ANERF_ISO_RELU if relu else 0) | (ANERF_ISO_FLIP if flip else 0)


@torch.no_grad()
def isosurface(volume, threshold, relu=False, flip=False):
    """(vertices float32 [V, 3], triangles int32 [T, 3]) of `volume` [n0, n1, n2] at `threshold`, as device
    tensors (see the module docstring for the contract).  A CPU tensor or NumPy array is uploaded to the
    current device; the grid is read as float32.  One host read of the two totals sits between the count and
    the emit launches; everything runs on the current stream."""
    if isinstance(volume, np.ndarray):
        volume = np.array(volume, dtype=np.float32)  # (a copy: torch takes no read-only arrays)
    vol = torch.as_tensor(volume)
    if vol.dim() != 3:
        raise ValueError(f"isosurface takes a 3-D grid, got shape {tuple(vol.shape)}")
    if not vol.is_cuda:
        vol = vol.to(torch.device("cuda", torch.cuda.current_device()))
    vol = vol.to(torch.float32).contiguous()
    dev = vol.device
    n0, n1, n2 = (int(s) for s in vol.shape)
    if min(n0, n1, n2) < 1:
        raise ValueError(f"isosurface: empty grid {tuple(vol.shape)}")
    lib = _lib.load()
    flags = _flags(relu, flip)
    with torch.cuda.device(dev):
        stream = _lib.stream_handle(dev)
        need = lib.anerf_isosurface_workspace(n0, n1, n2)
        if need == 0:
            raise _lib.AnerfError(f"anerf_isosurface_workspace: {lib.anerf_last_error().decode(errors='replace')}")
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        totals = torch.empty(2, device=dev, dtype=torch.int64)
        _lib.check(lib.anerf_isosurface_count(_lib.ptr(vol), n0, n1, n2, float(threshold), flags, _lib.ptr(ws), need,
                                              _lib.ptr(totals), stream), "anerf_isosurface_count")
        nv, nt = (int(x) for x in totals.cpu())  # (the one sync: the output sizes)
        if nv > 0x7fffffff or nt > 0x7fffffff:
            raise _lib.AnerfError(f"isosurface: {nv} vertices / {nt} triangles do not fit int32 ids")
        vertices = torch.empty((nv, 3), device=dev, dtype=torch.float32)
        triangles = torch.empty((nt, 3), device=dev, dtype=torch.int32)
        _lib.check(lib.anerf_isosurface_emit(_lib.ptr(vol), n0, n1, n2, float(threshold), flags, _lib.ptr(ws), need,
                                             _lib.ptr(vertices), nv, _lib.ptr(triangles), nt, stream),
                   "anerf_isosurface_emit")
    return vertices, triangles


def isosurface_reference(volume, threshold, relu=False, flip=False):
    """NumPy implementation of the same contract (same table, same fp32 arithmetic, same order): the checker
    of `isosurface`.  Returns (vertices float32 [V, 3], triangles int32 [T, 3]) as arrays."""
    if isinstance(volume, torch.Tensor):
        volume = volume.detach().cpu().numpy()
    v = np.ascontiguousarray(volume, dtype=np.float32)
    if v.ndim != 3 or min(v.shape) < 1:
        raise ValueError(f"isosurface_reference takes a non-empty 3-D grid, got shape {v.shape}")
    if relu:
        v = np.where(v < 0, np.float32(0), v)  # (np.maximum(v, 0): a NaN stays a NaN)
    thr = np.float32(threshold)
    tab = load_table()
    n = v.shape
    if min(n) < 2:  # (no cells: no triangles, and no vertices, which belong to the cells around their edge)
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    with np.errstate(invalid="ignore"):
        inside = v >= thr
    lin = np.arange(v.size, dtype=np.int64).reshape(n)
    # vertices: the sign-changing edges, sorted by (owner's linear index, axis)
    keys, pos = [], []
    for a in range(3):
        lo = tuple(slice(0, n[d] - 1) if d == a else slice(None) for d in range(3))
        hi = tuple(slice(1, None) if d == a else slice(None) for d in range(3))
        idx = np.nonzero(inside[lo] != inside[hi])
        va, vb = v[lo][idx], v[hi][idx]
        with np.errstate(all="ignore"):
            t = (thr - va) / (vb - va)
        p = np.stack([c.astype(np.float32) for c in idx], -1).reshape(-1, 3)
        p[:, a] = p[:, a] + t
        keys.append(lin[lo][idx] * 3 + a)
        pos.append(p)
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    vertices = np.concatenate(pos)[order].astype(np.float32).reshape(-1, 3)
    # triangles: the active cells in linear order, the table's order within a cell
    tris = []
    if min(n) >= 2:
        case = np.zeros((n[0] - 1, n[1] - 1, n[2] - 1), np.int64)
        for c in range(8):
            d = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
            case |= inside[d[0]:n[0] - 1 + d[0], d[1]:n[1] - 1 + d[1], d[2]:n[2] - 1 + d[2]].astype(np.int64) << c
        stride = (n[1] * n[2], n[2], 1)
        corner_off = [sum(((c >> d) & 1) * stride[d] for d in range(3)) for c in range(8)]
        edge_key = [(corner_off[int(c)] * 3 + int(a)) for c, a in zip(tab["edge_corner"], tab["edge_axis"])]
        for i, j, k in zip(*np.nonzero(tab["ntri"][case] > 0)):
            c = case[i, j, k]
            base = int(lin[i, j, k]) * 3
            e = tab["tri"][c, :3 * tab["ntri"][c]]
            ids = np.searchsorted(keys, [base + edge_key[x] for x in e])
            tris.append(ids.reshape(-1, 3))
    triangles = (np.concatenate(tris) if tris else np.zeros((0, 3))).astype(np.int32).reshape(-1, 3)
    if flip:
        triangles = np.ascontiguousarray(triangles[:, [0, 2, 1]])
    return vertices, triangles


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: float x / y / z per vertex, then `list uchar int vertex_indices` per face."""
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
    t = triangles.detach().cpu().numpy() if isinstance(triangles, torch.Tensor) else np.asarray(triangles)
    v = np.ascontiguousarray(v, dtype="<f4").reshape(-1, 3)
    t = np.ascontiguousarray(t, dtype="<i4").reshape(-1, 3)
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


def read_ply(path):
    """(vertices, triangles) of a file written by write_ply."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    head = blob[:end].decode("ascii")
    if "format binary_little_endian 1.0" not in head:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = int(re.search(r"element vertex (\d+)", head).group(1))
    nt = int(re.search(r"element face (\d+)", head).group(1))
    v = np.frombuffer(blob, "<f4", nv * 3, end).reshape(nv, 3).copy()
    faces = np.frombuffer(blob, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), nt, end + nv * 12)
    if nt and not (faces["n"] == 3).all():
        raise ValueError(f"{path}: non-triangle faces")
    return v, faces["i"].astype(np.int32).reshape(nt, 3).copy()


def mesh_from_grid(grid, kps, radius, res, threshold, coords="unit", flip=False):
    """extract_mesh's second half: the iso-surface of a caster's render_mesh_density grid (relu on load, as
    run_render.render_mesh's np.maximum(raw_d, 0)) in the requested coordinates:
      "index"  array-index coordinates, as mcubes.marching_cubes;
      "unit"   vertices / res - .5  (run_render.py:985);
      "world"  (lin(v1), lin(v0), lin(v2)) + kps[0, 0], lin(t) = -radius + 2 radius t / res: the grid is the
               'xy' meshgrid of anerf_density_grid, element (a, b, c) at (axis[b], axis[a], axis[c]); swapping two
               axes mirrors the mesh, so the winding is reversed there to keep the normals pointing outward."""
    if coords not in ("unit", "index", "world"):
        raise ValueError(f"coords must be 'unit', 'index' or 'world', got {coords!r}")
    v, t = isosurface(grid, threshold, relu=True, flip=bool(flip) != (coords == "world"))
    if coords == "unit":
        v = v / res - .5
    elif coords == "world":
        kp0 = torch.as_tensor(kps).to(v.device, torch.float32).reshape(-1, 3)[0]
        v = (-radius + (2.0 * radius / res) * v[:, [1, 0, 2]]) + kp0
    return v, t


@torch.no_grad()
def render_mesh(basedir, render_kwargs, tensor_data, chunk=1024, radius=1.80, res=255, threshold=10.):
    """Drop-in for run_render.render_mesh (run_render.py:970-986): per pose, the density grid and its iso-surface
    on the device, written to basedir/meshes/{i:03d}.ply in the reference's vertices / res - .5 coordinates.
    Returns the list of (vertices, triangles) device tensors (the reference builds that list and drops it)."""
    ray_caster = render_kwargs["ray_caster"]
    os.makedirs(os.path.join(basedir, "meshes"), exist_ok=True)
    kps, skts, bones = tensor_data["kp"], tensor_data["skts"], tensor_data["bones"]
    v_t_tuples = []
    for i in range(len(kps)):
        v, t = ray_caster.extract_mesh(kps[i:i + 1], skts[i:i + 1], None if bones is None else bones[i:i + 1],
                                       radius=radius, res=res, threshold=threshold)
        write_ply(os.path.join(basedir, "meshes", f"{i:03d}.ply"), v, t)
        v_t_tuples.append((v, t))
    return v_t_tuples

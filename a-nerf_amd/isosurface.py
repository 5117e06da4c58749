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

Vertex normals (`normals=True`; anerf_isosurface_normals, include/anerf.h) come from the grid's gradient, not from
the faces (the reference's viewer accumulates face normals on the host, render_mesh.py:35-53).  The contract, again
shared by the kernel and `isosurface_reference`; all arithmetic fp32, separately rounded:
  * values are taken as read: relu-clamped under `relu`, and a NaN stays a NaN;
  * the gradient at a grid point q along axis a is (f[q + e_a] - f[q - e_a]) * 0.5f in the interior,
    f[q + e_a] - f[q] in the first row and f[q] - f[q - e_a] in the last: no index ever leaves the grid;
  * for the vertex owned by (p, axis) with the vertex's own t: G = g(p) + t * (g(p + e_axis) - g(p)) per component;
  * n = -G / sqrtf((Gx*Gx + Gy*Gy) + Gz*Gz), which points from dense to empty; it is negated under `flip`, so that
    it always agrees with the winding.  Where G is zero or not finite in any component n = (0, 0, 0) (precisely:
    unless 0 < the squared length < inf, which also covers a squared length that underflows or overflows).
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
def isosurface(volume, threshold, relu=False, flip=False, normals=False):
    """(vertices float32 [V, 3], triangles int32 [T, 3]) of `volume` [n0, n1, n2] at `threshold`, as device
    tensors (see the module docstring for the contract).  A CPU tensor or NumPy array is uploaded to the
    current device; the grid is read as float32.  One host read of the two totals sits between the count and
    the emit launches; everything runs on the current stream.
    `normals=True` returns (vertices, triangles, normals float32 [V, 3]): one more pass over the grid."""
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
        need = _lib.workspace("anerf_isosurface_workspace", n0, n1, n2)
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
        if normals:
            nrm = torch.empty((nv, 3), device=dev, dtype=torch.float32)
            _lib.check(lib.anerf_isosurface_normals(_lib.ptr(vol), n0, n1, n2, float(threshold), flags, _lib.ptr(ws),
                                                    need, _lib.ptr(nrm), nv, stream), "anerf_isosurface_normals")
            return vertices, triangles, nrm
    return vertices, triangles


def _grid_gradient(v):
    """The contract's gradient of a float32 grid (every dimension >= 2): [3, n0, n1, n2]."""
    g = np.empty((3,) + v.shape, np.float32)
    half = np.float32(0.5)
    for a in range(3):
        f = np.moveaxis(v, a, 0)
        o = np.moveaxis(g[a], a, 0)
        o[1:-1] = (f[2:] - f[:-2]) * half
        o[0] = f[1] - f[0]
        o[-1] = f[-1] - f[-2]
    return g


def isosurface_reference(volume, threshold, relu=False, flip=False, normals=False):
    """NumPy implementation of the same contract (same table, same fp32 arithmetic, same order): the checker
    of `isosurface`.  Returns (vertices float32 [V, 3], triangles int32 [T, 3]) as arrays, and with
    `normals=True` the vertex normals float32 [V, 3] as the third."""
    v = np.ascontiguousarray(_lib.host_array(volume), dtype=np.float32)
    if v.ndim != 3 or min(v.shape) < 1:
        raise ValueError(f"isosurface_reference takes a non-empty 3-D grid, got shape {v.shape}")
    if relu:
        v = np.where(v < 0, np.float32(0), v)  # (np.maximum(v, 0): a NaN stays a NaN)
    thr = np.float32(threshold)
    tab = load_table()
    n = v.shape
    if min(n) < 2:  # (no cells: no triangles, and no vertices, which belong to the cells around their edge)
        empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
        return empty + (np.zeros((0, 3), np.float32),) if normals else empty
    grad = None
    if normals:
        with np.errstate(all="ignore"):
            grad = _grid_gradient(v)
    with np.errstate(invalid="ignore"):
        inside = v >= thr
    lin = np.arange(v.size, dtype=np.int64).reshape(n)
    # vertices: the sign-changing edges, sorted by (owner's linear index, axis)
    keys, pos, gvec = [], [], []
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
        if normals:  # G = g(p) + t (g(p + e_a) - g(p)), per component
            with np.errstate(all="ignore"):
                gvec.append(np.stack([grad[c][lo][idx] + t * (grad[c][hi][idx] - grad[c][lo][idx]) for c in range(3)],
                                     -1).astype(np.float32).reshape(-1, 3))
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
    if normals:
        G = np.concatenate(gvec)[order].reshape(-1, 3)
        with np.errstate(all="ignore"):
            sq = (G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2]
            ok = (sq > 0) & (sq < np.inf)
            nrm = (G if flip else -G) / np.sqrt(sq)[:, None]
        nrm = np.where(ok[:, None], nrm, np.float32(0)).astype(np.float32)
        return vertices, triangles, nrm
    return vertices, triangles


def _host(x, dtype):
    return np.ascontiguousarray(_lib.host_array(x), dtype=dtype).reshape(-1, 3)


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: float x / y / z per vertex (then float nx / ny / nz with `normals` [V, 3], then
    uchar red / green / blue with `colors` [V, 3]: floats in [0, 1] stored as clip(rint(255 c), 0, 255), or uint8
    as they are), then `list uchar int vertex_indices` per face.  Without the extras: the plain x / y / z file."""
    v = _host(vertices, "<f4")
    t = _host(triangles, "<i4")
    fields, props = [("xyz", "<f4", (3,))], "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        fields.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields.append(("c", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    rec = np.zeros(len(v), dtype=fields)
    rec["xyz"] = v
    if normals is not None:
        n = _host(normals, "<f4")
        if len(n) != len(v):
            raise ValueError(f"write_ply: {len(n)} normals for {len(v)} vertices")
        rec["n"] = n
    if colors is not None:
        c = _lib.host_array(colors)
        if c.dtype != np.uint8:
            with np.errstate(invalid="ignore"):
                c = np.clip(np.rint(np.float32(255) * c.astype(np.float32)), 0, 255)
            c = np.nan_to_num(c, nan=0.0).astype(np.uint8)
        c = c.reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"write_ply: {len(c)} colours for {len(v)} vertices")
        rec["c"] = c
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\n{props}"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2",
              "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4",
              "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def read_ply(path, attributes=False):
    """(vertices, triangles) of a file written by write_ply; the vertex properties are parsed from the header, so
    a file with normals or colours reads the same.  `attributes=True` returns (vertices, triangles, attrs) with
    attrs["normals"] float32 [V, 3] (nx / ny / nz) and attrs["colors"] uint8 [V, 3] (red / green / blue) where the
    file has them."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    head = blob[:end].decode("ascii")
    if "format binary_little_endian 1.0" not in head:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = int(re.search(r"element vertex (\d+)", head).group(1))
    nt = int(re.search(r"element face (\d+)", head).group(1))
    fields, element = [], None
    for line in head.splitlines():
        w = line.split()
        if w[:1] == ["element"]:
            element = w[1]
        elif w[:1] == ["property"] and element == "vertex":
            if len(w) != 3 or w[1] not in _PLY_TYPES:
                raise ValueError(f"{path}: unsupported vertex property {line!r}")
            fields.append((w[2], _PLY_TYPES[w[1]]))
    names = [n for n, _ in fields]
    if not all(c in names for c in "xyz"):
        raise ValueError(f"{path}: vertices without x / y / z")
    vdt = np.dtype(fields)
    rec = np.frombuffer(blob, vdt, nv, end)
    v = np.stack([rec[c].astype(np.float32) for c in "xyz"], -1).reshape(nv, 3)
    faces = np.frombuffer(blob, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), nt, end + nv * vdt.itemsize)
    if nt and not (faces["n"] == 3).all():
        raise ValueError(f"{path}: non-triangle faces")
    t = faces["i"].astype(np.int32).reshape(nt, 3).copy()
    if not attributes:
        return v, t
    attrs = {}
    if all(c in names for c in ("nx", "ny", "nz")):
        attrs["normals"] = np.stack([rec[c].astype(np.float32) for c in ("nx", "ny", "nz")], -1).reshape(nv, 3)
    if all(c in names for c in ("red", "green", "blue")):
        attrs["colors"] = np.stack([rec[c].astype(np.uint8) for c in ("red", "green", "blue")], -1).reshape(nv, 3)
    return v, t, attrs


def mesh_from_grid(grid, kps, radius, res, threshold, coords="unit", flip=False, normals=False, colors=False,
                   view="normal", cams=None, radiance=None, keep_largest=None, min_triangles=0, smooth=0,
                   smooth_lambda=0.5, smooth_mu=-0.53, simplify=None):
    """extract_mesh's second half: the iso-surface of a caster's render_mesh_density grid (relu on load, as
    run_render.render_mesh's np.maximum(raw_d, 0)) in the requested coordinates:
      "index"  array-index coordinates, as mcubes.marching_cubes;
      "unit"   vertices / res - .5  (run_render.py:985);
      "world"  (lin(v1), lin(v0), lin(v2)) + kps[0, 0], lin(t) = -radius + 2 radius t / res: the grid is the
               'xy' meshgrid of anerf_density_grid, element (a, b, c) at (axis[b], axis[a], axis[c]); swapping two
               axes mirrors the mesh, so the winding is reversed there to keep the normals pointing outward.
    With `normals` or `colors` returns (v, t, attrs), attrs a dict of device tensors [V, 3] float32:
      "normals"  the gradient normals (module docstring) in the frame of `coords`: as extracted for "index" and
                 "unit", columns [1, 0, 2] for "world"; dense to empty, negated under `flip` like the winding;
      "colors"   sigmoid of the raw rgb that `radiance(pts, dirs, cams)` (RayCaster.render_pts_radiance bound to
                 a pose) returns at the WORLD vertices, whatever `coords`, in [0, 1].  view="normal": each vertex
                 is looked at along its inward world normal (from outside, straight on), and where the normal is
                 zero along the direction from the vertex to kps[0, 0]; view=(x, y, z): one direction for all.
    An empty mesh gives (0, 3) attributes and launches nothing more.
    `keep_largest` / `min_triangles` drop connected components (meshops.filter_mesh: keep_largest=1 keeps the body
    and drops the floaters and cavity surfaces of a noisy density) right after the extraction, before the colour
    query: dropped vertices cost no radiance work, and the normals returned are the kept rows.  With the defaults
    that code is not entered.
    `smooth` > 0 runs that many Taubin iterations (meshops.smooth_mesh with lam=smooth_lambda, mu=smooth_mu,
    pin="boundary"; smooth_mu=None: plain Laplacian) right after the component filter, in index coordinates, before
    the `unit` / `world` mapping: the colours are queried at the smoothed world vertices.  attrs["normals"] stay the
    gradient normals of the UNSMOOTHED crossing (face-based normals of the smoothed surface are not computed), and
    they still give the view directions of view="normal".  With smooth=0 that code is not entered.
    `normals="faces"`: attrs["normals"] are instead the face-accumulated normals (meshops.vertex_normals, the
    colouring of the reference's viewer) of the FINAL vertices -- after the filter, the smoothing and the `coords`
    mapping, for the winding returned -- and with view="normal" these give the view directions of the colour query;
    the grid's gradient is not evaluated.  normals=True / False behave as before.
    `simplify`: a cell edge in voxels (> 0) runs meshops.simplify_mesh (vertex clustering) after the component filter
    and the smoothing, in index coordinates with origin (0, 0, 0) -- the cells are blocks of voxels, the same ones for
    every frame of a sequence -- and before the `coords` mapping and the colour query: colours are queried at the
    simplified vertices only.  The gradient normals are gathered by representative (a new vertex takes the normal of
    its cell's first vertex); normals="faces" are computed on the final, simplified mesh.  With simplify=None that
    code is not entered."""
    if coords not in ("unit", "index", "world"):
        raise ValueError(f"coords must be 'unit', 'index' or 'world', got {coords!r}")
    one_dir = None
    if colors:
        if radiance is None:
            raise ValueError("colors=True needs the network: use RayCaster.extract_mesh")
        if not (isinstance(view, str) and view == "normal"):
            one_dir = torch.as_tensor(view, dtype=torch.float32).reshape(-1)
            if one_dir.numel() != 3:
                raise ValueError(f"view must be 'normal' or one direction (x, y, z), got {view!r}")
    faces = isinstance(normals, str)
    if faces and normals != "faces":
        raise ValueError(f"normals must be True, False or 'faces', got {normals!r}")
    wflip = bool(flip) != (coords == "world")  # the winding's flag in index coordinates
    need_n = not faces and (bool(normals) or (bool(colors) and one_dir is None))
    if need_n:
        v, t, n = isosurface(grid, threshold, relu=True, flip=wflip, normals=True)
    else:
        v, t = isosurface(grid, threshold, relu=True, flip=wflip)
        n = None
    if keep_largest is not None or min_triangles > 0:
        from .meshops import filter_mesh
        if n is None:
            v, t = filter_mesh(v, t, keep_largest=keep_largest, min_triangles=min_triangles)
        else:
            v, t, (n,) = filter_mesh(v, t, [n], keep_largest=keep_largest, min_triangles=min_triangles)
    if smooth != 0:  # (a negative count is smooth_mesh's ValueError)
        from .meshops import smooth_mesh
        v = smooth_mesh(v, t, iterations=smooth, lam=smooth_lambda, mu=smooth_mu, pin="boundary")
    if simplify is not None:  # (a cell that is not > 0 is simplify_mesh's ValueError)
        from .meshops import simplify_mesh
        simple = simplify_mesh(v, t, simplify, attrs=None if n is None else [n], origin=(0.0, 0.0, 0.0))
        v, t = simple.vertices, simple.triangles
        if n is not None:
            (n,) = simple.attrs
    vi = v
    kp0 = torch.as_tensor(kps).to(v.device, torch.float32).reshape(-1, 3)[0]

    def world():  # the index-to-world mapping of the docstring, of the (smoothed) index vertices
        return (-radius + (2.0 * radius / res) * vi[:, [1, 0, 2]]) + kp0
    if coords == "unit":
        v = vi / res - .5
    elif coords == "world":
        v = world()
    if not (normals or colors):
        return v, t
    attrs = {}
    if faces:
        from .meshops import vertex_normals
        nf = vertex_normals(v, t)
        attrs["normals"] = nf
        # in place of the gradient normal of the index frame: the winding follows `wflip` there, and the axis swap
        # (a reflection) turns a face normal round, so nf read in index columns is n, negated under "world"
        n = nf if coords != "world" else (0.0 - nf)[:, [1, 0, 2]]
    elif normals:
        # (the axis swap is a reflection: a vector follows it as it is, while the winding's flag was reversed for
        # it -- so the extracted normals are negated back; 0 - n keeps a zero normal +0)
        attrs["normals"] = (0.0 - n[:, [1, 0, 2]]) if coords == "world" else n
    if colors:
        if len(v) == 0:
            attrs["colors"] = torch.zeros((0, 3), device=v.device, dtype=torch.float32)
        else:
            vw = v if coords == "world" else world()
            if one_dir is not None:
                dirs = one_dir.to(v.device)
            else:
                inward = (n if not wflip else 0.0 - n)[:, [1, 0, 2]]  # n is dense -> empty unless wflip
                inward = 0.0 - inward
                zero = (inward == 0).all(-1, keepdim=True)
                dirs = torch.where(zero, kp0 - vw, inward).contiguous()
            raw = radiance(vw.contiguous(), dirs, cams)
            attrs["colors"] = torch.sigmoid(raw[:, :3].to(torch.float32))
    return v, t, attrs


@torch.no_grad()
def render_mesh(basedir, render_kwargs, tensor_data, chunk=1024, radius=1.80, res=255, threshold=10.,
                normals=False, colors=False, view="normal", keep_largest=None, min_triangles=0, smooth=0,
                smooth_lambda=0.5, smooth_mu=-0.53, simplify=None):
    """Drop-in for run_render.render_mesh (run_render.py:970-986): per pose, the density grid and its iso-surface
    on the device, written to basedir/meshes/{i:03d}.ply in the reference's vertices / res - .5 coordinates.
    Returns the list of (vertices, triangles) device tensors (the reference builds that list and drops it).
    `normals` (True, or "faces" for the face-accumulated normals of the final vertices) / `colors` / `view`: as
    RayCaster.extract_mesh; the attributes go into the PLYs (nx / ny / nz,
    red / green / blue) and the list holds (vertices, triangles, attrs).  `keep_largest` / `min_triangles`: the
    component filter of RayCaster.extract_mesh (keep_largest=1: the body without floaters).  `smooth` /
    `smooth_lambda` / `smooth_mu`: its Taubin smoothing, after the filter; the PLYs hold the smoothed vertices, and
    their normals stay the gradient normals of the unsmoothed crossing.  `simplify`: its vertex clustering (a cell edge
    in voxels), after the smoothing; the PLYs hold the simplified mesh."""
    ray_caster = render_kwargs["ray_caster"]
    os.makedirs(os.path.join(basedir, "meshes"), exist_ok=True)
    kps, skts, bones = tensor_data["kp"], tensor_data["skts"], tensor_data["bones"]
    extras = dict(normals=normals, colors=colors, view=view) if (normals or colors) else {}
    keeps = (dict(keep_largest=keep_largest, min_triangles=min_triangles)
             if (keep_largest is not None or min_triangles > 0) else {})
    if smooth != 0:
        keeps.update(smooth=smooth, smooth_lambda=smooth_lambda, smooth_mu=smooth_mu)
    if simplify is not None:
        keeps.update(simplify=simplify)
    v_t_tuples = []
    for i in range(len(kps)):
        out = ray_caster.extract_mesh(kps[i:i + 1], skts[i:i + 1], None if bones is None else bones[i:i + 1],
                                      radius=radius, res=res, threshold=threshold, **extras, **keeps)
        attrs = out[2] if extras else {}
        write_ply(os.path.join(basedir, "meshes", f"{i:03d}.ply"), out[0], out[1], normals=attrs.get("normals"),
                  colors=attrs.get("colors"))
        v_t_tuples.append(tuple(out))
    return v_t_tuples

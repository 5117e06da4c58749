"""Connected components of an extracted mesh and floater removal, its vertex adjacency and smoothing, on the device.

The iso-surface of a noisy density (isosurface.py) is the body plus detached blobs of density ("floaters") and closed
cavity surfaces inside it.  The reference leaves them to the user (trimesh, split(), keep the biggest: a trip to the
host and a library that is not shipped).  Here the triangle list stays in HBM: `mesh_components` labels it with the
union-find of csrc/anerf_mesh.hip (anerf_mesh_components; include/anerf.h) and `filter_mesh` drops components with the
count / scan / emit compaction of the same file (anerf_mesh_compact_count, anerf_mesh_compact_emit).

The contract, shared by the kernels and by `mesh_components_reference` / `filter_mesh_reference` (NumPy, kept as the
checkers, reached only by those names -- nothing falls back to them):
  * two vertices are in one component iff a chain of triangle edges links them; a vertex that no triangle uses is a
    component with 0 triangles; a component's root is its smallest vertex id; a triangle belongs to the component of
    its first vertex;
  * components are ranked by triangle count, most first, ties by the smaller root (integers only: the order does not
    depend on the schedule -- ranking by area or volume would sum floats in arrival order);
  * filtering keeps a component iff rank < keep_largest (when given) and triangle_count >= min_triangles; a vertex
    survives iff its component does, a triangle iff its three vertices do; the surviving vertices and triangles
    keep their original relative order, ids remapped; every per-vertex array is gathered with the same index.

The surface that remains is a noisy density's: voxel staircases and ripple, which the reference's users smooth on the
host (trimesh.smoothing.filter_taubin).  `vertex_adjacency` builds the vertex connectivity as a CSR
(anerf_mesh_adjacency_count, anerf_mesh_adjacency_emit) and `smooth_mesh` runs Laplacian / Taubin steps over it
(anerf_mesh_smooth: one gather kernel, launched once per step).  Their contract, shared with
`vertex_adjacency_reference` / `smooth_mesh_reference` (NumPy checkers again, reached only by those names):
  * every triangle (a, b, c) lists the ordered pairs (a,b) (a,c) (b,a) (b,c) (c,a) (c,b); pairs with equal ends are
    dropped; row v is the set of distinct u with (v,u) listed, ascending (offsets int32 [V + 1], neighbors int32 [E]);
    a vertex that no triangle uses has an empty row;
  * boundary[v] iff some (v,u) is listed exactly once; a duplicated triangle, or a degenerate one such as (1,1,3),
    lists its pairs twice, which is not boundary.  Integers only: the same on every run;
  * one smoothing step with weight w, for a vertex v with neighbours u_0 < ... < u_{d-1}, d > 0, not pinned, per
    component in fp32 with every operation separately rounded: s = p[u_0], then s = s + p[u_k] for k = 1 .. d-1 in that
    order; m = s / float(d); p'[v] = p[v] + w (m - p[v]).  d = 0 or pinned: p'[v] = p[v], bit for bit.  Every step
    reads only the previous step's positions (Jacobi).  NaN and inf propagate as the arithmetic gives them;
  * one iteration is a step with lam, then a step with mu when mu is given (Taubin's lambda | mu, which does not
    shrink the body as the plain Laplacian does).

Looking at the result is the last step (the reference's render_mesh.py: 91 orthographic views through OpenGL, coloured
by normals).  `vertex_normals` (anerf_mesh_vertex_normals), `rasterize_mesh` (anerf_mesh_raster) and `mesh_turntable`
do it on the device, csrc/anerf_raster.hip; their contract, shared with `vertex_normals_reference` /
`rasterize_mesh_reference` (NumPy checkers, reached only by those names), is written out in include/anerf.h and
DESIGN.md: quantised face normals summed as 64-bit integers; coverage on vertices snapped to 1 / 256 pixel with
integer edge functions and a tie rule; a depth test that is one 64-bit atomic min per fragment.  Those are the viewer's
orthographic / affine cameras.  `camera_view`, `rasterize_mesh_camera` (anerf_mesh_raster_persp) and
`render_mesh_views` draw the mesh through the perspective cameras everything else here speaks in (c2w, H, W, focal,
center: render_path, gen_rays, the dataset), checked by `rasterize_mesh_camera_reference`: triangles are cut at the
near plane (a cut point is a function of its edge's IN and OUT end alone, so neighbours get the same bits: no cracks),
the cut polygon is fanned into one or two sub-triangles that go through the same integer coverage, 1 / depth is
interpolated (perspective-correct depth, weights and attributes), and the key holds the camera depth and the original
triangle's id.  No side-plane clipping, no multisampling, no back-face culling, and no image files are written.

The extracted mesh is as dense as the grid (two triangles per surface voxel), and whoever takes it further decimates it
first; the reference leaves that to trimesh, which needs open3d or fast_simplification for it.  `simplify_mesh` is
vertex clustering (Rossignac-Borrel) on the device, csrc/anerf_simplify.hip (anerf_mesh_simplify_count,
anerf_mesh_simplify_emit): one pass of integer decisions.  Its contract, shared with `simplify_mesh_reference` (the
NumPy checker, reached only by that name), for vertices fp32 [V, 3], triangles int32 [T, 3], a cell edge `cell` > 0
(fp32), an origin o (fp32 [3]) and dims (n0, n1, n2) with n0 n1 n2 <= SIMPLIFY_MAX_CELLS = 2^26; every fp32 operation
is separately rounded, divisions are correctly rounded:
  * the cell of a vertex: q_a = (p_a - o_a) / cell, c_a = floor(q_a); the vertex is valid iff all three q_a are finite
    and 0 <= c_a < n_a; its key is (c0 n1 + c1) n2 + c2;
  * a cell's representative is its valid member with the smallest vertex id; the new vertices are the representatives
    in ascending original id (the relative order is kept, as in filter_mesh); vertex_map[v] is the new id of v's
    cell, or -1 for a vertex that is not valid; representatives[j] is the original id of new vertex j;
  * the position of a new vertex is the fixed-point mean of its cell's members, which does not depend on the order of
    arrival: r_a = q_a - float(c_a) (exact in fp32), i_a = rint(r_a 2^20) as int64, S_a the 64-bit integer sum of
    i_a over the members (below 2^51), n their number; m_a = float(double(S_a) / double(n) 2^-20);
    p'_a = o_a + cell (float(c_a) + m_a);
  * a triangle (a, b, c) maps to (a', b', c') through vertex_map and is dropped if an id is outside [0, V), a mapped
    id is -1, two mapped ids are equal, or an earlier surviving triangle (a smaller original index) has the same
    unordered set {a', b', c'}, in either winding; the survivors keep their relative order and their own vertex
    order, neither rotated nor re-wound;
  * integers, or a fixed order of roundings, throughout: the same bits on every run and under any schedule.
Out of scope: quadric-error placement, edge-collapse decimation, target triangle counts, and keeping the result
manifold -- clustering can pinch thin parts into edges that more than two triangles share (it does on a random field's
surface; closed, well-separated surfaces such as a sphere or a torus stay closed).
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

MeshComponents = collections.namedtuple("MeshComponents", ["labels", "roots", "triangle_counts", "vertex_counts"])
VertexAdjacency = collections.namedtuple("VertexAdjacency", ["offsets", "neighbors", "boundary"])
MeshRaster = collections.namedtuple("MeshRaster", ["face_ids", "depth", "bary", "image"])
SimplifiedMesh = collections.namedtuple("SimplifiedMesh",
                                        ["vertices", "triangles", "vertex_map", "representatives", "attrs"])
SIMPLIFY_MAX_CELLS = _lib.ANERF_SIMPLIFY_MAX_CELLS  # the cells of simplify_mesh's grid at most (include/anerf.h)
# the clipped bounding box (in pixel centres) up to which the thread that set a triangle up also draws it
# (include/anerf.h; larger boxes are drained by workgroups -- the outputs are the same bits either way)
RASTER_SMALL_PIXELS = _lib.ANERF_RASTER_SMALL_PIXELS
RASTER_MAX_DIM = 16384
RASTER_MAX_CHANNELS = 8


def _check_ids(triangles, n_vertices, who):
    """The precondition of the kernels, checked with torch before anything is launched."""
    if triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"{who}: triangles must be [T, 3], got shape {tuple(triangles.shape)}")
    if triangles.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: triangles must be int32 or int64, got {triangles.dtype}")
    if n_vertices < 0 or n_vertices > 0x7fffffff or triangles.shape[0] > 0x7fffffff:
        raise ValueError(f"{who}: {n_vertices} vertices / {triangles.shape[0]} triangles do not fit int32 ids")
    if triangles.shape[0] > 0:
        lo, hi = int(triangles.amin()), int(triangles.amax())
        if lo < 0 or hi >= n_vertices:
            raise ValueError(f"{who}: vertex ids span [{lo}, {hi}], outside [0, {n_vertices})")


def _device_triangles(triangles, n_vertices, who):
    t = torch.as_tensor(triangles)
    _check_ids(t, int(n_vertices), who)
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t.to(torch.int32).contiguous()


def _components_raw(t, n_vertices):
    """anerf_mesh_components on a checked device list: (root, tri_count, vert_count int32 [V], n_components int)."""
    dev = t.device
    lib = _lib.load()
    nv, nt = int(n_vertices), int(t.shape[0])
    with torch.cuda.device(dev):
        root = torch.empty(nv, device=dev, dtype=torch.int32)
        tri_count = torch.empty(nv, device=dev, dtype=torch.int32)
        vert_count = torch.empty(nv, device=dev, dtype=torch.int32)
        n_comp = torch.empty(1, device=dev, dtype=torch.int64)
        need = lib.anerf_mesh_components_workspace(nv, nt)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        _lib.check(lib.anerf_mesh_components(_lib.ptr(t), nt, nv, _lib.ptr(root), _lib.ptr(tri_count),
                                             _lib.ptr(vert_count), _lib.ptr(n_comp), _lib.ptr(ws), need,
                                             _lib.stream_handle(dev)), "anerf_mesh_components")
        return root, tri_count, vert_count, int(n_comp.cpu())  # (the one sync: the number of components)


@torch.no_grad()
def mesh_components(triangles, n_vertices):
    """The connected components of the mesh (triangles int [T, 3], ids in [0, n_vertices)), ranked: rank 0 has the
    most triangles, ties go to the smaller root.  Returns device tensors
      labels int32 [V]            the rank of each vertex's component,
      roots int32 [C]             each component's smallest vertex id, by rank,
      triangle_counts int64 [C],  vertex_counts int64 [C].
    An id outside [0, n_vertices) raises ValueError before anything is launched.  The labelling runs in
    anerf_mesh_components on the current stream; ranking the C components is a torch sort."""
    return _components(_device_triangles(triangles, n_vertices, "mesh_components"), int(n_vertices))


def _components(t, n_vertices):
    dev = t.device
    with torch.cuda.device(dev):
        root, tri_count, vert_count, n_comp = _components_raw(t, n_vertices)
        ids = torch.arange(int(n_vertices), device=dev, dtype=torch.int32)
        roots = ids[root == ids]  # ascending
        if roots.shape[0] != n_comp:
            raise _lib.AnerfError(f"mesh_components: {n_comp} components counted, {roots.shape[0]} roots found")
        idx = roots.long()
        tc = tri_count[idx].long()
        order = torch.sort(-tc, stable=True).indices  # (the roots ascend: a stable sort breaks ties by root)
        rank_of_root = torch.empty(int(n_vertices), device=dev, dtype=torch.int32)
        rank_of_root[idx[order]] = torch.arange(n_comp, device=dev, dtype=torch.int32)
        labels = rank_of_root[root.long()]
        return MeshComponents(labels, roots[order], tc[order], vert_count[idx].long()[order])


def mesh_components_reference(triangles, n_vertices):
    """NumPy implementation of the same contract, the checker of `mesh_components`: minimum-label propagation over
    the triangles with pointer jumping, until nothing changes.  Returns MeshComponents of arrays."""
    tri = np.ascontiguousarray(_lib.host_array(triangles), dtype=np.int64).reshape(-1, 3)
    nv = int(n_vertices)
    if len(tri) and (tri.min() < 0 or tri.max() >= nv):
        raise ValueError(f"mesh_components_reference: vertex ids span [{tri.min()}, {tri.max()}], outside [0, {nv})")
    lab = np.arange(nv, dtype=np.int64)
    flat = tri.reshape(-1)
    while len(tri):
        new = lab.copy()
        np.minimum.at(new, flat, np.repeat(lab[tri].min(axis=1), 3))
        while True:  # (lab[v] <= v and lab[v] is in v's component throughout)
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.nonzero(lab == np.arange(nv))[0]
    tc = np.bincount(lab[tri[:, 0]], minlength=nv)[roots] if len(tri) else np.zeros(len(roots), np.int64)
    vc = np.bincount(lab, minlength=nv)[roots]
    order = np.lexsort((roots, -tc))
    rank_of_root = np.zeros(nv, np.int64)
    rank_of_root[roots[order]] = np.arange(len(roots))
    return MeshComponents(rank_of_root[lab].astype(np.int32), roots[order].astype(np.int32),
                          tc[order].astype(np.int64), vc[order].astype(np.int64))


def _kept_components(triangle_counts, keep_largest, min_triangles):
    """The filter's rule on the ranked counts (a torch tensor or an array): a bool per component."""
    n = len(triangle_counts)
    ok = triangle_counts >= int(min_triangles)
    if keep_largest is not None:
        if isinstance(ok, torch.Tensor):
            ok = ok & (torch.arange(n, device=ok.device) < int(keep_largest))
        else:
            ok = ok & (np.arange(n) < int(keep_largest))
    return ok


def _gather_attrs(attrs, gather, n_vertices, who="filter_mesh"):
    if attrs is None:
        return None
    items = attrs.items() if isinstance(attrs, dict) else enumerate(attrs)
    out = {}
    for k, a in items:
        if a.shape[0] != n_vertices:
            raise ValueError(f"{who}: attribute {k!r} has {a.shape[0]} rows for {n_vertices} vertices")
        out[k] = gather(a)
    return out if isinstance(attrs, dict) else [out[i] for i in range(len(out))]


@torch.no_grad()
def compact_mesh(keep, triangles):
    """The compaction alone: keep uint8 / bool [V] (a vertex survives iff keep[v] != 0), triangles int32 [T, 3] on
    the device.  Returns (vertex_map int32 [V] (the new id or -1), kept int32 [V'] (old ids, ascending), triangles
    int32 [T', 3] remapped), both in their original relative order.  One host read of the two totals sits between
    the count and the emit launches (as in isosurface); everything runs on the current stream.
    Stricter than the C entry it wraps: anerf_mesh_compact_* drop a triangle with an id outside [0, V) silently (so
    that a bad list cannot read out of bounds), here such an id raises ValueError before anything is launched, as
    in mesh_components.  A module-level helper of filter_mesh (tools/mesh_bench.py times it), not exported from
    the package."""
    keep = torch.as_tensor(keep)
    return _compact(keep, _device_triangles(triangles, int(keep.shape[0]), "compact_mesh"))


def _compact(keep, t):
    dev = t.device
    keep = keep.to(dev).ne(0).to(torch.uint8).contiguous()
    nv, nt = int(keep.shape[0]), int(t.shape[0])
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _lib.stream_handle(dev)
        need = _lib.workspace("anerf_mesh_compact_workspace", nv, nt)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        totals = torch.empty(2, device=dev, dtype=torch.int64)
        _lib.check(lib.anerf_mesh_compact_count(_lib.ptr(keep), nv, _lib.ptr(t), nt, _lib.ptr(ws), need,
                                                _lib.ptr(totals), stream), "anerf_mesh_compact_count")
        kv, kt = (int(x) for x in totals.cpu())  # (the one sync: the output sizes)
        vertex_map = torch.empty(nv, device=dev, dtype=torch.int32)
        kept = torch.empty(kv, device=dev, dtype=torch.int32)
        out = torch.empty((kt, 3), device=dev, dtype=torch.int32)
        _lib.check(lib.anerf_mesh_compact_emit(_lib.ptr(keep), nv, _lib.ptr(t), nt, _lib.ptr(ws), need,
                                               _lib.ptr(vertex_map), _lib.ptr(kept), kv, _lib.ptr(out), kt, stream),
                   "anerf_mesh_compact_emit")
    return vertex_map, kept, out


@torch.no_grad()
def filter_mesh(vertices, triangles, attrs=None, keep_largest=None, min_triangles=0):
    """Drop connected components of a mesh (vertices [V, 3], triangles int32 [T, 3], device tensors as `isosurface`
    returns them): a component is kept iff rank < keep_largest (when given; rank 0 has the most triangles, ties go
    to the smaller root) and its triangle count >= min_triangles.  keep_largest=1 gives "the body, not the debris".
    Returns (vertices, triangles), or (vertices, triangles, attrs) when `attrs` is given: a dict (or list) of
    per-vertex tensors [V, ...], each gathered with the same index as the vertices.  Surviving vertices and
    triangles keep their relative order; nothing kept gives (0, 3) tensors.  With keep_largest=None and
    min_triangles=0 the inputs are returned unchanged and nothing is launched."""
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError(f"filter_mesh: keep_largest must be >= 0 or None, got {keep_largest}")
    if keep_largest is None and int(min_triangles) <= 0:
        return (vertices, triangles) if attrs is None else (vertices, triangles, attrs)
    v = torch.as_tensor(vertices)
    nv = int(v.shape[0])
    t = _device_triangles(triangles, nv, "filter_mesh")
    dev = t.device
    with torch.cuda.device(dev):
        comp = _components(t, nv)
        ok = _kept_components(comp.triangle_counts, keep_largest, min_triangles)
        keep = ok[comp.labels.long()].to(torch.uint8)
        _, kept, tris = _compact(keep, t)
        idx = kept.long()

        def gather(a):
            return torch.as_tensor(a).to(dev).index_select(0, idx)
        out_v = gather(v)
        out_a = _gather_attrs(attrs, gather, nv)
    return (out_v, tris) if attrs is None else (out_v, tris, out_a)


def filter_mesh_reference(vertices, triangles, attrs=None, keep_largest=None, min_triangles=0):
    """NumPy implementation of `filter_mesh`'s contract on `mesh_components_reference`: its checker."""
    host = _lib.host_array
    v = host(vertices)
    tri = np.ascontiguousarray(host(triangles), dtype=np.int32).reshape(-1, 3)
    if keep_largest is None and int(min_triangles) <= 0:
        return (vertices, triangles) if attrs is None else (vertices, triangles, attrs)
    comp = mesh_components_reference(tri, len(v))
    keep = _kept_components(comp.triangle_counts, keep_largest, min_triangles)[comp.labels]
    kept = np.nonzero(keep)[0]
    vertex_map = np.full(len(v), -1, np.int32)
    vertex_map[kept] = np.arange(len(kept), dtype=np.int32)
    alive = keep[tri].all(axis=1) if len(tri) else np.zeros(0, bool)
    out_t = vertex_map[tri[alive]].astype(np.int32).reshape(-1, 3)
    out_a = _gather_attrs(attrs, lambda a: host(a)[kept], len(v))
    return (v[kept], out_t) if attrs is None else (v[kept], out_t, out_a)


# ------------------------------------------------------------------ vertex adjacency and smoothing
def _adjacency(t, n_vertices):
    """anerf_mesh_adjacency_count / _emit on a checked device list."""
    dev = t.device
    lib = _lib.load()
    nv, nt = int(n_vertices), int(t.shape[0])
    if 6 * nt >= 2 ** 31:
        raise ValueError(f"vertex_adjacency: {nt} triangles list {6 * nt} pairs, which do not fit int32 offsets")
    with torch.cuda.device(dev):
        stream = _lib.stream_handle(dev)
        need = _lib.workspace("anerf_mesh_adjacency_workspace", nv, nt)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        offsets = torch.empty(nv + 1, device=dev, dtype=torch.int32)
        boundary = torch.empty(nv, device=dev, dtype=torch.uint8)
        totals = torch.empty(2, device=dev, dtype=torch.int64)
        _lib.check(lib.anerf_mesh_adjacency_count(_lib.ptr(t), nt, nv, _lib.ptr(ws), need, _lib.ptr(offsets),
                                                  _lib.ptr(boundary), _lib.ptr(totals), stream),
                   "anerf_mesh_adjacency_count")
        ne = int(totals.cpu()[0])  # (the one sync: the number of entries)
        neighbors = torch.empty(ne, device=dev, dtype=torch.int32)
        _lib.check(lib.anerf_mesh_adjacency_emit(nv, _lib.ptr(ws), need, _lib.ptr(offsets), _lib.ptr(neighbors), ne,
                                                 stream), "anerf_mesh_adjacency_emit")
    return VertexAdjacency(offsets, neighbors, boundary.view(torch.bool))  # (the kernels write 0 / 1)


@torch.no_grad()
def vertex_adjacency(triangles, n_vertices):
    """The vertex adjacency of the mesh (triangles int [T, 3], ids in [0, n_vertices)) as a CSR of device tensors:
      offsets int32 [V + 1], neighbors int32 [E]   row v, neighbors[offsets[v]:offsets[v + 1]], holds the distinct
                                                   vertices that share a triangle edge with v, ascending;
      boundary bool [V]                            v is on an edge that only one triangle has (module docstring).
    An id outside [0, n_vertices) raises ValueError before anything is launched, and so do 6 T >= 2^31 listed pairs.
    One host read of E sits between the count and the emit launches (as in compact_mesh); everything runs on the
    current stream."""
    return _adjacency(_device_triangles(triangles, n_vertices, "vertex_adjacency"), int(n_vertices))


def _listed_pairs(tri):
    """The ordered pairs the triangles list, equal ends dropped: (first ends, second ends), int64."""
    a, b = tri[:, [0, 0, 1, 1, 2, 2]].reshape(-1), tri[:, [1, 2, 0, 2, 0, 1]].reshape(-1)
    ok = a != b
    return a[ok], b[ok]


def vertex_adjacency_reference(triangles, n_vertices):
    """NumPy implementation of the adjacency's contract, the checker of `vertex_adjacency`: the listed pairs as
    sorted keys v * V + u, their distinct values and multiplicities.  Returns VertexAdjacency of arrays."""
    tri = np.ascontiguousarray(_lib.host_array(triangles), dtype=np.int64).reshape(-1, 3)
    nv = int(n_vertices)
    if len(tri) and (tri.min() < 0 or tri.max() >= nv):
        raise ValueError(f"vertex_adjacency_reference: vertex ids span [{tri.min()}, {tri.max()}], outside [0, {nv})")
    if 6 * len(tri) >= 2 ** 31:
        raise ValueError(f"vertex_adjacency_reference: {len(tri)} triangles list too many pairs for int32 offsets")
    a, b = _listed_pairs(tri)
    keys, mult = np.unique(a * max(nv, 1) + b, return_counts=True)
    v, u = keys // max(nv, 1), keys % max(nv, 1)
    offsets = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(v, minlength=nv), out=offsets[1:])
    boundary = np.zeros(nv, bool)
    boundary[v[mult == 1]] = True
    return VertexAdjacency(offsets.astype(np.int32), u.astype(np.int32), boundary)


def _smooth_args(shape, iterations, lam, mu, who):
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{who}: vertices must be [V, 3], got shape {tuple(shape)}")
    if int(iterations) != iterations or iterations < 0:
        raise ValueError(f"{who}: iterations must be an integer >= 0, got {iterations}")
    if not np.isfinite(lam) or (mu is not None and not np.isfinite(mu)):
        raise ValueError(f"{who}: lam and mu must be finite, got {lam}, {mu}")


def _pin_mask(pin, n_vertices, boundary, who):
    """`pin` as None or a [V] mask: "boundary" -> boundary() (evaluated only then), None, or the caller's mask."""
    if pin is None:
        return None
    if isinstance(pin, str):
        if pin != "boundary":
            raise ValueError(f"{who}: pin must be 'boundary', None or a mask [V], got {pin!r}")
        return boundary()
    shape = tuple(pin.shape)
    if shape != (n_vertices,):
        raise ValueError(f"{who}: the pin mask has shape {shape} for {n_vertices} vertices")
    return pin


@torch.no_grad()
def smooth_mesh(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, pin="boundary", adjacency=None):
    """Laplacian / Taubin smoothing of a mesh (vertices float [V, 3], triangles int [T, 3]) on the device: every
    iteration moves each vertex towards the mean of its neighbours by `lam`, then by `mu` (negative: back out, so
    that the body keeps its volume -- Taubin's lambda | mu); mu=None gives the plain Laplacian, which shrinks.
    Returns the positions float32 [V, 3] on the device; the input is not written.  The arithmetic is the module
    docstring's contract, bit for bit the same as `smooth_mesh_reference`.
    `pin`: "boundary" holds the vertices of open edges in place (a body cut open by the grid box does not shrink
    from its rim), None pins nothing, or a bool / uint8 mask [V] of vertices to hold.
    `adjacency`: a VertexAdjacency of the same mesh from `vertex_adjacency` to reuse (the triangles are not read
    then); otherwise it is built here, with its one host read.
    iterations=0 returns `vertices` as given and launches nothing.  Every step is one launch of anerf_mesh_smooth's
    kernel on the current stream."""
    shape = tuple(vertices.shape) if hasattr(vertices, "shape") else np.shape(vertices)
    _smooth_args(shape, iterations, lam, mu, "smooth_mesh")
    if not isinstance(pin, str) and pin is not None:
        pin = torch.as_tensor(pin)
    _pin_mask(pin, shape[0], lambda: None, "smooth_mesh")  # (the argument errors come before any launch)
    if int(iterations) == 0:
        return vertices
    nv = shape[0]
    adj = adjacency if adjacency is not None else vertex_adjacency(triangles, nv)
    if tuple(adj.offsets.shape) != (nv + 1,):
        raise ValueError(f"smooth_mesh: the adjacency has {adj.offsets.shape[0] - 1} rows for {nv} vertices")
    dev = adj.offsets.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        p = torch.as_tensor(vertices).to(dev, torch.float32).contiguous()
        mask = _pin_mask(pin, nv, lambda: adj.boundary, "smooth_mesh")
        if mask is not None:
            mask = mask.to(dev).ne(0).to(torch.uint8).contiguous()
        out = torch.empty_like(p)
        scratch = torch.empty_like(p)
        flags = _lib.ANERF_SMOOTH_TAUBIN if mu is not None else 0
        _lib.check(lib.anerf_mesh_smooth(_lib.ptr(p), nv, _lib.ptr(adj.offsets), _lib.ptr(adj.neighbors),
                                         int(adj.neighbors.shape[0]), _lib.ptr(mask), int(iterations), float(lam),
                                         float(mu) if mu is not None else 0.0, flags, _lib.ptr(out),
                                         _lib.ptr(scratch), _lib.stream_handle(dev)), "anerf_mesh_smooth")
    return out


def _smooth_step_reference(p, offsets, neighbors, w, pinned):
    """One step of the contract on float32 [V, 3]: the row sums taken column by column (k = 0, 1, ...: the k-th
    neighbour of every row that has one), which keeps each row's order of additions."""
    deg = np.diff(offsets)
    start = offsets[:-1]
    s = np.zeros_like(p)
    for k in range(int(deg.max()) if len(deg) else 0):
        rows = np.nonzero(deg > k)[0]
        q = p[neighbors[start[rows] + k]]
        s[rows] = q if k == 0 else s[rows] + q
    out = p.copy()
    move = np.nonzero((deg > 0) & ~pinned)[0]
    with np.errstate(all="ignore"):
        m = s[move] / deg[move].astype(np.float32)[:, None]
        out[move] = p[move] + np.float32(w) * (m - p[move])
    return out


def smooth_mesh_reference(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, pin="boundary", adjacency=None):
    """NumPy implementation of `smooth_mesh`'s contract on `vertex_adjacency_reference`: its checker.  float32
    throughout; returns an array [V, 3]."""
    host = _lib.host_array
    v = host(vertices)
    _smooth_args(v.shape, iterations, lam, mu, "smooth_mesh_reference")
    p = np.array(v, dtype=np.float32)
    nv = len(p)
    if not isinstance(pin, str) and pin is not None:
        pin = host(pin)
    _pin_mask(pin, nv, lambda: None, "smooth_mesh_reference")
    if int(iterations) == 0:
        return p
    adj = adjacency if adjacency is not None else vertex_adjacency_reference(triangles, nv)
    mask = _pin_mask(pin, nv, lambda: host(adj.boundary), "smooth_mesh_reference")
    pinned = np.zeros(nv, bool) if mask is None else mask != 0
    offsets, neighbors = host(adj.offsets).astype(np.int64), host(adj.neighbors).astype(np.int64)
    for _ in range(int(iterations)):
        p = _smooth_step_reference(p, offsets, neighbors, lam, pinned)
        if mu is not None:
            p = _smooth_step_reference(p, offsets, neighbors, mu, pinned)
    return p


# ------------------------------------------------------------------ face-accumulated vertex normals
_F = np.float32
_QUANT = np.float32(2.0 ** 30)
_NORMAL_EPS = np.float32(1e-8)


def _check_vertices(shape, who):
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{who}: vertices must be [V, 3], got shape {tuple(shape)}")


@torch.no_grad()
def vertex_normals(vertices, triangles):
    """Vertex normals float32 [V, 3] (device) of a mesh (vertices float [V, 3], triangles int [T, 3]) from its faces:
    every triangle adds its unit normal, with equal weight, to its three vertices, and the sums are normalised -- the
    colouring of the reference's viewer (render_mesh.py compute_normal), for the winding as given.  The arithmetic is
    include/anerf.h's contract (fp32, separately rounded; lengths below 1e-8 raised to it, the viewer's normalize_v3;
    the face normals quantised to 2^-30 and summed as 64-bit integers, so the result is the same on every run), bit
    for bit that of `vertex_normals_reference`.  A vertex that no triangle uses gets (0, 0, 0).
    Not mirrored: the viewer's own `norm[faces[:, k]] += n` loses duplicate indices (NumPy's buffered fancy-index add:
    only one face per column reaches a vertex); its intent, equal-weight accumulation over ALL incident faces, is
    what is implemented.  An id outside [0, V) raises ValueError before anything is launched.  Three launches on the
    current stream, no host read."""
    v = torch.as_tensor(vertices)
    _check_vertices(tuple(v.shape), "vertex_normals")
    nv = int(v.shape[0])
    t = _device_triangles(triangles, nv, "vertex_normals")
    return _vertex_normals(v.to(t.device, torch.float32).contiguous(), t)


def _vertex_normals(p, t):
    dev = t.device
    lib = _lib.load()
    nv, nt = int(p.shape[0]), int(t.shape[0])
    with torch.cuda.device(dev):
        need = _lib.workspace("anerf_mesh_vertex_normals_workspace", nv, nt)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        out = torch.empty((nv, 3), device=dev, dtype=torch.float32)
        _lib.check(lib.anerf_mesh_vertex_normals(_lib.ptr(p), nv, _lib.ptr(t), nt, _lib.ptr(out), _lib.ptr(ws), need,
                                                 _lib.stream_handle(dev)), "anerf_mesh_vertex_normals")
    return out


def _normalize_reference(n):
    """n / max(|n|, 1e-8) on float32 [N, 3], |n| = sqrt((x x + y y) + z z)."""
    with np.errstate(all="ignore"):
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ln = np.where(ln < _NORMAL_EPS, _NORMAL_EPS, ln)  # (a NaN length stays)
        return (n / ln[:, None]).astype(_F)


def _host_triangles(triangles, nv, who):
    tri = np.ascontiguousarray(_lib.host_array(triangles), dtype=np.int64).reshape(-1, 3)
    if len(tri) and (tri.min() < 0 or tri.max() >= nv):
        raise ValueError(f"{who}: vertex ids span [{tri.min()}, {tri.max()}], outside [0, {nv})")
    return tri


def vertex_normals_reference(vertices, triangles):
    """NumPy implementation of `vertex_normals`' contract: its checker.  Returns float32 [V, 3]."""
    p = np.ascontiguousarray(_lib.host_array(vertices), dtype=_F)
    _check_vertices(p.shape, "vertex_normals_reference")
    nv = len(p)
    tri = _host_triangles(triangles, nv, "vertex_normals_reference")
    acc = np.zeros((nv, 3), np.int64)
    if len(tri):
        with np.errstate(all="ignore"):
            a = p[tri[:, 0]]
            e1, e2 = p[tri[:, 1]] - a, p[tri[:, 2]] - a
            n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(_F)
            n = _normalize_reference(n)
            q = np.where(np.isfinite(n), np.rint(np.where(np.isfinite(n), n, _F(0)) * _QUANT), _F(0)).astype(np.int64)
        for k in range(3):
            np.add.at(acc, tri[:, k], q)
    s = acc.astype(_F) * _F(2.0 ** -30)
    return _normalize_reference(s)


# ------------------------------------------------------------------ the rasteriser
def _raster_args(vertices_shape, transform, width, height, attrs_shape, background, who):
    """The argument errors of rasterize_mesh and its checker: (transform float32 [3, 4], C, background float32 [C])."""
    _check_vertices(vertices_shape, who)
    A = np.ascontiguousarray(_lib.host_array(transform), dtype=_F)
    if A.shape != (3, 4):
        raise ValueError(f"{who}: transform must be [3, 4], got shape {A.shape}")
    for name, x in (("width", width), ("height", height)):
        if int(x) != x or not 1 <= int(x) <= RASTER_MAX_DIM:
            raise ValueError(f"{who}: {name} must be an integer in [1, {RASTER_MAX_DIM}], got {x}")
    if attrs_shape is None:
        return A, 0, np.zeros(0, _F)
    if len(attrs_shape) != 2 or attrs_shape[0] != vertices_shape[0]:
        raise ValueError(f"{who}: attrs of shape {tuple(attrs_shape)} for {vertices_shape[0]} vertices ([V, C] wanted)")
    nch = int(attrs_shape[1])
    if not 1 <= nch <= RASTER_MAX_CHANNELS:
        raise ValueError(f"{who}: attrs must have 1 to {RASTER_MAX_CHANNELS} channels, got {nch}")
    bg = np.asarray(background, dtype=_F).reshape(-1)
    if bg.size == 1:
        bg = np.repeat(bg, nch)
    if bg.size != nch:
        raise ValueError(f"{who}: background must be one value or {nch}, got {bg.size}")
    return A, nch, np.ascontiguousarray(bg)


def _raster_launch(p, t, A, width, height, a, nch, bg, ws):
    """One anerf_mesh_raster call on checked device tensors (ws: its workspace, reusable between frames)."""
    dev = t.device
    lib = _lib.load()
    face_ids = torch.empty((height, width), device=dev, dtype=torch.int32)
    depth = torch.empty((height, width), device=dev, dtype=torch.float32)
    bary = torch.empty((height, width, 3), device=dev, dtype=torch.float32)
    image = torch.empty((height, width, nch), device=dev, dtype=torch.float32) if nch else None
    _lib.check(lib.anerf_mesh_raster(_lib.ptr(p), int(p.shape[0]), _lib.ptr(t), int(t.shape[0]),
                                     A.ctypes.data_as(ctypes.c_void_p), width, height, _lib.ptr(a), nch,
                                     bg.ctypes.data_as(ctypes.c_void_p) if nch else None, _lib.ptr(face_ids),
                                     _lib.ptr(depth), _lib.ptr(bary), _lib.ptr(image), _lib.ptr(ws), int(ws.shape[0]),
                                     _lib.stream_handle(dev)), "anerf_mesh_raster")
    return MeshRaster(face_ids, depth, bary, image)


def _raster_inputs(vertices, triangles, attrs, who):
    v = torch.as_tensor(vertices)
    t = _device_triangles(triangles, int(v.shape[0]), who)
    dev = t.device
    p = v.to(dev, torch.float32).contiguous()
    a = None if attrs is None else torch.as_tensor(attrs).to(dev, torch.float32).contiguous()
    return p, t, a


@torch.no_grad()
def rasterize_mesh(vertices, triangles, transform, width, height, attrs=None, background=1.0):
    """One orthographic (affine) view of a mesh (vertices float [V, 3], triangles int [T, 3]) on the device.
    `transform` float [3, 4] (host) maps a vertex to (pixel x, pixel y downward, depth): pixel (row j, column i) has
    its centre at (i + 0.5, j + 0.5), smaller depths are nearer, and only depths in [0, 1] are drawn.  Returns
    MeshRaster of device tensors:
      face_ids int32 [H, W]    the nearest triangle covering the pixel's centre (equal depths: the smaller id), or -1;
      depth float32 [H, W]     its depth there, +inf where empty;
      bary float32 [H, W, 3]   its barycentric weights there, 0 where empty;
      image float32 [H, W, C]  `attrs` float [V, C] (1 <= C <= 8) interpolated with them, `background` (one value or
                               C) where empty; None without `attrs`.
    Both windings are drawn (no back-face culling, as in the reference's viewer); a triangle with a vertex that maps
    to a non-finite value or beyond 2^20 pixels is dropped whole.  The contract (include/anerf.h) is
    integers wherever a decision is taken, so the result does not depend on the schedule and is bit for bit that of
    `rasterize_mesh_reference`.  Triangles whose clipped bounding box holds more than RASTER_SMALL_PIXELS pixel
    centres are drawn by whole workgroups, smaller ones by one thread each: the same bits either way.
    ValueError before anything is launched: ids outside [0, V), width or height outside [1, 16384], attrs rows != V.
    Four launches on the current stream, no host read.  Perspective cameras: `rasterize_mesh_camera`.  Out of scope:
    multisampling, writing image files."""
    shape = tuple(vertices.shape) if hasattr(vertices, "shape") else np.shape(vertices)
    ashape = None if attrs is None else (tuple(attrs.shape) if hasattr(attrs, "shape") else np.shape(attrs))
    A, nch, bg = _raster_args(shape, transform, width, height, ashape, background, "rasterize_mesh")
    p, t, a = _raster_inputs(vertices, triangles, attrs, "rasterize_mesh")
    width, height = int(width), int(height)
    with torch.cuda.device(t.device):
        need = _lib.workspace("anerf_mesh_raster_workspace", int(p.shape[0]), int(t.shape[0]), width, height)
        ws = torch.empty(need, device=t.device, dtype=torch.uint8)
        return _raster_launch(p, t, A, width, height, a, nch, bg, ws)


_RASTER_CHUNK = 1 << 21  # candidate fragments per pass of the checker
_EMPTY_KEY = np.uint64(0xffffffffffffffff)


def _boxes_reference(X, Y, W, H):
    """Of triangles snapped to X, Y (int64 [T, 3]): twice the area made positive, whether it was negative, and the
    pixel columns i0 .. i1 and rows j0 .. j1 whose centres the bounding box holds, clipped to the image."""
    a2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    i0 = np.maximum((X.min(1) - 128 + 255) >> 8, 0)
    i1 = np.minimum((X.max(1) - 128) >> 8, W - 1)
    j0 = np.maximum((Y.min(1) - 128 + 255) >> 8, 0)
    j1 = np.minimum((Y.max(1) - 128) >> 8, H - 1)
    return np.abs(a2), a2 < 0, i0, i1, j0, j1


def _candidates_reference(live, i0, i1, j0, j1):
    """The candidate fragments (triangle, column, row) of the triangles `live` over their boxes, a bounded number at
    a time (a larger box: a pass of its own)."""
    bw = (i1 - i0 + 1)[live]
    box = bw * (j1 - j0 + 1)[live]
    start = 0
    while start < len(live):
        end = start + max(1, int(np.searchsorted(np.cumsum(box[start:]), _RASTER_CHUNK, side="right")))
        sel, n = live[start:end], box[start:end]
        tid = np.repeat(sel, n)
        k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
        w = np.repeat(bw[start:end], n)
        yield tid, i0[tid] + k % w, j0[tid] + k // w
        start = end


def _coverage_reference(X, Y, a2, flip, tid, i, j):
    """The contract's coverage of triangles `tid` at pixels (i, j) (arrays of one length), shared by the affine and
    the perspective checker: (inside, b0, b1, b2)."""
    px, py = 256 * i + 128, 256 * j + 128
    inside = np.ones(len(tid), bool)
    E = {}
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = X[tid, b] - X[tid, a], Y[tid, b] - Y[tid, a]
        e = dx * (py - Y[tid, a]) - dy * (px - X[tid, a])
        sgn = np.where(flip[tid], -1, 1)
        e, dx, dy = e * sgn, dx * sgn, dy * sgn
        inside &= (e > 0) | ((e == 0) & ((dy > 0) | ((dy == 0) & (dx < 0))))
        E[(a, b)] = e
    with np.errstate(all="ignore"):
        area = a2[tid].astype(_F)
        b1 = E[(2, 0)].astype(_F) / area
        b2 = E[(0, 1)].astype(_F) / area
        b0 = (_F(1) - b1) - b2
    return inside, b0, b1, b2


def _fragments_reference(X, Y, z, a2, flip, tid, i, j):
    """The contract's fragment of triangles `tid` at pixels (i, j) (arrays of one length): (ok, b0, b1, b2, z)."""
    inside, b0, b1, b2 = _coverage_reference(X, Y, a2, flip, tid, i, j)
    with np.errstate(all="ignore"):
        zz = (b0 * z[tid, 0] + b1 * z[tid, 1]) + b2 * z[tid, 2]
        ok = inside & (zz >= 0) & (zz <= 1)
    zz = np.where(zz == 0, _F(0), zz).astype(_F)
    return ok, b0, b1, b2, zz


def rasterize_mesh_reference(vertices, triangles, transform, width, height, attrs=None, background=1.0):
    """NumPy implementation of `rasterize_mesh`'s contract: its checker.  Returns MeshRaster of arrays."""
    p = np.ascontiguousarray(_lib.host_array(vertices), dtype=_F)
    a = None if attrs is None else np.ascontiguousarray(_lib.host_array(attrs), dtype=_F)
    A, nch, bg = _raster_args(p.shape, transform, width, height, None if a is None else a.shape, background,
                              "rasterize_mesh_reference")
    W, H = int(width), int(height)
    tri = _host_triangles(triangles, len(p), "rasterize_mesh_reference")
    keys = np.full(H * W, _EMPTY_KEY, np.uint64)
    nt = len(tri)
    if nt:
        with np.errstate(all="ignore"):
            s = np.stack([((A[r, 0] * p[:, 0] + A[r, 1] * p[:, 1]) + A[r, 2] * p[:, 2]) + A[r, 3]
                          for r in range(3)], -1)
            s = s.astype(_F)[tri]  # [T, 3 vertices, 3]
            good = np.isfinite(s).all(axis=(1, 2)) & (np.abs(s[..., :2]) <= _F(2.0 ** 20)).all(axis=(1, 2))
            s = np.where(good[:, None, None], s, _F(0))
            X = np.rint(s[..., 0] * _F(256)).astype(np.int64)
            Y = np.rint(s[..., 1] * _F(256)).astype(np.int64)
        z = np.ascontiguousarray(s[..., 2])
        a2, flip, i0, i1, j0, j1 = _boxes_reference(X, Y, W, H)
        live = np.nonzero(good & (a2 != 0) & (i0 <= i1) & (j0 <= j1))[0]
        for tid, i, j in _candidates_reference(live, i0, i1, j0, j1):
            ok, _, _, _, zz = _fragments_reference(X, Y, z, a2, flip, tid, i, j)
            key = (zz[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | tid[ok].astype(np.uint64)
            np.minimum.at(keys, (j[ok] * W + i[ok]), key)
    hit = np.nonzero(keys != _EMPTY_KEY)[0]
    face_ids = np.full(H * W, -1, np.int32)
    depth = np.full(H * W, np.inf, _F)
    bary = np.zeros((H * W, 3), _F)
    image = None if a is None else np.tile(bg, (H * W, 1)).astype(_F)
    if len(hit):
        tid = (keys[hit] & np.uint64(0xffffffff)).astype(np.int64)
        ok, b0, b1, b2, zz = _fragments_reference(X, Y, z, a2, flip, tid, hit % W, hit // W)
        assert ok.all()
        face_ids[hit] = tid
        depth[hit] = zz
        bary[hit] = np.stack([b0, b1, b2], -1)
        if a is not None:
            with np.errstate(all="ignore"):
                a0, a1, a2_ = a[tri[tid, 0]], a[tri[tid, 1]], a[tri[tid, 2]]
                image[hit] = (b0[:, None] * a0 + b1[:, None] * a1) + b2[:, None] * a2_
    return MeshRaster(face_ids.reshape(H, W), depth.reshape(H, W), bary.reshape(H, W, 3),
                      None if image is None else image.reshape(H, W, nch))


# ------------------------------------------------------------------ turntable
def _bounding_box(vertices):
    """(min, max) float64 [3] over the finite vertices (one read); a mesh without any: the origin."""
    if isinstance(vertices, torch.Tensor):
        v = vertices.reshape(-1, 3)
        v = v[torch.isfinite(v).all(-1)]
        if v.shape[0] == 0:
            return np.zeros(3), np.zeros(3)
        box = torch.stack([v.amin(0), v.amax(0)]).double().cpu().numpy()  # (the one read)
        return box[0], box[1]
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(-1)]
    if len(v) == 0:
        return np.zeros(3), np.zeros(3)
    return v.min(0), v.max(0)


def turntable_transforms(vertices, frames=91, step_deg=4.0, width=512, height=512, up=(0, 0, 1), ortho_ratio=1.2):
    """The [F, 3, 4] float32 matrices (a host array) of `mesh_turntable`'s views, for `rasterize_mesh`: the framing of
    the reference's viewer, in float64 on the vertices' bounding box, cast to float32 at the end.
      * the box's centre goes to the origin and the mesh is scaled by 1 / (the box's extent along `up`);
      * the camera is orthographic, its window `ortho_ratio` wide and ortho_ratio * height / width high (the body,
        of height 1, fills 1 / ortho_ratio of a square image), `up` pointing up the image; at frame 0 it looks along
        u x r, r the coordinate axis least aligned with `up`, made orthogonal to it (up = z: from -y, x to the right);
      * frame k has the mesh turned about `up` by k * step_deg degrees;
      * depth: the scaled mesh lies within its box's half-diagonal rho of the origin; the signed distance along the
        viewing direction in [-rho, rho] is mapped to [0.1, 0.9], so nothing is cut by the [0, 1] depth range."""
    if int(frames) != frames or frames < 0:
        raise ValueError(f"turntable_transforms: frames must be an integer >= 0, got {frames}")
    u = np.asarray(up, dtype=np.float64).reshape(-1)
    if u.size != 3 or not np.isfinite(u).all() or not np.linalg.norm(u) > 0:
        raise ValueError(f"turntable_transforms: up must be a non-zero direction (x, y, z), got {up!r}")
    if not (np.isfinite(ortho_ratio) and ortho_ratio > 0):
        raise ValueError(f"turntable_transforms: ortho_ratio must be positive, got {ortho_ratio}")
    u = u / np.linalg.norm(u)
    lo, hi = _bounding_box(vertices)
    centre = 0.5 * (lo + hi)
    extent = float(np.abs(u) @ (hi - lo))
    scale = 1.0 / extent if extent > 0 else 1.0
    rho = 0.5 * float(np.linalg.norm(hi - lo)) * scale
    rho = rho if rho > 0 else 1.0
    e = np.zeros(3)
    e[int(np.argmin(np.abs(u)))] = 1.0
    r = e - (e @ u) * u
    r = r / np.linalg.norm(r)
    view = np.cross(u, r)  # the viewing direction at frame 0: depth grows along it
    ppu = float(width) / float(ortho_ratio)  # pixels per unit
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    out = np.zeros((int(frames), 3, 4))
    for k in range(int(frames)):
        th = np.radians(k * float(step_deg))
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)  # the mesh turned about u
        M = np.stack([ppu * r, -ppu * u, view / (2.5 * rho)]) @ R * scale  # rows: pixel x, pixel y, depth
        out[k, :, :3] = M
        out[k, :, 3] = np.array([0.5 * width, 0.5 * height, 0.5]) - M @ centre
    return out.astype(_F)


def _to_uint8_reference(image):
    with np.errstate(invalid="ignore"):
        x = np.rint(_F(255) * np.clip(np.nan_to_num(image.astype(_F), nan=0.0), _F(0), _F(1)))
    return x.astype(np.uint8)


def _to_uint8(image):
    return torch.round(torch.nan_to_num(image, nan=0.0).clamp_(0.0, 1.0).mul_(255.0)).to(torch.uint8)


def _turntable_colors(colors, n_vertices, who, normals):
    """The per-vertex colours float32 [V, 3] in [0, 1]: given (uint8: c * fl(1 / 255)), or 0.5 n + 0.5 of normals()."""
    if colors is None:
        n = normals()
        return n * 0.5 + 0.5
    c = colors if isinstance(colors, torch.Tensor) else np.asarray(colors)
    if tuple(c.shape) != (n_vertices, 3):
        raise ValueError(f"{who}: colors of shape {tuple(c.shape)} for {n_vertices} vertices ([V, 3] wanted)")
    if c.dtype in (torch.uint8, np.uint8):
        # (times fl(1 / 255), not a division: a product is rounded the same way everywhere; rint(255 x) gives c back)
        return (c.to(torch.float32) if isinstance(c, torch.Tensor) else c.astype(_F)) * float(_F(1.0 / 255.0))
    return c


@torch.no_grad()
def mesh_turntable(vertices, triangles, colors=None, frames=91, step_deg=4.0, width=512, height=512, up=(0, 0, 1),
                   ortho_ratio=1.2, background=1.0):
    """The reference viewer's turntable of a mesh, on the device: uint8 [F, H, W, 3] (a device tensor), frame k the
    mesh turned about `up` by k * step_deg degrees in `turntable_transforms`' framing (91 frames of 4 degrees: the
    viewer's 0 .. 360).  `colors`: None colours by normal, 0.5 * vertex_normals(vertices, triangles) + 0.5 as the
    viewer does (the normals of the mesh as given, computed once: the colours turn with the mesh, where the viewer
    recomputes them in every frame's camera space); or float [V, 3] in [0, 1], or uint8 [V, 3] (extract_mesh's
    attrs["colors"], a PLY's), used as given.  `background`: one value or three, in [0, 1].  A float image x becomes
    rint(255 clamp(x, 0, 1)).  One rasterize_mesh (anerf_mesh_raster) per frame on the current stream; the only host
    read is the bounding box.  Writing the frames to image files is left to the caller."""
    v = torch.as_tensor(vertices)
    _check_vertices(tuple(v.shape), "mesh_turntable")
    nv = int(v.shape[0])
    t = _device_triangles(triangles, nv, "mesh_turntable")
    dev = t.device
    width, height = int(width), int(height)
    with torch.cuda.device(dev):
        p = v.to(dev, torch.float32).contiguous()
        c = _turntable_colors(colors, nv, "mesh_turntable", lambda: _vertex_normals(p, t))
        c = torch.as_tensor(c).to(dev, torch.float32).contiguous()
        Ts = turntable_transforms(p, frames, step_deg, width, height, up, ortho_ratio)
        A0, nch, bg = _raster_args((nv, 3), np.zeros((3, 4), _F), width, height, (nv, 3), background, "mesh_turntable")
        need = _lib.workspace("anerf_mesh_raster_workspace", nv, int(t.shape[0]), width, height)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        out = torch.empty((len(Ts), height, width, 3), device=dev, dtype=torch.uint8)
        for k in range(len(Ts)):
            img = _raster_launch(p, t, np.ascontiguousarray(Ts[k]), width, height, c, nch, bg, ws).image
            out[k] = _to_uint8(img)
    return out


def mesh_turntable_reference(vertices, triangles, colors=None, frames=91, step_deg=4.0, width=512, height=512,
                             up=(0, 0, 1), ortho_ratio=1.2, background=1.0):
    """NumPy implementation of `mesh_turntable` on the checkers: uint8 [F, H, W, 3] as an array."""
    p = np.ascontiguousarray(_lib.host_array(vertices), dtype=_F)
    _check_vertices(p.shape, "mesh_turntable_reference")
    c = _turntable_colors(None if colors is None else _lib.host_array(colors), len(p), "mesh_turntable_reference",
                          lambda: vertex_normals_reference(p, triangles))
    c = np.asarray(c, dtype=_F)
    Ts = turntable_transforms(p, frames, step_deg, width, height, up, ortho_ratio)
    out = np.zeros((len(Ts), int(height), int(width), 3), np.uint8)
    for k in range(len(Ts)):
        out[k] = _to_uint8_reference(rasterize_mesh_reference(p, triangles, Ts[k], width, height, c, background).image)
    return out


# ------------------------------------------------------------------ the dataset's perspective cameras
def _focal_pair(focal, who):
    f = np.asarray(focal, dtype=np.float64).reshape(-1)  # (a scalar or a pair, as rays._intrinsic takes it)
    if f.size not in (1, 2):
        raise ValueError(f"{who}: focal must be one value or (fx, fy), got {f.size} values")
    return float(f[0]), float(f[-1])


def camera_view(c2w, H, W, focal, center=None):
    """(view float32 [3, 4], intrinsics float32 [4] = fx, fy, cx, cy), host arrays, of the camera that `render_path`,
    `gen_rays` and the dataset describe by `c2w` (camera to world, [3, 4] or [4, 4]: x right, y up, looking along
    -z), `H, W, focal` (one value or (fx, fy)) and `center` (the principal point's offsets (x, y); None: W / 2,
    H / 2), for `rasterize_mesh_camera`.  In float64, cast at the end: with R = c2w[:3, :3] the rows of view are
    R[:, 0], -R[:, 1], -R[:, 2] (right, down the image, along the optical axis), its translation -rows @ c2w[:3, 3];
    cx = offset_x + 0.5, cy = offset_y + 0.5.  The centre of pixel (row j, column i), at (i + 0.5, j + 0.5), is then
    the ray that get_rays / anerf_gen_rays cast for that pixel, dirs = ((i - offset_x) / fx, -(j - offset_y) / fy, -1),
    and because that direction has unit depth the ray's parameter at the surface is the raster's depth[j, i]."""
    c = np.asarray(_lib.host_array(c2w), dtype=np.float64)
    if c.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"camera_view: c2w must be [3, 4] or [4, 4], got shape {c.shape}")
    fx, fy = _focal_pair(focal, "camera_view")
    if center is None:
        ox, oy = 0.5 * float(W), 0.5 * float(H)
    else:
        o = np.asarray(_lib.host_array(center), dtype=np.float64).reshape(-1)
        if o.size != 2:
            raise ValueError(f"camera_view: center must be (x, y), got {o.size} values")
        ox, oy = float(o[0]), float(o[1])
    R = c[:3, :3]
    rows = np.stack([R[:, 0], -R[:, 1], -R[:, 2]])
    view = np.concatenate([rows, (-rows @ c[:3, 3])[:, None]], 1)
    return np.ascontiguousarray(view, dtype=_F), np.array([fx, fy, ox + 0.5, oy + 0.5], dtype=_F)


def _camera_range(box, c2w, near, far, who):
    """(near, far) as float32 values: those given, or from the vertices' bounding box `box` = (min, max) in float64 --
    D the camera's distance to the box's centre, rho its half-diagonal (1 for a box without extent):
    near = max(D - rho, 1e-3 rho), far = D + rho."""
    if near is None or far is None:
        lo, hi = box
        eye = np.asarray(_lib.host_array(c2w), dtype=np.float64)[:3, 3]
        rho = 0.5 * float(np.linalg.norm(hi - lo))
        rho = rho if rho > 0 else 1.0
        D = float(np.linalg.norm(eye - 0.5 * (lo + hi)))
        near = max(D - rho, 1e-3 * rho) if near is None else near
        far = D + rho if far is None else far
    near, far = _F(near), _F(far)
    if not (np.isfinite(near) and near > 0):
        raise ValueError(f"{who}: near must be finite and > 0, got {near}")
    if not (np.isfinite(far) and far >= near):
        raise ValueError(f"{who}: far must be finite and >= near ({near}), got {far}")
    return near, far


def _persp_args(vertices_shape, view, intrinsics, width, height, attrs_shape, background, who):
    """The argument errors of the perspective rasteriser and its checker: (view float32 [3, 4], intrinsics float32
    [4], C, background float32 [C])."""
    _, nch, bg = _raster_args(vertices_shape, np.zeros((3, 4), _F), width, height, attrs_shape, background, who)
    V = np.ascontiguousarray(_lib.host_array(view), dtype=_F)
    K = np.ascontiguousarray(_lib.host_array(intrinsics), dtype=_F).reshape(-1)
    if V.shape != (3, 4):
        raise ValueError(f"{who}: view must be [3, 4], got shape {V.shape}")
    if K.shape != (4,) or not np.isfinite(K).all() or K[0] == 0 or K[1] == 0:
        raise ValueError(f"{who}: intrinsics must be finite (fx, fy, cx, cy) with fx, fy != 0, got {K}")
    return V, K, nch, bg


def _raster_persp_launch(p, t, V, K, near, far, width, height, a, nch, bg, ws):
    """One anerf_mesh_raster_persp call on checked device tensors (ws: its workspace, reusable between frames)."""
    dev = t.device
    lib = _lib.load()
    face_ids = torch.empty((height, width), device=dev, dtype=torch.int32)
    depth = torch.empty((height, width), device=dev, dtype=torch.float32)
    bary = torch.empty((height, width, 3), device=dev, dtype=torch.float32)
    image = torch.empty((height, width, nch), device=dev, dtype=torch.float32) if nch else None
    _lib.check(lib.anerf_mesh_raster_persp(_lib.ptr(p), int(p.shape[0]), _lib.ptr(t), int(t.shape[0]),
                                           V.ctypes.data_as(ctypes.c_void_p), K.ctypes.data_as(ctypes.c_void_p),
                                           float(near), float(far), width, height, _lib.ptr(a), nch,
                                           bg.ctypes.data_as(ctypes.c_void_p) if nch else None, _lib.ptr(face_ids),
                                           _lib.ptr(depth), _lib.ptr(bary), _lib.ptr(image), _lib.ptr(ws),
                                           int(ws.shape[0]), _lib.stream_handle(dev)), "anerf_mesh_raster_persp")
    return MeshRaster(face_ids, depth, bary, image)


def _shape(x):
    return None if x is None else (tuple(x.shape) if hasattr(x, "shape") else np.shape(x))


@torch.no_grad()
def rasterize_mesh_camera(vertices, triangles, c2w, H, W, focal, center=None, near=None, far=None, attrs=None,
                          background=1.0):
    """One view of a mesh (vertices float [V, 3], triangles int [T, 3]) on the device through the perspective camera
    `c2w, H, W, focal, center` of `camera_view` -- the camera of render_path, gen_rays and the dataset, so the mesh is
    drawn where the field is rendered.  Returns MeshRaster of device tensors, as `rasterize_mesh` does, with
      face_ids  the ORIGINAL triangle's id (a triangle cut by the near plane keeps it);
      depth     the camera depth of the surface at the pixel's centre: the parameter of that pixel's get_rays ray, to
                set against the depth of render_rays; +inf where empty;
      bary      perspective-correct weights over the triangle's three original vertices;
      image     `attrs` under them.
    Only depths in [near, far] are drawn: a triangle across the near plane is cut there (neighbours get the same cut
    points bit for bit: no cracks), fragments beyond far are discarded.  near / far None: from the vertices' bounding
    box (one host read), D the camera's distance to its centre and rho its half-diagonal, near = max(D - rho,
    1e-3 rho), far = D + rho.  The contract (include/anerf.h) keeps every decision on integers: the result
    does not depend on the schedule and is bit for bit that of `rasterize_mesh_camera_reference`.  ValueError before
    anything is launched: rasterize_mesh's cases, near not finite or <= 0, far not finite or < near, a focal of 0.
    Four launches on the current stream.  Out of scope: side-plane clipping (a triangle reaching beyond 2^20 pixels is
    dropped, not cut), multisampling, back-face culling, writing image files."""
    who = "rasterize_mesh_camera"
    V, K = camera_view(c2w, H, W, focal, center)
    V, K, nch, bg = _persp_args(_shape(vertices), V, K, W, H, _shape(attrs), background, who)
    if near is not None and far is not None:
        near, far = _camera_range(None, c2w, near, far, who)
    p, t, a = _raster_inputs(vertices, triangles, attrs, who)
    width, height = int(W), int(H)
    with torch.cuda.device(t.device):
        if near is None or far is None:
            near, far = _camera_range(_bounding_box(p), c2w, near, far, who)
        need = _lib.workspace("anerf_mesh_raster_persp_workspace", int(p.shape[0]), int(t.shape[0]), width, height)
        ws = torch.empty(need, device=t.device, dtype=torch.uint8)
        return _raster_persp_launch(p, t, V, K, near, far, width, height, a, nch, bg, ws)


def _persp_polygons_reference(ct, near):
    """The near-plane cut of the contract on camera-space triangles ct float32 [T, 3, 3] (xc, yc, d), all finite:
    (nq int [T]: 0, 3 or 4 polygon vertices; Q float32 [T, 4, 3]; rows float32 [T, 4, 3] over the ORIGINAL vertices)."""
    T = len(ct)
    ar = np.arange(T)
    IN = ct[..., 2] >= near
    n_in = IN.sum(1)
    s = np.zeros(T, np.int64)  # the IN vertex whose predecessor is not IN (0 when all or none are IN)
    for k in range(3):
        s = np.where(IN[:, k] & ~IN[:, (k + 2) % 3], k, s)
    r = (s[:, None] + np.arange(3)) % 3
    rot = ct[ar[:, None], r]  # the vertices from s on, in the triangle's order
    unit = np.eye(3, dtype=_F)

    def cut(i, o):  # from the IN end i to the OUT end o (places in `rot`)
        t = (rot[:, i, 2] - near) / (rot[:, i, 2] - rot[:, o, 2])
        q = np.stack([rot[:, i, 0] + t * (rot[:, o, 0] - rot[:, i, 0]),
                      rot[:, i, 1] + t * (rot[:, o, 1] - rot[:, i, 1]), np.full(T, near, _F)], -1)
        row = np.zeros((T, 3), _F)
        row[:, i] = _F(1) - t
        row[:, o] = t
        return q.astype(_F), row

    with np.errstate(all="ignore"):
        c01, c02, c12 = cut(0, 1), cut(0, 2), cut(1, 2)
    one, two = (n_in == 1)[:, None], (n_in == 2)[:, None]
    Q = np.zeros((T, 4, 3), _F)
    rows = np.zeros((T, 4, 3), _F)  # over the places in `rot`
    Q[:, 0], rows[:, 0] = rot[:, 0], unit[0]
    Q[:, 1], rows[:, 1] = np.where(one, c01[0], rot[:, 1]), np.where(one, c01[1], unit[1])
    Q[:, 2] = np.where(one, c02[0], np.where(two, c12[0], rot[:, 2]))
    rows[:, 2] = np.where(one, c02[1], np.where(two, c12[1], unit[2]))
    Q[:, 3], rows[:, 3] = c02[0], c02[1]
    back = np.empty_like(rows)  # place k of `rot` is the original vertex r[:, k]
    for k in range(3):
        back[ar, :, r[:, k]] = rows[:, :, k]
    nq = np.where(n_in == 0, 0, np.where(n_in == 2, 4, 3))
    return nq, Q, back


_PERSP_SUBS = ((0, 1, 2), (0, 2, 3))  # the fan of the cut polygon


def _persp_fragments_reference(X, Y, iw, a2, flip, far, sid, i, j):
    """The contract's fragment of sub-triangles `sid` at pixels (i, j): (ok, u [n, 3], dep)."""
    inside, b0, b1, b2 = _coverage_reference(X, Y, a2, flip, sid, i, j)
    with np.errstate(all="ignore"):
        u = np.stack([b0 * iw[sid, 0], b1 * iw[sid, 1], b2 * iw[sid, 2]], -1).astype(_F)
        dep = (_F(1) / ((u[:, 0] + u[:, 1]) + u[:, 2])).astype(_F)
        ok = inside & (dep > 0) & (dep <= far)
    return ok, u, dep


def _persp_setup_reference(p, tri, V, K, near, W, H):
    """The contract's set-up of all 2 T sub-triangles (2 t + m is sub-triangle m of triangle t): snapped X, Y int64
    [2 T, 3], iw float32 [2 T, 3], rows float32 [2 T, 3, 3] over the original vertices, a2, flip, the boxes i0, i1, j0,
    j1, and draws bool [2 T]: the sub-triangle exists, has an area and a pixel centre in its box."""
    nt = len(tri)
    with np.errstate(all="ignore"):
        c = np.stack([((V[k, 0] * p[:, 0] + V[k, 1] * p[:, 1]) + V[k, 2] * p[:, 2]) + V[k, 3]
                      for k in range(3)], -1).astype(_F)[tri]  # [T, 3 vertices, (xc, yc, d)]
        finite = np.isfinite(c).all(axis=(1, 2))
        nq, Q, rows = _persp_polygons_reference(np.where(finite[:, None, None], c, _F(0)), near)
        nq = np.where(finite, nq, 0)
        s0 = K[0] * (Q[..., 0] / Q[..., 2]) + K[2]
        s1 = K[1] * (Q[..., 1] / Q[..., 2]) + K[3]
        iw4 = (_F(1) / Q[..., 2]).astype(_F)
        used = np.arange(4)[None] < nq[:, None]
        fine = (np.isfinite(s0) & np.isfinite(s1) & np.isfinite(iw4) & (np.abs(s0) <= _F(2.0 ** 20)) &
                (np.abs(s1) <= _F(2.0 ** 20)))
        good = (nq > 0) & (fine | ~used).all(1)
        keep = good[:, None] & used
        X4 = np.rint(np.where(keep, s0, _F(0)).astype(_F) * _F(256)).astype(np.int64)
        Y4 = np.rint(np.where(keep, s1, _F(0)).astype(_F) * _F(256)).astype(np.int64)
    sub = np.array(_PERSP_SUBS)
    X, Y = X4[:, sub].reshape(2 * nt, 3), Y4[:, sub].reshape(2 * nt, 3)
    iw = np.ascontiguousarray(iw4[:, sub].reshape(2 * nt, 3))
    srows = rows[:, sub].reshape(2 * nt, 3, 3)
    exists = (good[:, None] & (np.array([3, 4])[None] <= nq[:, None])).reshape(-1)
    a2, flip, i0, i1, j0, j1 = _boxes_reference(X, Y, W, H)
    draws = exists & (a2 != 0) & (i0 <= i1) & (j0 <= j1)
    return X, Y, iw, srows, a2, flip, i0, i1, j0, j1, draws


def _raster_persp_reference(p, tri, V, K, near, far, W, H, a, nch, bg):
    """The checker on checked host arrays: MeshRaster of arrays."""
    keys = np.full(H * W, _EMPTY_KEY, np.uint64)
    nt = len(tri)
    if nt:
        X, Y, iw, srows, a2, flip, i0, i1, j0, j1, draws = _persp_setup_reference(p, tri, V, K, near, W, H)
        for sid, i, j in _candidates_reference(np.nonzero(draws)[0], i0, i1, j0, j1):
            ok, _, dep = _persp_fragments_reference(X, Y, iw, a2, flip, far, sid, i, j)
            key = (dep[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (sid[ok] >> 1).astype(np.uint64)
            np.minimum.at(keys, (j[ok] * W + i[ok]), key)
    hit = np.nonzero(keys != _EMPTY_KEY)[0]
    face_ids = np.full(H * W, -1, np.int32)
    depth = np.full(H * W, np.inf, _F)
    bary = np.zeros((H * W, 3), _F)
    image = None if a is None else np.tile(bg, (H * W, 1)).astype(_F)
    if len(hit):
        tid = (keys[hit] & np.uint64(0xffffffff)).astype(np.int64)
        bits = (keys[hit] >> np.uint64(32)).astype(np.uint32)
        done = np.zeros(len(hit), bool)
        B = np.zeros((len(hit), 3), _F)
        dd = np.zeros(len(hit), _F)
        for m in range(2):  # the first sub-triangle that reproduces the key
            sid = 2 * tid + m
            ok, u, dep = _persp_fragments_reference(X, Y, iw, a2, flip, far, sid, hit % W, hit // W)
            ok &= draws[sid] & (dep.view(np.uint32) == bits) & ~done
            with np.errstate(all="ignore"):
                g = (u * dep[:, None]).astype(_F)
                r = srows[sid]
                Bm = (g[:, 0, None] * r[:, 0] + g[:, 1, None] * r[:, 1]) + g[:, 2, None] * r[:, 2]
            B[ok], dd[ok] = Bm[ok], dep[ok]
            done |= ok
        assert done.all()
        face_ids[hit] = tid
        depth[hit] = dd
        bary[hit] = B
        if a is not None:
            with np.errstate(all="ignore"):
                a0, a1, a2_ = a[tri[tid, 0]], a[tri[tid, 1]], a[tri[tid, 2]]
                image[hit] = (B[:, 0, None] * a0 + B[:, 1, None] * a1) + B[:, 2, None] * a2_
    return MeshRaster(face_ids.reshape(H, W), depth.reshape(H, W), bary.reshape(H, W, 3),
                      None if image is None else image.reshape(H, W, nch))


def rasterize_mesh_camera_reference(vertices, triangles, c2w, H, W, focal, center=None, near=None, far=None,
                                    attrs=None, background=1.0):
    """NumPy implementation of `rasterize_mesh_camera`'s contract: its checker.  Returns MeshRaster of arrays."""
    who = "rasterize_mesh_camera_reference"
    p = np.ascontiguousarray(_lib.host_array(vertices), dtype=_F)
    a = None if attrs is None else np.ascontiguousarray(_lib.host_array(attrs), dtype=_F)
    V, K = camera_view(c2w, H, W, focal, center)
    V, K, nch, bg = _persp_args(p.shape, V, K, W, H, None if a is None else a.shape, background, who)
    tri = _host_triangles(triangles, len(p), who)
    near, far = _camera_range(_bounding_box(p) if near is None or far is None else None, c2w, near, far, who)
    return _raster_persp_reference(p, tri, V, K, near, far, int(W), int(H), a, nch, bg)


MeshViews = collections.namedtuple("MeshViews", ["rgb", "depth", "mask"])


def _views_args(c2ws, focal, centers, who):
    """Per frame (c2w, focal, center) of render_mesh_views: focal one value, [F] or [F, 2] (as rays.device_boxes takes
    it; a sequence of F values is read per frame), centers None or [F, 2]."""
    cs = np.asarray(_lib.host_array(c2ws), dtype=np.float64)
    if cs.ndim != 3 or cs.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError(f"{who}: c2ws must be [F, 3, 4] or [F, 4, 4], got shape {cs.shape}")
    F = len(cs)
    f = np.asarray(_lib.host_array(focal), dtype=np.float64)
    if f.ndim == 0:
        f = np.full(F, float(f))
    if f.shape not in ((F,), (F, 2)):
        raise ValueError(f"{who}: focal must be one value, [{F}] or [{F}, 2], got shape {f.shape}")
    ce = None if centers is None else np.asarray(_lib.host_array(centers), dtype=np.float64)
    if ce is not None and ce.shape != (F, 2):
        raise ValueError(f"{who}: centers must be [{F}, 2], got shape {ce.shape}")
    return [(cs[k], f[k], None if ce is None else ce[k]) for k in range(F)]


@torch.no_grad()
def render_mesh_views(vertices, triangles, c2ws, H, W, focal, centers=None, colors=None, near=None, far=None,
                      background=1.0):
    """The mesh at the render cameras: one `rasterize_mesh_camera` per camera of `c2ws` [F, 3, 4] or [F, 4, 4] --
    render_path's poses, the dataset's -- with `focal` one value, [F] or [F, 2] and `centers` None or [F, 2].  Returns
    MeshViews of device tensors: rgb uint8 [F, H, W, 3] to lay over the images, depth float32 [F, H, W] (camera
    depth, +inf where empty) to set against render_rays' depth, mask bool [F, H, W] to set against a dataset mask or
    acc.  `colors` and the conversion to uint8 are mesh_turntable's: None colours by normal (0.5 vertex_normals + 0.5),
    or float [V, 3] in [0, 1], or uint8 [V, 3]; x becomes rint(255 clamp(x, 0, 1)).  near / far None: per camera from
    the one bounding box (rasterize_mesh_camera).  One workspace serves all frames; the bounding box is the only host
    read."""
    who = "render_mesh_views"
    v = torch.as_tensor(vertices)
    _check_vertices(tuple(v.shape), who)
    nv = int(v.shape[0])
    cams = _views_args(c2ws, focal, centers, who)
    _, nch, bg = _raster_args((nv, 3), np.zeros((3, 4), _F), W, H, (nv, 3), background, who)
    t = _device_triangles(triangles, nv, who)
    dev = t.device
    width, height = int(W), int(H)
    with torch.cuda.device(dev):
        p = v.to(dev, torch.float32).contiguous()
        c = _turntable_colors(colors, nv, who, lambda: _vertex_normals(p, t))
        c = torch.as_tensor(c).to(dev, torch.float32).contiguous()
        box = _bounding_box(p) if near is None or far is None else None
        need = _lib.workspace("anerf_mesh_raster_persp_workspace", nv, int(t.shape[0]), width, height)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        rgb = torch.empty((len(cams), height, width, 3), device=dev, dtype=torch.uint8)
        depth = torch.empty((len(cams), height, width), device=dev, dtype=torch.float32)
        mask = torch.empty((len(cams), height, width), device=dev, dtype=torch.bool)
        for k, (c2w, f, centre) in enumerate(cams):
            V, K = camera_view(c2w, height, width, f, centre)
            V, K, _, _ = _persp_args((nv, 3), V, K, width, height, None, 0.0, who)
            nr, fr = _camera_range(box, c2w, near, far, who)
            r = _raster_persp_launch(p, t, V, K, nr, fr, width, height, c, nch, bg, ws)
            rgb[k] = _to_uint8(r.image)
            depth[k] = r.depth
            mask[k] = r.face_ids >= 0
    return MeshViews(rgb, depth, mask)


def render_mesh_views_reference(vertices, triangles, c2ws, H, W, focal, centers=None, colors=None, near=None,
                                far=None, background=1.0):
    """NumPy implementation of `render_mesh_views` on the checkers: MeshViews of arrays."""
    who = "render_mesh_views_reference"
    p = np.ascontiguousarray(_lib.host_array(vertices), dtype=_F)
    _check_vertices(p.shape, who)
    cams = _views_args(c2ws, focal, centers, who)
    c = _turntable_colors(None if colors is None else _lib.host_array(colors), len(p), who,
                          lambda: vertex_normals_reference(p, triangles))
    c = np.asarray(c, dtype=_F)
    rgb = np.zeros((len(cams), int(H), int(W), 3), np.uint8)
    depth = np.zeros((len(cams), int(H), int(W)), _F)
    mask = np.zeros((len(cams), int(H), int(W)), bool)
    for k, (c2w, f, centre) in enumerate(cams):
        r = rasterize_mesh_camera_reference(p, triangles, c2w, H, W, f, centre, near, far, c, background)
        rgb[k], depth[k], mask[k] = _to_uint8_reference(r.image), r.depth, r.face_ids >= 0
    return MeshViews(rgb, depth, mask)


# ------------------------------------------------------------------ vertex clustering
def _simplify_args(vertices_shape, triangles, cell, origin, attrs, who):
    """The argument errors of simplify_mesh and its checker that need no look at the data: (cell float32, the given
    origin float32 [3] or None)."""
    _check_vertices(vertices_shape, who)
    shape = tuple(triangles.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{who}: triangles must be [T, 3], got shape {shape}")
    if str(triangles.dtype).split(".")[-1] not in ("int32", "int64"):  # (a tensor's or an array's)
        raise ValueError(f"{who}: triangles must be int32 or int64, got {triangles.dtype}")
    nv = vertices_shape[0]
    if nv > 0x7fffffff or shape[0] > 0x7fffffff:
        raise ValueError(f"{who}: {nv} vertices / {shape[0]} triangles do not fit int32 ids")
    with np.errstate(all="ignore"):
        c = _F(cell)
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"{who}: cell must be finite and > 0 (as float32), got {cell}")
    o = None
    if origin is not None:
        o = np.ascontiguousarray(_lib.host_array(origin), dtype=_F).reshape(-1)
        if o.size != 3 or not np.isfinite(o).all():
            raise ValueError(f"{who}: origin must be three finite values (x, y, z), got {origin!r}")
    _gather_attrs(attrs, lambda a: None, nv, who)  # (the row counts)
    return c, o


def _simplify_grid(lo, hi, finite, tri_lo, tri_hi, n_vertices, cell, origin, who):
    """The errors that need the one look at the data (the vertices' per-axis minimum and maximum, whether all are
    finite, the smallest and largest triangle id or None), and the grid: (origin float32 [3], dims int32 [3])."""
    if tri_lo is not None and (tri_lo < 0 or tri_hi >= n_vertices):
        raise ValueError(f"{who}: vertex ids span [{int(tri_lo)}, {int(tri_hi)}], outside [0, {n_vertices})")
    if not finite:
        raise ValueError(f"{who}: the vertices must be finite, found a NaN or infinite coordinate")
    lo, hi = np.asarray(lo, dtype=_F), np.asarray(hi, dtype=_F)
    o = lo if origin is None else origin
    if (lo < o).any():
        raise ValueError(f"{who}: a vertex lies below the origin {tuple(float(x) for x in o)}: the minimum is "
                         f"{tuple(float(x) for x in lo)}")
    with np.errstate(all="ignore"):
        top = np.floor((hi - o) / cell)  # float32, the arithmetic of the contract: the largest cell index per axis
    cells = 1
    for x in top:
        cells = cells * (int(x) + 1) if np.isfinite(x) and cells <= SIMPLIFY_MAX_CELLS else SIMPLIFY_MAX_CELLS + 1
    if cells > SIMPLIFY_MAX_CELLS:
        raise ValueError(f"{who}: cells of {float(cell)} over the extent {tuple(float(x) for x in hi - o)} are more "
                         f"than SIMPLIFY_MAX_CELLS = {SIMPLIFY_MAX_CELLS} (2^26): use a larger cell")
    return np.ascontiguousarray(o, dtype=_F), np.ascontiguousarray(top.astype(np.int32) + 1)


def _simplify_count(p, t, origin, cell, dims, ws, totals):
    """anerf_mesh_simplify_count on checked device tensors (ws: its workspace; totals int64 [2] on the device)."""
    _lib.check(_lib.load().anerf_mesh_simplify_count(
        _lib.ptr(p), int(p.shape[0]), _lib.ptr(t), int(t.shape[0]), origin.ctypes.data_as(ctypes.c_void_p),
        float(cell), dims.ctypes.data_as(ctypes.c_void_p), _lib.ptr(ws), int(ws.shape[0]), _lib.ptr(totals),
        _lib.stream_handle(p.device)), "anerf_mesh_simplify_count")


def _simplify_emit(p, t, origin, cell, dims, ws, out_v, out_t, vertex_map, reps):
    """anerf_mesh_simplify_emit after _simplify_count on the same arguments, into outputs of the counted sizes."""
    _lib.check(_lib.load().anerf_mesh_simplify_emit(
        _lib.ptr(p), int(p.shape[0]), _lib.ptr(t), int(t.shape[0]), origin.ctypes.data_as(ctypes.c_void_p),
        float(cell), dims.ctypes.data_as(ctypes.c_void_p), _lib.ptr(ws), int(ws.shape[0]), _lib.ptr(out_v),
        int(out_v.shape[0]), _lib.ptr(out_t), int(out_t.shape[0]), _lib.ptr(vertex_map), _lib.ptr(reps),
        _lib.stream_handle(p.device)), "anerf_mesh_simplify_emit")


def _simplify_workspace(n_vertices, n_tri, dims, device):
    need = _lib.workspace("anerf_mesh_simplify_workspace", int(n_vertices), int(n_tri),
                          int(dims[0]) * int(dims[1]) * int(dims[2]))
    return torch.empty(need, device=device, dtype=torch.uint8)


@torch.no_grad()
def simplify_mesh(vertices, triangles, cell, attrs=None, origin=None):
    """Simplify a mesh (vertices float [V, 3], triangles int [T, 3]) by vertex clustering on the device: the vertices
    are snapped to a grid of cubic cells of edge `cell` that starts at `origin`, every cell's vertices become one (at
    their fixed-point mean), and the triangles that collapse, or that repeat the vertex set of an earlier one in
    either winding, are dropped.  Returns SimplifiedMesh of device tensors:
      vertices float32 [V', 3], triangles int32 [T', 3]   the new mesh, both in their original relative order;
      vertex_map int32 [V]                                the new id of every old vertex;
      representatives int32 [V']                          the old id of every new vertex: its cell's smallest;
      attrs                                               `attrs` (a dict or list of per-vertex tensors [V, ...]; None
                                                          gives None) gathered with `representatives`, exactly as
                                                          filter_mesh gathers with its kept index: a new vertex takes
                                                          its representative's normal or colour, nothing is averaged.
    origin=None: the per-axis fp32 minimum of the vertices; a given origin (x, y, z) keeps the cells where they are from
    one mesh to the next (extract_mesh clusters in index coordinates from (0, 0, 0): cells aligned with the voxels).
    The grid's dims follow from the per-axis maximum.  The contract is the module docstring's, bit for bit that of
    `simplify_mesh_reference`.
    Two host reads: the minimum, the maximum, the finiteness of the vertices and the range of the ids in one; the two
    totals between anerf_mesh_simplify_count and anerf_mesh_simplify_emit in the other.  Everything runs on the current
    stream.  ValueError before anything is launched: a non-finite vertex; a cell that is not finite or <= 0; a vertex
    below a given origin; more than SIMPLIFY_MAX_CELLS = 2^26 cells; ids outside [0, V); attrs whose row count is not V.
    Stricter than the C entries, which drop a vertex outside the grid or a triangle with an id outside [0, V) silently.
    Without vertices the result is empty; without triangles the vertices are still clustered.  Out of scope (module
    docstring): quadric-error placement, edge collapses, target triangle counts, keeping the result manifold."""
    who = "simplify_mesh"
    v, t = torch.as_tensor(vertices), torch.as_tensor(triangles)
    cell, origin = _simplify_args(tuple(v.shape), t, cell, origin, attrs, who)
    nv, nt = int(v.shape[0]), int(t.shape[0])
    dev = v.device if v.is_cuda else (t.device if t.is_cuda else None)
    vf = v.to(torch.float32)
    if nv == 0:
        lo = hi = np.zeros(3, _F)
        stats = [1.0] + ([float(t.amin()), float(t.amax())] if nt else [])  # (ids without vertices: an error)
    else:
        parts = [vf.amin(0).double(), vf.amax(0).double(), torch.isfinite(vf).all().double().reshape(1)]
        if nt:  # (ids below 2^31 are exact in float64)
            parts += [t.amin().double().reshape(1).to(vf.device), t.amax().double().reshape(1).to(vf.device)]
        stats = torch.cat(parts).cpu().numpy()  # (the first host read: put together where the vertices are)
        lo, hi, stats = stats[0:3], stats[3:6], stats[6:]
    o, dims = _simplify_grid(lo, hi, bool(stats[0]), stats[1] if nt else None, stats[2] if nt else None, nv, cell,
                             origin, who)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        if nv == 0:
            empty_v = torch.zeros((0, 3), device=dev, dtype=torch.float32)
            empty_i = torch.zeros(0, device=dev, dtype=torch.int32)
            out_a = _gather_attrs(attrs, lambda a: torch.as_tensor(a).to(dev)[:0], 0, who)
            return SimplifiedMesh(empty_v, empty_i.reshape(0, 3), empty_i, empty_i.clone(), out_a)
        p = vf.to(dev).contiguous()
        tt = t.to(dev, torch.int32).contiguous()
        ws = _simplify_workspace(nv, nt, dims, dev)
        totals = torch.empty(2, device=dev, dtype=torch.int64)
        _simplify_count(p, tt, o, cell, dims, ws, totals)
        kv, kt = (int(x) for x in totals.cpu())  # (the second and last host read: the output sizes)
        out_v = torch.empty((kv, 3), device=dev, dtype=torch.float32)
        out_t = torch.empty((kt, 3), device=dev, dtype=torch.int32)
        vertex_map = torch.empty(nv, device=dev, dtype=torch.int32)
        reps = torch.empty(kv, device=dev, dtype=torch.int32)
        _simplify_emit(p, tt, o, cell, dims, ws, out_v, out_t, vertex_map, reps)
        idx = reps.long()
        out_a = _gather_attrs(attrs, lambda a: torch.as_tensor(a).to(dev).index_select(0, idx), nv, who)
    return SimplifiedMesh(out_v, out_t, vertex_map, reps, out_a)


def simplify_mesh_reference(vertices, triangles, cell, attrs=None, origin=None):
    """NumPy implementation of `simplify_mesh`'s contract (module docstring): its checker, with the same argument
    errors.  Returns SimplifiedMesh of arrays (attrs gathered on the host)."""
    who = "simplify_mesh_reference"
    host = _lib.host_array
    p = np.ascontiguousarray(host(vertices), dtype=_F)
    tri = np.asarray(host(triangles))
    cell, origin = _simplify_args(p.shape, tri, cell, origin, attrs, who)
    tri = np.ascontiguousarray(tri, dtype=np.int64)
    nv, nt = len(p), len(tri)
    if nv == 0:
        _simplify_grid(np.zeros(3, _F), np.zeros(3, _F), True, tri.min() if nt else None, tri.max() if nt else None,
                       0, cell, origin, who)
        none = np.zeros(0, np.int32)
        return SimplifiedMesh(np.zeros((0, 3), _F), none.reshape(0, 3), none, none.copy(),
                              _gather_attrs(attrs, lambda a: host(a)[:0], 0, who))
    with np.errstate(all="ignore"):
        finite = bool(np.isfinite(p).all())
        o, dims = _simplify_grid(p.min(0), p.max(0), finite, tri.min() if nt else None, tri.max() if nt else None, nv,
                                 cell, origin, who)
        q = (p - o) / cell
        c = np.floor(q)
        valid = np.isfinite(q).all(1) & (c >= 0).all(1) & (c < dims.astype(_F)).all(1)
    members = np.nonzero(valid)[0]  # ascending: the first member of a cell in this order is its smallest id
    ci = c[members].astype(np.int64)
    keys = (ci[:, 0] * int(dims[1]) + ci[:, 1]) * int(dims[2]) + ci[:, 2]
    _, first, cell_of_member = np.unique(keys, return_index=True, return_inverse=True)
    reps = np.sort(members[first])
    new_of_cell = np.empty(len(first), np.int64)
    new_of_cell[np.argsort(members[first], kind="stable")] = np.arange(len(first))
    vertex_map = np.full(nv, -1, np.int64)
    vertex_map[members] = new_of_cell[cell_of_member.reshape(-1)]
    # the fixed-point mean
    r = (q - c)[members]
    assert np.array_equal(r.astype(np.float64), q[members].astype(np.float64) - c[members].astype(np.float64)), \
        "q - floor(q) is exact in fp32"
    fixed = np.rint(r * _F(2.0 ** 20)).astype(np.int64)
    sums = np.zeros((len(reps), 3), np.int64)
    np.add.at(sums, vertex_map[members], fixed)
    count = np.bincount(vertex_map[members], minlength=len(reps))
    m = (sums.astype(np.float64) / count.astype(np.float64)[:, None] * 2.0 ** -20).astype(_F)
    out_v = (o + cell * (c[reps] + m)).astype(_F)  # (float32 operands throughout: each operation rounds to float32)
    # the triangles
    mapped = vertex_map[tri]
    live = (mapped >= 0).all(1) & (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & \
        (mapped[:, 0] != mapped[:, 2])
    alive = np.nonzero(live)[0]
    if len(alive):
        sets = np.sort(mapped[alive], axis=1)
        nk = max(len(reps), 1)
        if nk ** 3 < 2 ** 62:
            _, firsts = np.unique((sets[:, 0] * nk + sets[:, 1]) * nk + sets[:, 2], return_index=True)
        else:
            _, firsts = np.unique(sets, axis=0, return_index=True)
        alive = np.sort(alive[firsts])  # (return_index: the first occurrence, the smallest original index)
    out_t = mapped[alive].astype(np.int32).reshape(-1, 3)
    out_a = _gather_attrs(attrs, lambda a: host(a)[reps], nv, who)
    return SimplifiedMesh(out_v, out_t, vertex_map.astype(np.int32), reps.astype(np.int32), out_a)

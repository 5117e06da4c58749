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
"""
import collections

import numpy as np
import torch

from . import _lib

MeshComponents = collections.namedtuple("MeshComponents", ["labels", "roots", "triangle_counts", "vertex_counts"])
VertexAdjacency = collections.namedtuple("VertexAdjacency", ["offsets", "neighbors", "boundary"])


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


def _gather_attrs(attrs, gather, n_vertices):
    if attrs is None:
        return None
    items = attrs.items() if isinstance(attrs, dict) else enumerate(attrs)
    out = {}
    for k, a in items:
        if a.shape[0] != n_vertices:
            raise ValueError(f"filter_mesh: attribute {k!r} has {a.shape[0]} rows for {n_vertices} vertices")
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

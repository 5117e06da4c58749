"""Fields and mesh checks shared by test_isosurface.py (CPU) and test_gpu_isosurface.py."""
import functools
import importlib

import numpy as np

iso = importlib.import_module("a-nerf_amd.isosurface")


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_field(seed, shape=(9, 9, 9), border=True):
    """default_rng(seed).random(shape), the outer layer set to 0 (threshold 0.5)."""
    f = np.random.default_rng(seed).random(shape)
    if border:
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = 0, 0, 0, 0, 0, 0
    return _ro(f)


def _coords(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


SPHERE_C, SPHERE_R = 7.5, 5.6


@functools.lru_cache(maxsize=None)
def sphere_field():
    """16^3, inside = high, threshold 0: R - |p - c|."""
    x, y, z = _coords((16, 16, 16))
    return _ro(SPHERE_R - np.sqrt((x - SPHERE_C) ** 2 + (y - SPHERE_C) ** 2 + (z - SPHERE_C) ** 2))


@functools.lru_cache(maxsize=None)
def torus_field():
    """24^3, radii 7 and 3 around the grid's centre, threshold 0."""
    x, y, z = _coords((24, 24, 24))
    ring = np.sqrt((x - 11.5) ** 2 + (y - 11.5) ** 2) - 7.0
    return _ro(3.0 - np.sqrt(ring ** 2 + (z - 11.5) ** 2))


@functools.lru_cache(maxsize=None)
def two_spheres_field():
    x, y, z = _coords((24, 16, 16))
    d0 = np.sqrt((x - 5.5) ** 2 + (y - 7.5) ** 2 + (z - 7.5) ** 2)
    d1 = np.sqrt((x - 17.5) ** 2 + (y - 7.5) ** 2 + (z - 7.5) ** 2)
    return _ro(np.maximum(3.6 - d0, 3.6 - d1))


@functools.lru_cache(maxsize=None)
def blobs_field():
    """67 x 61 x 71 (290,177 points: 284 workgroups of 1024 points, two scan tiles of 256 workgroups, a ragged
    last workgroup), a few Gaussian blobs, threshold 0.5: few active cells."""
    shape = (67, 61, 71)
    x, y, z = _coords(shape)
    rng = np.random.default_rng(7)
    f = np.zeros(shape)
    for _ in range(5):
        c = rng.uniform(8, 52, 3)
        s = rng.uniform(2.5, 5.0)
        f += np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
    return _ro(f)


@functools.lru_cache(maxsize=None)
def last_rows_field():
    """The whole surface in the last rows of each axis: a small ball around the grid's far corner cell."""
    shape = (11, 13, 37)
    x, y, z = _coords(shape)
    d = np.sqrt((x - 8.4) ** 2 + (y - 10.4) ** 2 + (z - 34.4) ** 2)
    return _ro(1.45 - d)


# Grids of exactly 1024, 1025 (one workgroup's tile of points, + 1) and 262143, 262144, 262145 points (the 256 tiles
# of one round of the one-workgroup scan, -1, +0, +1)
TILE_EDGE_SHAPES = ((8, 8, 16), (5, 5, 41), (27, 133, 73), (64, 64, 64), (65, 37, 109))


@functools.lru_cache(maxsize=None)
def tile_edge_field(shape, corner=False):
    """A sphere of radius 0.3 min(shape) about the grid's centre and a ball of radius 1.6 three points in from the far
    corner, inside = high, threshold 0.  That ball ends two rows short of the last row of axis 0, so the last
    workgroups' tiles stay empty; `corner` puts a ball of radius 1.45 around the far corner point instead (a surface
    cut open by the grid's end): the edge two points before the corner along the last axis crosses, so the base of
    the last tile that owns an edge matters."""
    x, y, z = _coords(shape)
    c = [(n - 1) / 2 for n in shape]
    q, r = ([n - 1 for n in shape], 1.45) if corner else ([n - 4 for n in shape], 1.6)
    sphere = 0.3 * min(shape) - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    ball = r - np.sqrt((x - q[0]) ** 2 + (y - q[1]) ** 2 + (z - q[2]) ** 2)
    return _ro(np.maximum(sphere, ball))


@functools.lru_cache(maxsize=None)
def tile_edge_reference(shape, corner=False):
    """isosurface_reference (vertices, triangles, normals) of tile_edge_field(shape, corner), read-only."""
    out = iso.isosurface_reference(tile_edge_field(shape, corner), 0.0, normals=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def relu_field():
    """Values on both sides of 0 and a positive threshold (0.25): the clamp moves the vertices of every edge whose
    outside end is negative."""
    return _ro(np.random.default_rng(11).random((10, 9, 12)) * 2.0 - 1.0)


@functools.lru_cache(maxsize=None)
def nan_field():
    """The sphere with NaN samples in its empty surroundings (no NaN next to an inside sample)."""
    f = sphere_field().copy()
    f[0, 0, 0] = f[1, 2, 3] = f[15, 15, 15] = f[0, 8, 15] = f[14, 1, 7] = np.nan
    return _ro(f)


@functools.lru_cache(maxsize=None)
def reference(name, *args, threshold=0.0, relu=False, flip=False):
    """isosurface_reference of a named field, computed once per session (read-only arrays)."""
    v, t = iso.isosurface_reference(globals()[name](*args), threshold, relu=relu, flip=flip)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


# ------------------------------------------------------------------ mesh checks
def directed_edge_imbalance(tri):
    """{(a, b): count(a -> b) - count(b -> a)} over the directed edges, zero entries dropped."""
    tri = np.asarray(tri, np.int64)
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    bal = {}
    for a, b in e.tolist():
        k, s = ((a, b), 1) if a < b else ((b, a), -1)
        bal[k] = bal.get(k, 0) + s
    return {k: v for k, v in bal.items() if v}


def euler(vertices, tri):
    tri = np.asarray(tri, np.int64)
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    return len(vertices) - len(np.unique(e, axis=0)) + len(tri)


def signed_volume(vertices, tri):
    p = np.asarray(vertices, np.float64)[np.asarray(tri, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def areas(vertices, tri):
    p = np.asarray(vertices, np.float64)[np.asarray(tri, np.int64)]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def crossing_edges(field, threshold, relu=False):
    """The number of sign-changing grid edges, by slicing."""
    f = np.asarray(field, np.float32)
    if relu:
        f = np.maximum(f, 0)
    with np.errstate(invalid="ignore"):
        ins = f >= np.float32(threshold)
    return int((ins[1:] != ins[:-1]).sum() + (ins[:, 1:] != ins[:, :-1]).sum() + (ins[:, :, 1:] != ins[:, :, :-1]).sum())


def interpolated_values(field, vertices):
    """The grid linearly interpolated along each vertex's edge (float64), and the count of integer coordinates."""
    f = np.asarray(field, np.float64)
    v = np.asarray(vertices, np.float64)
    lo = np.floor(v)
    frac = v - lo
    axis = np.argmax(frac, axis=1)
    n_int = (frac == 0).sum(axis=1)
    lo = lo.astype(np.int64)
    hi = lo.copy()
    hi[np.arange(len(v)), axis] += 1
    hi = np.minimum(hi, np.array(f.shape) - 1)
    a, b = f[lo[:, 0], lo[:, 1], lo[:, 2]], f[hi[:, 0], hi[:, 1], hi[:, 2]]
    t = frac[np.arange(len(v)), axis]
    return a + t * (b - a), n_int

"""Meshes and expected results shared by test_mesh_smooth.py (CPU) and test_gpu_mesh_smooth.py, on top of _mesh_cases
and _iso_cases.  Everything is computed once per session and handed out read-only."""
import functools
import importlib

import numpy as np

import _mesh_cases as M

meshops = importlib.import_module("a-nerf_amd.meshops")

CLOSED = ("sphere", "torus", "blobs", "random33")  # the named meshes of the adjacency and smoothing tests
SMALL = ("no_triangles", "no_vertices", "one_triangle", "degenerate", "duplicated")
SHORT_ROW = 64  # csrc/anerf_mesh.hip: the raw entries up to which one thread sorts a row


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def hemisphere():
    """(vertices, triangles) of `sphere` cut open at x <= its centre: 288 vertices, 526 triangles, a rim of 48."""
    v, t = M.mesh("sphere")
    keep = v[:, 0] <= v.mean(0)[0]
    _, kept, tri = M.compact_expected(keep, t)
    return _ro(np.ascontiguousarray(v[kept]), tri)


@functools.lru_cache(maxsize=None)
def wheel(n):
    """(triangles, V) of n triangles (0, 1 + i, 1 + (i + 1) % n) around the hub 0: the hub's row lists 2 n pairs and
    has n distinct entries; every rim vertex is on the open edge (1 + i, 1 + (i + 1) % n), the hub on none."""
    i = np.arange(n, dtype=np.int64)
    tri = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1).astype(np.int32)
    return _ro(tri)[0], n + 1


@functools.lru_cache(maxsize=None)
def wheels(*ns):
    """(triangles, V) of disjoint wheels of ns[0], ns[1], ... triangles in one list, wheel i's ids after wheel
    i - 1's (wheels of 33: offset by 34 i)."""
    parts, nv = [], 0
    for n in ns:
        tri, v = wheel(n)
        parts.append(tri + nv)
        nv += v
    return _ro(np.concatenate(parts).astype(np.int32))[0], nv


# many_wheels: 1100 wheels of 33, every hub's row just over SHORT_ROW (66 listed pairs) and more rows than the 1024
# workgroups of the long-row kernels, so that 76 of them take a second row.  mixed_wheels: a short-of-LDS row, a row
# sorted over LDS and a row sorted over global memory on one list.
WHEEL_SETS = {"many_wheels": (33,) * 1100, "mixed_wheels": (33, 40, 5000)}


def wheel_vertices(n, seed=11):
    """Positions for wheel(n): the hub above a noisy unit circle."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1) + rng.normal(0, 0.05, (n, 3))
    return np.concatenate([[[0.1, -0.2, 0.7]], rim]).astype(np.float32)


def triangle_list(case):
    """(triangles, V) of a case: a named mesh, "name/kind" relabelled, "hemisphere", "wheel<n>", one of WHEEL_SETS, or
    one of _mesh_cases' synthetic lists."""
    if case in M.MESHES:
        v, t = M.mesh(case)
        return t, len(v)
    if "/" in case:
        return M.relabelled(*case.split("/"))[:2]
    if case == "hemisphere":
        v, t = hemisphere()
        return t, len(v)
    if case in WHEEL_SETS:
        return wheels(*WHEEL_SETS[case])
    if case.startswith("wheel"):
        return wheel(int(case[5:]))
    return M.synthetic(case)[:2]


@functools.lru_cache(maxsize=None)
def adjacency(case):
    """vertex_adjacency_reference of a case (read-only arrays)."""
    tri, nv = triangle_list(case)
    adj = meshops.vertex_adjacency_reference(tri, nv)
    _ro(*adj)
    return adj


def noisy(vertices, sigma=0.15, seed=7):
    return (vertices + np.random.default_rng(seed).normal(0, sigma, vertices.shape)).astype(np.float32)


def radial_std(vertices, clean):
    """The std of the radial deviation from the clean mesh's radii, about the clean mesh's centroid."""
    c = clean.mean(0)
    return float((np.linalg.norm(vertices - c, axis=1) - np.linalg.norm(clean - c, axis=1)).std())

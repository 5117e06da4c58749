"""Scenes and expected results shared by test_mesh_raster.py (CPU) and test_gpu_mesh_raster.py, on top of _mesh_cases
and _smooth_cases.  A scene is (vertices, triangles, transform, width, height, attrs); everything is computed once per
session and handed out read-only.  Unless a scene says otherwise its vertices are (pixel x, pixel y, depth) and its
transform the identity."""
import functools
import importlib

import numpy as np

import _mesh_cases as M

meshops = importlib.import_module("a-nerf_amd.meshops")

IDENTITY = np.eye(3, 4, dtype=np.float32)
IDENTITY.setflags(write=False)
SMALL = meshops.RASTER_SMALL_PIXELS  # the bounding box up to which a triangle's own thread draws it


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _scene(v, t, width, height, transform=IDENTITY, channels=3, seed=0):
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)
    attrs = None
    if channels:
        attrs = np.random.default_rng(100 + seed).random((len(v), channels)).astype(np.float32)
    A = np.array(transform, dtype=np.float32)
    _ro(v, t, A, attrs)
    return v, t, A, width, height, attrs


def reverse(t):
    return np.ascontiguousarray(np.asarray(t)[:, [0, 2, 1]])


# ------------------------------------------------------------------ coverage: vertices on pixel centres of 33 x 33
def _perimeter():
    """The 128 pixel centres on the rim of the 33 x 33 image, in order around it."""
    k = np.arange(32)
    top = np.stack([k, np.zeros(32)], 1)
    right = np.stack([np.full(32, 32), k], 1)
    bottom = np.stack([32 - k, np.full(32, 32)], 1)
    left = np.stack([np.zeros(32), 32 - k], 1)
    return np.concatenate([top, right, bottom, left]) + 0.5


def fan_mesh():
    """32 triangles around the image's centre pixel, each spanning 4 rim pixels: (vertices [33, 3], triangles)."""
    rim = _perimeter()[::4]
    v = np.concatenate([[[16.5, 16.5]], rim])
    v = np.concatenate([v, np.full((len(v), 1), 0.5)], 1)
    i = np.arange(32)
    return v, np.stack([np.zeros(32, np.int64), 1 + i, 1 + (i + 1) % 32], 1)


def grid_mesh(seed=3):
    """8 x 8 quads over the image, corners every 4 pixels, the inner corners moved by up to one pixel each way (still
    on pixel centres), every quad cut along a random diagonal: (vertices [81, 3], triangles [128, 3])."""
    rng = np.random.default_rng(seed)
    gy, gx = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    x, y = 4.0 * gx + 0.5, 4.0 * gy + 0.5
    inner = (gx > 0) & (gx < 8) & (gy > 0) & (gy < 8)
    x = x + np.where(inner, rng.integers(-1, 2, x.shape), 0)
    y = y + np.where(inner, rng.integers(-1, 2, y.shape), 0)
    v = np.stack([x.reshape(-1), y.reshape(-1), rng.uniform(0.2, 0.8, 81)], 1)
    tri = []
    for r in range(8):
        for c in range(8):
            a, b, d, e = 9 * r + c, 9 * r + c + 1, 9 * (r + 1) + c, 9 * (r + 1) + c + 1
            tri += [[a, b, e], [a, e, d]] if rng.random() < 0.5 else [[a, b, d], [b, e, d]]
    return v, np.array(tri)


def _fan(reverse_every=0):
    v, t = fan_mesh()
    if reverse_every:
        t[::reverse_every] = t[::reverse_every][:, [0, 2, 1]]
    return _scene(v, t, 33, 33)


def _quads(order):
    """Two parallel quads, the second nearer, overlapping in the middle; `order`: the triangle list's."""
    v = [[2, 2, .6], [20, 2, .6], [20, 18, .6], [2, 18, .6], [9.3, 7.1, .3], [30.2, 7.1, .3], [30.2, 24.6, .3],
         [9.3, 24.6, .3]]
    t = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    return _scene(v, t[list(order)], 33, 27)


def _duplicates():
    v = [[1.2, 1.1, .4], [28.7, 3.3, .4], [9.4, 25.2, .4], [5, 5, .4], [25, 8, .4], [12, 20, .4]]
    return _scene(v, [[3, 4, 5], [0, 1, 2], [0, 1, 2], [3, 4, 5]], 31, 29)


def _degenerate():
    v = [[2, 2, .5], [20, 3, .5], [7, 19, .5], [11, 2.5, .5], [12, 12, .2], [2, 2, .5]]
    # repeated ids, three points in line, two vertices at one place, and one triangle that does draw
    return _scene(v, [[1, 1, 3], [0, 0, 0], [0, 3, 1], [0, 5, 2], [0, 1, 2], [4, 4, 2]], 24, 22)


def _bad_vertices():
    v = [[2, 2, .5], [20, 3, .5], [7, 19, .5], [np.nan, 5, .5], [5, np.inf, .5], [5, 5, np.nan], [2.0 ** 20 + 1, 4, .5],
         [4, -2.0 ** 21, .5], [2.0 ** 20, 10, .5], [-2.0 ** 20, 8, .7]]
    # (the last triangle's vertices are at the 2^20 limit itself: it is drawn)
    return _scene(v, [[0, 1, 3], [0, 4, 2], [5, 1, 2], [0, 1, 6], [7, 1, 2], [0, 1, 2], [8, 9, 2]], 24, 22)


def _off_image():
    v, t = [], []
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1)):
        for reach in (0.6, 2.0):  # across the border, and wholly outside
            cx, cy = 20 + dx * 20 * reach, 15 + dy * 15 * reach
            k = len(v)
            v += [[cx - 7.3, cy - 5.2, .5], [cx + 8.1, cy - 3.7, .4], [cx + 0.4, cy + 9.9, .6]]
            t.append([k, k + 1, k + 2])
    return _scene(v, t, 40, 30)


def _depth_range():
    v = [[1, 1, -0.5], [38, 2, 1.5], [4, 28, 0.5], [1, 1, 1.5], [38, 2, -0.5], [30, 29, 0.25]]
    return _scene(v, [[0, 1, 2], [3, 4, 5]], 40, 30)


def _sliver(tall):
    v = [[1.0, 3.0, .3], [2.0, 3.0, .5], [1.5, 1003.0, .7]]
    if not tall:
        v = [[p[1], p[0], p[2]] for p in v]
    return _scene(v, [[0, 1, 2]], 4 if tall else 1010, 1010 if tall else 4)


def _soup(width, height, n=60, channels=3, seed=1):
    """Random triangles in unit coordinates reaching past the image, through a transform with no round number in it."""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.uniform(-0.3, 1.3, (3 * n, 2)), rng.uniform(-0.2, 1.2, (3 * n, 1))], 1)
    t = rng.permutation(3 * n).reshape(n, 3)
    A = np.array([[0.97 * width, 0.013 * width, 0.02 * width, 0.011 * width],
                  [-0.021 * height, 1.03 * height, 0.017 * height, -0.013 * height],
                  [0.031, -0.027, 0.93, 0.019]])
    return _scene(v, t, width, height, A, channels, seed)


def _box(w, h):
    """One triangle whose bounding box holds exactly w x h pixel centres."""
    v = [[2.25, 2.25, .2], [2.25 + w - 0.5, 2.25, .5], [2.25, 2.25 + h - 0.5, .8]]
    return _scene(v, [[0, 2, 1]], w + 6, h + 6)


def _full():
    return _scene([[-10, -10, .1], [2100, -10, .5], [-10, 2100, .9]], [[0, 1, 2]], 1024, 1024)


def _cube():
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * 0.4
    t = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
         [1, 5, 7], [1, 7, 3]]
    A = meshops.turntable_transforms(c, 3, 33.0, 512, 512, up=(0.2, 0.3, 1.0))[1]
    return _scene(c, t, 512, 512, A)


def _empty():
    return _scene(np.zeros((4, 3)), np.zeros((0, 3)), 9, 7)


SCENES = {
    "fan": _fan, "fan_mixed_windings": lambda: _fan(3), "grid": lambda: _scene(*grid_mesh(), 33, 33),
    "quads": lambda: _quads((0, 1, 2, 3)), "quads_swapped": lambda: _quads((2, 0, 3, 1)), "duplicates": _duplicates,
    "degenerate": _degenerate, "bad_vertices": _bad_vertices, "off_image": _off_image, "depth_range": _depth_range,
    "sliver_tall": lambda: _sliver(True), "sliver_wide": lambda: _sliver(False),
    "soup_1x1": lambda: _soup(1, 1), "soup_37x21": lambda: _soup(37, 21), "soup_257x255": lambda: _soup(257, 255, 200),
    "no_triangles": _empty, "one_channel": lambda: _soup(37, 21, channels=1, seed=2),
    "eight_channels": lambda: _soup(37, 21, channels=8, seed=3), "no_attrs": lambda: _soup(37, 21, channels=0, seed=4),
    "box_below": lambda: _box(SMALL - 1, 1), "box_at": lambda: _box(SMALL, 1), "box_above": lambda: _box(SMALL + 1, 1),
    "box_16x16": lambda: _box(16, SMALL // 16), "box_16x17": lambda: _box(16, SMALL // 16 + 1),
    "full_1024": _full, "cube_512": _cube,
}
BASIC = ("fan", "fan_mixed_windings", "grid", "quads", "quads_swapped", "duplicates", "degenerate", "bad_vertices",
         "off_image", "depth_range", "sliver_tall", "sliver_wide", "soup_1x1", "soup_37x21", "soup_257x255",
         "no_triangles", "one_channel", "eight_channels", "no_attrs")
SPLIT = ("box_below", "box_at", "box_above", "box_16x16", "box_16x17", "full_1024", "cube_512")
BACKGROUND = 0.25


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """rasterize_mesh_reference of a scene (read-only arrays)."""
    v, t, A, w, h, attrs = scene(name)
    out = meshops.rasterize_mesh_reference(v, t, A, w, h, attrs, BACKGROUND)
    _ro(*out)
    return out


# ------------------------------------------------------------------ real meshes under the turntable's matrices
VIEWS = (0, 7, 40)  # frames of the 91


@functools.lru_cache(maxsize=None)
def mesh_scene(name, frame, size=64):
    v, t = M.mesh(name)
    A = meshops.turntable_transforms(v, 91, 4.0, size, size)[frame]
    return _scene(v, t, size, size, A, 3, frame)


@functools.lru_cache(maxsize=None)
def mesh_reference(name, frame, size=64):
    v, t, A, w, h, attrs = mesh_scene(name, frame, size)
    out = meshops.rasterize_mesh_reference(v, t, A, w, h, attrs, BACKGROUND)
    _ro(*out)
    return out


@functools.lru_cache(maxsize=None)
def normals_reference(case):
    """(vertices, triangles, vertex_normals_reference) of a mesh case of _smooth_cases / _mesh_cases."""
    import _smooth_cases as S
    if case in M.MESHES:
        v, t = M.mesh(case)
    elif case == "hemisphere":
        v, t = S.hemisphere()
    elif case.startswith("wheel"):
        t, nv = S.triangle_list(case)
        v = S.wheel_vertices(nv - 1)
    else:
        t, nv = S.triangle_list(case)
        v = np.random.default_rng(21).normal(0, 1, (nv, 3)).astype(np.float32)
    n = meshops.vertex_normals_reference(v, t)
    n.setflags(write=False)
    return v, t, n

"""Scenes and expected results shared by test_mesh_raster_persp.py (CPU) and test_gpu_mesh_raster_persp.py.  A scene
is the keyword arguments of meshops.rasterize_mesh_camera (without `background`); everything is computed once per
session and handed out read-only."""
import functools
import importlib

import numpy as np

meshops = importlib.import_module("a-nerf_amd.meshops")

F = np.float32
BACKGROUND = 0.25
CUBE_TRIANGLES = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6],
                  [0, 6, 4], [1, 5, 7], [1, 7, 3]]


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def camera(R=np.eye(3), eye=(0, 0, 0)):
    c2w = np.eye(4)
    c2w[:3, :3] = R
    c2w[:3, 3] = eye
    return c2w


def _scene(v, t, c2w, H, W, focal, near, far, center=None, channels=3, seed=0, attrs=None):
    v = np.ascontiguousarray(v, dtype=F).reshape(-1, 3)
    t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)
    if attrs is None and channels:
        attrs = np.random.default_rng(100 + seed).random((len(v), channels)).astype(F)
    c2w = np.array(c2w, dtype=np.float64)
    _ro(v, t, c2w, attrs)
    return dict(vertices=v, triangles=t, c2w=c2w, H=H, W=W, focal=focal, center=center, near=near, far=far, attrs=attrs)


def ray_dirs(sc):
    """The world directions float64 [H, W, 3] of get_rays' rays for a scene's camera (their depth along the axis is 1,
    so a ray's parameter is the camera depth), and the rays' origin."""
    H, W = sc["H"], sc["W"]
    f = np.asarray(sc["focal"], dtype=np.float64).reshape(-1)
    ox, oy = (W / 2, H / 2) if sc["center"] is None else sc["center"]
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(i - ox) / f[0], -(j - oy) / f[-1], -np.ones((H, W))], -1)
    return d @ sc["c2w"][:3, :3].T, sc["c2w"][:3, 3]


# ------------------------------------------------------------------ case A: a quad receding from depth 1 to depth 4
def _case_a():
    v = [[-.5, -.5, -1], [-.5, .5, -1], [2, 2, -4], [2, -2, -4]]
    return _scene(v, [[0, 1, 2], [0, 2, 3]], camera(), 48, 64, 32.0, 0.05, 100.0, attrs=np.array(v, dtype=F))


def case_a_hits():
    """(hit points float64 [H, W, 3], ray parameters [H, W]) of every pixel's ray with the quad's plane."""
    sc = scene("case_a")
    d, o = ray_dirs(sc)
    v = sc["vertices"].astype(np.float64)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    t = (n @ (v[0] - o)) / (d @ n)
    return o + t[..., None] * d, t


# ------------------------------------------------------------------ case B: a ground plane through near and far
PLANE_Y, PLANE_X, PLANE_Z = -0.4, (-3.0, 3.0), (-6.0, 2.0)


def _case_b():
    n = 24
    rng = np.random.default_rng(0)
    gz, gx = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x = PLANE_X[0] + (PLANE_X[1] - PLANE_X[0]) * gx / n
    z = PLANE_Z[0] + (PLANE_Z[1] - PLANE_Z[0]) * gz / n
    inner = (gx > 0) & (gx < n) & (gz > 0) & (gz < n)
    x = x + np.where(inner, rng.uniform(-0.1, 0.1, x.shape), 0)
    z = z + np.where(inner, rng.uniform(-0.1, 0.1, z.shape), 0)
    v = np.stack([x.reshape(-1), np.full(x.size, PLANE_Y), z.reshape(-1)], 1)
    tri = []
    for r in range(n):
        for c in range(n):
            a, b, d, e = (n + 1) * r + c, (n + 1) * r + c + 1, (n + 1) * (r + 1) + c, (n + 1) * (r + 1) + c + 1
            tri += [[a, b, e], [a, e, d]] if (r + c) % 2 else [[a, b, d], [b, e, d]]
    return _scene(v, tri, camera(rot_x(-0.3)), 64, 96, 60.0, 0.6, 5.0)


def case_b_hits():
    """(x, z, ray parameter) float64 [H, W] of every pixel's ray with the plane y = PLANE_Y (parameter <= 0: no hit)."""
    sc = scene("case_b")
    d, o = ray_dirs(sc)
    with np.errstate(divide="ignore"):
        t = (PLANE_Y - o[1]) / d[..., 1]
    return o[0] + t * d[..., 0], o[2] + t * d[..., 2], t


def in_counts(sc):
    """Per triangle, how many of its vertices are at or beyond the near plane (float64)."""
    V, _ = meshops.camera_view(sc["c2w"], sc["H"], sc["W"], sc["focal"], sc["center"])
    d = sc["vertices"].astype(np.float64) @ V[2, :3].astype(np.float64) + float(V[2, 3])
    return (d[sc["triangles"]] >= sc["near"]).sum(1)


# ------------------------------------------------------------------ seams
def _seam_pair(order):
    """Two triangles over the edge A (in front of near) - B (behind the eye), C and D on either side of it; the second
    one lists its vertices in `order`, a permutation of (A, B, D) = (0, 1, 3)."""
    v = [[0.13, -0.21, -2.1], [-0.31, 0.47, 0.6], [-0.9, -0.55, -1.4], [0.85, 0.6, -1.7]]
    return _scene(v, [[0, 1, 2], list(order)], camera(), 40, 48, 30.0, 0.5, 50.0)


def _seam_diagonal():
    """One triangle with two vertices IN, cut at t = 1 / 2 on both edges: the seam q0 - q2 runs from pixel centre
    (4.5, 4.5) to (20.5, 20.5) through the centres (k + 0.5, k + 0.5) between them (camera space (xc, yc, d) ->
    world (xc, -yc, -d) under the identity c2w)."""
    v = [[-0.75, 0.75, -2.0], [1.0, 0.5, -2.0], [-0.75, -0.75, 0.0]]
    return _scene(v, [[0, 1, 2]], camera(), 32, 32, 32.0, 1.0, 50.0)


# ------------------------------------------------------------------ triangles that draw nothing
def _nothing(kind):
    a = {"behind": [[-1, -1, 1], [1, -1, 2], [0, 1, 3]],            # wholly behind the eye
         "too_near": [[-.1, -.1, -.2], [.1, -.1, -.3], [0, .1, -.4]],  # in front of it, nearer than near
         "too_far": [[-9, -9, -30], [9, -9, -31], [0, 9, -32]],
         "nan": [[-1, -1, -2], [1, -1, np.nan], [0, 1, -2]],
         "edge_on": [[-.5, 0, -1], [.5, 0, -2], [0, 0, -3]],         # its plane holds the eye: no area on the screen
         "beyond_2^20": [[-1, -1, -2], [1e6, -1, -1], [0, 1, -2]]}[kind]
    return _scene(a, [[0, 1, 2]], camera(), 24, 32, 32.0, 0.5, 20.0)


def _ties():
    """Two triangles that overlap on the screen, each listed twice."""
    v = [[-1, -1, -2], [1, -1, -3], [0, 1, -2.5], [-1, 1, -1.5], [1, 0.5, -2], [0, -1, -4]]
    return _scene(v, [[3, 4, 5], [0, 1, 2], [0, 1, 2], [3, 4, 5]], camera(), 24, 32, 20.0, 0.5, 20.0)


# ------------------------------------------------------------------ a soup around the near plane
def _soup(W, H, n=300, channels=3, seed=1):
    """Random triangles in front of, across and behind the near plane and across far, both windings (random vertex
    orders), some repeated, some degenerate, one with a NaN vertex; a camera with no round number in it."""
    rng = np.random.default_rng(seed)
    centre = np.concatenate([rng.uniform(-1.6, 1.6, (n, 1, 2)), rng.uniform(-3.2, 0.6, (n, 1, 1))], 2)
    v = (centre + rng.uniform(-0.45, 0.45, (n, 3, 3))).reshape(3 * n, 3)
    v[7, 1] = np.nan
    t = np.stack([rng.permutation(3) + 3 * k for k in range(n)])
    t[5], t[9] = t[2], t[3][[0, 2, 1]]                     # repeated, in either winding
    t[11], t[12] = [t[0, 0], t[0, 0], t[0, 1]], [4, 4, 4]  # degenerate
    c2w = camera(rot_y(0.07) @ rot_x(-0.05), (0.03, -0.02, 0.35))
    return _scene(v, t, c2w, H, W, (0.93 * W, 1.07 * W), 0.4, 2.9, center=(0.52 * W, 0.47 * H), channels=channels,
                  seed=seed)


# ------------------------------------------------------------------ a cube over the whole image, its near corner cut
def _cube(W, H):
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    c2w = camera(rot_y(0.5) @ rot_x(-0.4), (0.0, 0.0, 0.0))
    c2w[:3, 3] = c2w[:3, :3] @ np.array([0.0, 0.0, 2.3])  # looking at the origin from 2.3 away
    return _scene(c, CUBE_TRIANGLES, c2w, H, W, 0.62 * W, 1.1, 10.0, seed=5)


def _empty(nv):
    return _scene(np.zeros((nv, 3)), np.zeros((0, 3)), camera(), 7, 9, 8.0, 0.1, 10.0)


SCENES = {
    "case_a": _case_a, "case_b": _case_b, "seam_diagonal": _seam_diagonal, "ties": _ties,
    "soup": lambda: _soup(64, 48), "soup_1_channel": lambda: _soup(64, 48, channels=1, seed=2),
    "soup_8_channels": lambda: _soup(64, 48, channels=8, seed=3), "soup_no_attrs": lambda: _soup(64, 48, channels=0),
    "soup_w1": lambda: _soup(1, 48, n=120, seed=4), "soup_h1": lambda: _soup(64, 1, n=120, seed=6),
    "cube_large": lambda: _cube(256, 192), "cube_small": lambda: _cube(24, 16),
    "no_triangles": lambda: _empty(4), "no_vertices": lambda: _empty(0),
}
NOTHING = ("behind", "too_near", "too_far", "nan", "edge_on", "beyond_2^20")
SEAM_ORDERS = ((1, 0, 3), (0, 1, 3), (3, 1, 0), (0, 3, 1), (1, 3, 0), (3, 0, 1))
SIZES = ("soup_1_channel", "soup_8_channels", "soup_no_attrs", "soup_w1", "soup_h1", "no_triangles", "no_vertices")


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in SCENES:
        return SCENES[name]()
    kind, _, arg = name.partition(":")
    if kind == "nothing":
        return _nothing(arg)
    if kind == "seam_pair":
        return _seam_pair(tuple(int(c) for c in arg))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """rasterize_mesh_camera_reference of a scene (read-only arrays)."""
    out = meshops.rasterize_mesh_camera_reference(**scene(name), background=BACKGROUND)
    _ro(*out)
    return out


def box_pixels(name):
    """Per triangle of a scene, the pixel centres in its sub-triangles' clipped boxes together: what decides between the
    thread's and the workgroups' path (meshops.RASTER_SMALL_PIXELS)."""
    sc = scene(name)
    V, K = meshops.camera_view(sc["c2w"], sc["H"], sc["W"], sc["focal"], sc["center"])
    st = meshops._persp_setup_reference(sc["vertices"], sc["triangles"].astype(np.int64), V, K, F(sc["near"]), sc["W"],
                                        sc["H"])
    i0, i1, j0, j1, draws = st[6:]
    return (np.where(draws, (i1 - i0 + 1) * (j1 - j0 + 1), 0)).reshape(-1, 2).sum(1)


# ------------------------------------------------------------------ three cameras around the cube
@functools.lru_cache(maxsize=None)
def views():
    """Keyword arguments of render_mesh_views: the cube under three cameras with their own focal pairs and centres."""
    sc = scene("cube_small")
    H, W = 20, 28
    c2ws = []
    for k, (yaw, dist) in enumerate(((0.2, 2.4), (1.3, 3.1), (2.9, 4.0))):
        c = camera(rot_y(yaw) @ rot_x(-0.3 + 0.1 * k))
        c[:3, 3] = c[:3, :3] @ np.array([0.05 * k, 0.0, dist])
        c2ws.append(c)
    focal = np.array([[17.0, 18.5], [22.0, 21.0], [30.0, 30.0]])
    centers = np.array([[13.2, 10.4], [14.0, 10.0], [15.1, 9.3]])
    colors = np.random.default_rng(9).random((len(sc["vertices"]), 3)).astype(F)
    c2ws = np.stack(c2ws)
    _ro(c2ws, focal, centers, colors)
    return dict(vertices=sc["vertices"], triangles=sc["triangles"], c2ws=c2ws, H=H, W=W, focal=focal, centers=centers,
                colors=colors, background=(1.0, 0.5, 0.25))


@functools.lru_cache(maxsize=None)
def views_reference():
    out = meshops.render_mesh_views_reference(**views())
    _ro(*out)
    return out

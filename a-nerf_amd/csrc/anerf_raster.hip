// anerf_raster.hip — looking at an extracted mesh on the device: face-accumulated vertex normals and a triangle
// rasteriser, orthographic (what the reference's viewer does through OpenGL on the host, render_mesh.py) and through
// the perspective cameras the field is rendered with.
//
//   anerf_mesh_vertex_normals  nrm_zero_kernel    the 64-bit accumulators [V][3] zeroed
//                              nrm_face_kernel    per triangle: its unit normal, quantised to 2^-30, added to the
//                                                 accumulators of its three vertices (64-bit integer atomics)
//                              nrm_vertex_kernel  per vertex: the sum back to fp32, normalised
//   anerf_mesh_raster          clear_kernel       the key buffer set to all ones, the list counter zeroed
//                              setup_kernel       per triangle: screen transform, snap, bounding box; a box of at most
//                                                 ANERF_RASTER_SMALL_PIXELS pixel centres is walked by the thread,
//                                                 a larger one goes onto the list (an integer atomic counter)
//                              large_kernel       the list, whose length is read on the device: LARGE_SPLIT workgroups
//                                                 per triangle, each taking tiles of 64 x 4 pixels of the clipped box
//                              resolve_kernel     per pixel: the winning triangle's barycentrics, depth and attributes
//   anerf_mesh_raster_persp    the same passes behind a pinhole camera (setup_persp_kernel, large_persp_kernel,
//                              resolve_persp_kernel): clip_triangle() cuts a triangle at the near plane into one or
//                              two sub-triangles, each a Setup that cover(), edge(), put_key() and walk_tiles() take
//                              as they take the affine path's; fragment_persp() interpolates 1 / depth
//
// Why integers.  A float atomic add sums in arrival order, so a vertex normal would differ in its last bits from run
// to run; the quantised face normals are summed as 64-bit integers, whose sum has no order.  Coverage is decided on
// vertices snapped to 1/256 pixel with 64-bit edge functions and a tie rule on the edge's direction, so a pixel centre
// on an edge two triangles share belongs to exactly one of them; the depth test is one 64-bit unsigned atomic min
// per fragment on the key (bits(z) << 32) | triangle id -- over [0, 1] the order of the bit patterns is the order of
// the depths, equal depths go to the smaller id, and a minimum does not depend on the order of arrival either.
// Every float of a fragment comes out of fragment(), which the small path, the large path and the resolve pass all
// call with the same integers: the outputs are the same bits whichever path a triangle took.  (DESIGN.md has the
// contract, the reasons for the threshold and the tile shape.)
//
// Bounds.  A triangle with an id outside [0, V) is skipped by every kernel; pixel loops run over the box clipped to
// the image; the list holds each triangle at most once (capacity n_tri) and large_kernel clamps the count it reads.
#include <cmath>

#include "anerf_scan.hpp"

namespace {

constexpr int MAX_DIM = 16384;       // width, height
constexpr int MAX_CH = 8;            // attribute channels
constexpr int SNAP = 256;            // sub-pixel steps per pixel
constexpr float SCREEN_MAX = 1048576.f;  // 2^20: |s_0|, |s_1| beyond it drop the triangle
constexpr int LARGE_BLOCKS = 2048;   // workgroups of large_kernel
constexpr int LARGE_SPLIT = 32;      // workgroups that share one listed triangle
constexpr int TILE_W = 64, TILE_H = NTHR / TILE_W;  // a wave's 64 keys are 512 contiguous bytes of one row
constexpr unsigned long long EMPTY = ~0ull;
constexpr float QUANT = 1073741824.f;  // 2^30
constexpr float NORMAL_EPS = 1e-8f;    // the viewer's normalize_v3

// ------------------------------------------------------------------ vertex normals
// v / max(|v|, 1e-8), |v| = sqrt((x x + y y) + z z), every operation separately rounded.
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
    float len = sqrtf((x * x + y * y) + z * z);
    if (len < NORMAL_EPS) len = NORMAL_EPS;
    x = __fdiv_rn(x, len);
    y = __fdiv_rn(y, len);
    z = __fdiv_rn(z, len);
}

__device__ __forceinline__ long long quantise(float c) {
    return isfinite(c) ? llrintf(c * QUANT) : 0ll;  // (|c| <= 1 + a few ulp: the product is exact)
}

__global__ __launch_bounds__(NTHR) void nrm_zero_kernel(long long* __restrict__ acc, long long n) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i < n) acc[i] = 0;
}

__global__ __launch_bounds__(NTHR) void nrm_face_kernel(const float* __restrict__ p, int nv,
                                                        const int* __restrict__ tri, long long nt, long long* acc) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= nt) return;
    const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    if (!in_range(a, b, c, nv)) return;
    const float ax = p[3 * (long long)a], ay = p[3 * (long long)a + 1], az = p[3 * (long long)a + 2];
    const float e1x = p[3 * (long long)b] - ax, e1y = p[3 * (long long)b + 1] - ay, e1z = p[3 * (long long)b + 2] - az;
    const float e2x = p[3 * (long long)c] - ax, e2y = p[3 * (long long)c + 1] - ay, e2z = p[3 * (long long)c + 2] - az;
    float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    normalize3(nx, ny, nz);
    const long long q[3] = {quantise(nx), quantise(ny), quantise(nz)};
    const int ids[3] = {a, b, c};
    for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d)
            if (q[d] != 0)
                __hip_atomic_fetch_add((unsigned long long*)acc + 3 * (long long)ids[k] + d, (unsigned long long)q[d],
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(NTHR) void nrm_vertex_kernel(const long long* __restrict__ acc, int nv,
                                                          float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v >= nv) return;
    const float inv = 1.f / QUANT;  // (a power of two: the products are exact)
    float x = (float)acc[3 * v] * inv, y = (float)acc[3 * v + 1] * inv, z = (float)acc[3 * v + 2] * inv;
    normalize3(x, y, z);
    out[3 * v] = x;
    out[3 * v + 1] = y;
    out[3 * v + 2] = z;
}

// ------------------------------------------------------------------ the rasteriser
struct Scene {
    const float* pos;
    const int* tri;
    int nv;
    long long nt;
    int width, height;
    float A[12];
};

// A triangle on the screen: snapped vertices (|X|, |Y| <= 2^28), depths, twice its area (made positive: `flip`), and
// the pixel columns and rows whose centres its bounding box holds, clipped to the image.
struct Setup {
    int X[3], Y[3];
    float z[3];
    long long area2;
    bool flip;
    int i0, i1, j0, j1;
};

__device__ __forceinline__ float screen(const float* A, int row, float x, float y, float z) {
    return ((A[4 * row] * x + A[4 * row + 1] * y) + A[4 * row + 2] * z) + A[4 * row + 3];
}

// The rest of a Setup from its snapped vertices: false without an area or without a pixel centre of the image in its box.
__device__ __forceinline__ bool finish_setup(Setup& s, int width, int height) {
    const long long a2 = (long long)(s.X[1] - s.X[0]) * (long long)(s.Y[2] - s.Y[0]) -
                         (long long)(s.Y[1] - s.Y[0]) * (long long)(s.X[2] - s.X[0]);
    if (a2 == 0) return false;
    s.flip = a2 < 0;
    s.area2 = s.flip ? -a2 : a2;
    const int xmin = min(s.X[0], min(s.X[1], s.X[2])), xmax = max(s.X[0], max(s.X[1], s.X[2]));
    const int ymin = min(s.Y[0], min(s.Y[1], s.Y[2])), ymax = max(s.Y[0], max(s.Y[1], s.Y[2]));
    // centre SNAP i + SNAP / 2 in [xmin, xmax]: i from ceil((xmin - 128) / 256) to floor((xmax - 128) / 256)
    s.i0 = max((xmin - SNAP / 2 + SNAP - 1) >> 8, 0);
    s.i1 = min((xmax - SNAP / 2) >> 8, width - 1);
    s.j0 = max((ymin - SNAP / 2 + SNAP - 1) >> 8, 0);
    s.j1 = min((ymax - SNAP / 2) >> 8, height - 1);
    return s.i0 <= s.i1 && s.j0 <= s.j1;
}

// false: the triangle draws nothing (an id out of range, a screen value that is not finite or beyond 2^20, no area,
// or a box that holds no pixel centre of the image).
__device__ __forceinline__ bool setup_triangle(const Scene& sc, long long t, Setup& s) {
    const int ids[3] = {sc.tri[3 * t], sc.tri[3 * t + 1], sc.tri[3 * t + 2]};
    if (!in_range(ids[0], ids[1], ids[2], sc.nv)) return false;
    for (int k = 0; k < 3; ++k) {
        const float* p = sc.pos + 3 * (long long)ids[k];
        const float x = p[0], y = p[1], z = p[2];
        const float sx = screen(sc.A, 0, x, y, z), sy = screen(sc.A, 1, x, y, z), sz = screen(sc.A, 2, x, y, z);
        if (!(isfinite(sx) && isfinite(sy) && isfinite(sz)) || fabsf(sx) > SCREEN_MAX || fabsf(sy) > SCREEN_MAX)
            return false;
        s.X[k] = (int)llrintf(sx * (float)SNAP);
        s.Y[k] = (int)llrintf(sy * (float)SNAP);
        s.z[k] = sz;
    }
    return finish_setup(s, sc.width, sc.height);
}

// The edge function of (a -> b) at the sub-pixel point (px, py), oriented, and whether the point is on its inner side.
__device__ __forceinline__ bool edge(const Setup& s, int a, int b, int px, int py, long long& e) {
    int dx = s.X[b] - s.X[a], dy = s.Y[b] - s.Y[a];
    e = (long long)dx * (long long)(py - s.Y[a]) - (long long)dy * (long long)(px - s.X[a]);
    if (s.flip) {
        e = -e;
        dx = -dx;
        dy = -dy;
    }
    return e > 0 || (e == 0 && (dy > 0 || (dy == 0 && dx < 0)));
}

struct Fragment {
    float b0, b1, b2, z;
};

// Whether the centre of pixel (i, j) is covered, and its screen barycentrics -- the one place they are computed, for the
// affine and the perspective path alike.
__device__ __forceinline__ bool cover(const Setup& s, int i, int j, float& b0, float& b1, float& b2) {
    const int px = SNAP * i + SNAP / 2, py = SNAP * j + SNAP / 2;
    long long e12, e20, e01;
    const bool in12 = edge(s, 1, 2, px, py, e12), in20 = edge(s, 2, 0, px, py, e20), in01 = edge(s, 0, 1, px, py, e01);
    if (!(in12 && in20 && in01)) return false;
    const float area = (float)s.area2;
    b1 = __fdiv_rn((float)e20, area);
    b2 = __fdiv_rn((float)e01, area);
    b0 = (1.f - b1) - b2;
    return true;
}

// The fragment of pixel (i, j): covered or not, and its barycentrics and depth.
__device__ __forceinline__ bool fragment(const Setup& s, int i, int j, Fragment& f) {
    if (!cover(s, i, j, f.b0, f.b1, f.b2)) return false;
    float z = (f.b0 * s.z[0] + f.b1 * s.z[1]) + f.b2 * s.z[2];
    if (!(z >= 0.f && z <= 1.f)) return false;  // (a NaN fails both)
    if (z == 0.f) z = 0.f;                       // (-0 would sort last)
    f.z = z;
    return true;
}

// One fragment's depth test: the pixel keeps the smallest key (bits(depth) << 32) | triangle id (depth >= +0).
__device__ __forceinline__ void put_key(unsigned long long* keys, int i, int j, int width, float depth, long long t) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(unsigned)t;
    unsigned long long* k = keys + (long long)j * width + i;
    // keys only fall during a frame: a fragment behind what is already there need not go to the memory side
    if (key < __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_min(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void depth_test(const Setup& s, int i, int j, int width, long long t,
                                           unsigned long long* keys) {
    Fragment f;
    if (fragment(s, i, j, f)) put_key(keys, i, j, width, f.z, t);
}

// A workgroup's share `sub` of LARGE_SPLIT of a box's 64 x 4 tiles: test(i, j) for its thread's pixel of each.
template <class Test>
__device__ __forceinline__ void walk_tiles(const Setup& s, int sub, Test test) {
    const int ti = threadIdx.x % TILE_W, tj = threadIdx.x / TILE_W;
    const int tiles_x = (s.i1 - s.i0) / TILE_W + 1, tiles_y = (s.j1 - s.j0) / TILE_H + 1;
    const long long ntiles = (long long)tiles_x * tiles_y;
    for (long long tile = sub; tile < ntiles; tile += LARGE_SPLIT) {
        const int i = s.i0 + (int)(tile % tiles_x) * TILE_W + ti, j = s.j0 + (int)(tile / tiles_x) * TILE_H + tj;
        if (i <= s.i1 && j <= s.j1) test(i, j);
    }
}

__global__ __launch_bounds__(NTHR) void clear_kernel(unsigned long long* __restrict__ keys, long long npix,
                                                     int* __restrict__ n_large) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i < npix) keys[i] = EMPTY;
    if (i == 0) *n_large = 0;
}

__global__ __launch_bounds__(NTHR) void setup_kernel(Scene sc, unsigned long long* keys, int* __restrict__ large,
                                                     int* n_large) {
    const long long t = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (t >= sc.nt) return;
    Setup s;
    if (!setup_triangle(sc, t, s)) return;
    const long long box = (long long)(s.i1 - s.i0 + 1) * (long long)(s.j1 - s.j0 + 1);
    if (box > ANERF_RASTER_SMALL_PIXELS) {
        large[atomicAdd(n_large, 1)] = (int)t;  // (each triangle at most once: the index stays below nt)
        return;
    }
    for (int j = s.j0; j <= s.j1; ++j)
        for (int i = s.i0; i <= s.i1; ++i) depth_test(s, i, j, sc.width, t, keys);
}

__global__ __launch_bounds__(NTHR) void large_kernel(Scene sc, unsigned long long* keys, const int* __restrict__ large,
                                                     const int* __restrict__ n_large) {
    const long long n = min((long long)max(*n_large, 0), sc.nt);
    const int group = blockIdx.x / LARGE_SPLIT, sub = blockIdx.x % LARGE_SPLIT, ngroups = gridDim.x / LARGE_SPLIT;
    for (long long li = group; li < n; li += ngroups) {  // (uniform over the workgroup)
        const long long t = large[li];
        if (t < 0 || t >= sc.nt) continue;
        Setup s;
        if (!setup_triangle(sc, t, s)) continue;
        walk_tiles(s, sub, [&](int i, int j) { depth_test(s, i, j, sc.width, t, keys); });
    }
}

struct Channels {
    float bg[MAX_CH];
};

__global__ __launch_bounds__(NTHR) void resolve_kernel(Scene sc, const unsigned long long* __restrict__ keys,
                                                       const float* __restrict__ attrs, int nch, Channels bg,
                                                       int* __restrict__ face_ids, float* __restrict__ depth,
                                                       float* __restrict__ bary, float* __restrict__ image) {
    const long long pix = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (pix >= (long long)sc.width * sc.height) return;
    const unsigned long long key = keys[pix];
    const long long t = (long long)(key & 0xffffffffull);
    Setup s;
    Fragment f;
    // (a key other than EMPTY names a triangle that produced this fragment: the three tests hold again)
    const bool hit = key != EMPTY && t < sc.nt && setup_triangle(sc, t, s) &&
                     fragment(s, (int)(pix % sc.width), (int)(pix / sc.width), f);
    face_ids[pix] = hit ? (int)t : -1;
    depth[pix] = hit ? f.z : __builtin_inff();
    bary[3 * pix] = hit ? f.b0 : 0.f;
    bary[3 * pix + 1] = hit ? f.b1 : 0.f;
    bary[3 * pix + 2] = hit ? f.b2 : 0.f;
    if (nch <= 0) return;
    const float *a0 = nullptr, *a1 = nullptr, *a2 = nullptr;
    if (hit) {
        a0 = attrs + (long long)sc.tri[3 * t] * nch;
        a1 = attrs + (long long)sc.tri[3 * t + 1] * nch;
        a2 = attrs + (long long)sc.tri[3 * t + 2] * nch;
    }
    for (int c = 0; c < nch; ++c)
        image[pix * nch + c] = hit ? (f.b0 * a0[c] + f.b1 * a1[c]) + f.b2 * a2[c] : bg.bg[c];
}

// ------------------------------------------------------------------ the perspective camera (ABI 26)
struct Lens {
    float fx, fy, cx, cy, near, far;
};

// A triangle behind a pinhole camera (sc.A is its view matrix), cut at the near plane into one or two sub-triangles.
// A sub-triangle is a Setup whose z[] holds 1 / d of its vertices; row[] are the weights of the cut polygon's vertices
// q0 .. q3 over the triangle's vertices counted from `start`, the IN vertex the walk begins at.
struct Clipped {
    Setup sub[2];  // (q0 q1 q2), (q0 q2 q3)
    bool draws[2];
    float row[4][3];
    int start;
};

// The cut point of the edge from its IN end i to its OUT end o (places in r), and its row.
__device__ __forceinline__ void cut(const float (&r)[3][3], int i, int o, float near, float (&q)[3], float (&row)[3]) {
    const float t = __fdiv_rn(r[i][2] - near, r[i][2] - r[o][2]);
    q[0] = r[i][0] + t * (r[o][0] - r[i][0]);
    q[1] = r[i][1] + t * (r[o][1] - r[i][1]);
    q[2] = near;
    row[0] = row[1] = row[2] = 0.f;
    row[i] = 1.f - t;
    row[o] = t;
}

// false: the triangle draws nothing (an id out of range, a camera-space value that is not finite, no vertex at or
// beyond near, a projected value that is not finite or beyond 2^20, or no sub-triangle with an area and a pixel centre).
__device__ __forceinline__ bool clip_triangle(const Scene& sc, const Lens& ln, long long t, Clipped& c) {
    const int ids[3] = {sc.tri[3 * t], sc.tri[3 * t + 1], sc.tri[3 * t + 2]};
    if (!in_range(ids[0], ids[1], ids[2], sc.nv)) return false;
    float cam[3][3];
    for (int k = 0; k < 3; ++k) {
        const float* p = sc.pos + 3 * (long long)ids[k];
        const float x = p[0], y = p[1], z = p[2];
        for (int a = 0; a < 3; ++a) cam[k][a] = screen(sc.A, a, x, y, z);
        if (!(isfinite(cam[k][0]) && isfinite(cam[k][1]) && isfinite(cam[k][2]))) return false;
    }
    const bool in0 = cam[0][2] >= ln.near, in1 = cam[1][2] >= ln.near, in2 = cam[2][2] >= ln.near;
    const int n_in = (int)in0 + (int)in1 + (int)in2;
    if (n_in == 0) return false;
    // the walk starts at the IN vertex whose predecessor is not IN (all IN: at vertex 0)
    const int s = n_in == 3 ? 0 : (in0 && !in2) ? 0 : (in1 && !in0) ? 1 : 2;
    c.start = s;
    float r[3][3];
    for (int k = 0; k < 3; ++k) {
        const int m = s + k >= 3 ? s + k - 3 : s + k;
        for (int a = 0; a < 3; ++a) r[k][a] = m == 0 ? cam[0][a] : m == 1 ? cam[1][a] : cam[2][a];
    }
    float q[4][3];
    for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 3; ++a) {
            q[k][a] = k < 3 ? r[k][a] : 0.f;
            c.row[k][a] = k == a ? 1.f : 0.f;
        }
    int nq = 3;
    if (n_in == 1) {
        cut(r, 0, 1, ln.near, q[1], c.row[1]);
        cut(r, 0, 2, ln.near, q[2], c.row[2]);
    } else if (n_in == 2) {
        cut(r, 1, 2, ln.near, q[2], c.row[2]);
        cut(r, 0, 2, ln.near, q[3], c.row[3]);
        nq = 4;
    }
    int X[4], Y[4];
    float iw[4];
    for (int k = 0; k < 4; ++k) {
        X[k] = Y[k] = 0;
        iw[k] = 0.f;
        if (k >= nq) continue;
        const float sx = ln.fx * __fdiv_rn(q[k][0], q[k][2]) + ln.cx, sy = ln.fy * __fdiv_rn(q[k][1], q[k][2]) + ln.cy;
        iw[k] = __fdiv_rn(1.f, q[k][2]);
        if (!(isfinite(sx) && isfinite(sy) && isfinite(iw[k])) || fabsf(sx) > SCREEN_MAX || fabsf(sy) > SCREEN_MAX)
            return false;
        X[k] = (int)llrintf(sx * (float)SNAP);
        Y[k] = (int)llrintf(sy * (float)SNAP);
    }
    for (int m = 0; m < 2; ++m) {
        Setup& ss = c.sub[m];
        const int v[3] = {0, m + 1, m + 2};
        for (int k = 0; k < 3; ++k) {
            ss.X[k] = X[v[k]];
            ss.Y[k] = Y[v[k]];
            ss.z[k] = iw[v[k]];
        }
        c.draws[m] = m + 3 <= nq && finish_setup(ss, sc.width, sc.height);
    }
    return c.draws[0] || c.draws[1];
}

struct PerspFragment {
    float u0, u1, u2, dep;
};

// The fragment of pixel (i, j) under a sub-triangle: u_k = b_k / d_k and the camera depth 1 / sum u -- the one place.
__device__ __forceinline__ bool fragment_persp(const Setup& s, float far, int i, int j, PerspFragment& f) {
    float b0, b1, b2;
    if (!cover(s, i, j, b0, b1, b2)) return false;
    f.u0 = b0 * s.z[0];
    f.u1 = b1 * s.z[1];
    f.u2 = b2 * s.z[2];
    f.dep = __fdiv_rn(1.f, (f.u0 + f.u1) + f.u2);
    return f.dep > 0.f && f.dep <= far;  // (a NaN fails both; near was the cut)
}

__device__ __forceinline__ void depth_test_persp(const Setup& s, float far, int i, int j, int width, long long t,
                                                 unsigned long long* keys) {
    PerspFragment f;
    if (fragment_persp(s, far, i, j, f)) put_key(keys, i, j, width, f.dep, t);
}

__global__ __launch_bounds__(NTHR) void setup_persp_kernel(Scene sc, Lens ln, unsigned long long* keys,
                                                           int* __restrict__ large, int* n_large) {
    const long long t = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (t >= sc.nt) return;
    Clipped c;
    if (!clip_triangle(sc, ln, t, c)) return;
    long long box = 0;
    for (int m = 0; m < 2; ++m)
        if (c.draws[m]) box += (long long)(c.sub[m].i1 - c.sub[m].i0 + 1) * (long long)(c.sub[m].j1 - c.sub[m].j0 + 1);
    if (box > ANERF_RASTER_SMALL_PIXELS) {
        large[atomicAdd(n_large, 1)] = (int)t;  // (once, with both sub-triangles: the index stays below nt)
        return;
    }
    for (int m = 0; m < 2; ++m) {
        if (!c.draws[m]) continue;
        const Setup& s = c.sub[m];
        for (int j = s.j0; j <= s.j1; ++j)
            for (int i = s.i0; i <= s.i1; ++i) depth_test_persp(s, ln.far, i, j, sc.width, t, keys);
    }
}

__global__ __launch_bounds__(NTHR) void large_persp_kernel(Scene sc, Lens ln, unsigned long long* keys,
                                                           const int* __restrict__ large,
                                                           const int* __restrict__ n_large) {
    const long long n = min((long long)max(*n_large, 0), sc.nt);
    const int group = blockIdx.x / LARGE_SPLIT, sub = blockIdx.x % LARGE_SPLIT, ngroups = gridDim.x / LARGE_SPLIT;
    for (long long li = group; li < n; li += ngroups) {  // (uniform over the workgroup)
        const long long t = large[li];
        if (t < 0 || t >= sc.nt) continue;
        Clipped c;
        if (!clip_triangle(sc, ln, t, c)) continue;
        for (int m = 0; m < 2; ++m) {
            if (!c.draws[m]) continue;
            const Setup& s = c.sub[m];
            walk_tiles(s, sub, [&](int i, int j) { depth_test_persp(s, ln.far, i, j, sc.width, t, keys); });
        }
    }
}

__global__ __launch_bounds__(NTHR) void resolve_persp_kernel(Scene sc, Lens ln,
                                                             const unsigned long long* __restrict__ keys,
                                                             const float* __restrict__ attrs, int nch, Channels bg,
                                                             int* __restrict__ face_ids, float* __restrict__ depth,
                                                             float* __restrict__ bary, float* __restrict__ image) {
    const long long pix = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (pix >= (long long)sc.width * sc.height) return;
    const unsigned long long key = keys[pix];
    const long long t = (long long)(key & 0xffffffffull);
    const int i = (int)(pix % sc.width), j = (int)(pix / sc.width);
    Clipped c;
    bool hit = false;
    float dep = __builtin_inff(), B[3] = {0.f, 0.f, 0.f};
    if (key != EMPTY && t < sc.nt && clip_triangle(sc, ln, t, c)) {
        // the first sub-triangle whose fragment is the key's (the one that produced it, or an equal one before it)
        float R[3] = {0.f, 0.f, 0.f};
        for (int m = 0; m < 2; ++m) {
            PerspFragment f;
            if (hit || !c.draws[m] || !fragment_persp(c.sub[m], ln.far, i, j, f) ||
                __float_as_uint(f.dep) != (unsigned)(key >> 32))
                continue;
            hit = true;
            dep = f.dep;
            const float g0 = f.u0 * dep, g1 = f.u1 * dep, g2 = f.u2 * dep;
            for (int a = 0; a < 3; ++a)
                R[a] = (g0 * c.row[0][a] + g1 * c.row[m + 1][a]) + g2 * c.row[m + 2][a];
        }
        // from the places counted from `start` back to the triangle's own vertices
        B[0] = c.start == 0 ? R[0] : c.start == 1 ? R[2] : R[1];
        B[1] = c.start == 0 ? R[1] : c.start == 1 ? R[0] : R[2];
        B[2] = c.start == 0 ? R[2] : c.start == 1 ? R[1] : R[0];
    }
    face_ids[pix] = hit ? (int)t : -1;
    depth[pix] = hit ? dep : __builtin_inff();
    bary[3 * pix] = hit ? B[0] : 0.f;
    bary[3 * pix + 1] = hit ? B[1] : 0.f;
    bary[3 * pix + 2] = hit ? B[2] : 0.f;
    if (nch <= 0) return;
    const float *a0 = nullptr, *a1 = nullptr, *a2 = nullptr;
    if (hit) {
        a0 = attrs + (long long)sc.tri[3 * t] * nch;
        a1 = attrs + (long long)sc.tri[3 * t + 1] * nch;
        a2 = attrs + (long long)sc.tri[3 * t + 2] * nch;
    }
    for (int ch = 0; ch < nch; ++ch)
        image[pix * nch + ch] = hit ? (B[0] * a0[ch] + B[1] * a1[ch]) + B[2] * a2[ch] : bg.bg[ch];
}

// Workspace: unsigned long long keys[W H] | int n_large, pad | int large[n_tri]
struct RasterPlan {
    size_t off_count, off_list, bytes;
};

bool raster_plan(int64_t nv, int64_t nt, int32_t w, int32_t h, RasterPlan* pl) {
    if (nv < 0 || nt < 0 || nv > MAXN || nt > MAXN || w < 1 || h < 1 || w > MAX_DIM || h > MAX_DIM) return false;
    pl->off_count = (size_t)w * (size_t)h * sizeof(unsigned long long);
    pl->off_list = pl->off_count + 8;
    pl->bytes = pl->off_list + (size_t)nt * sizeof(int);
    return true;
}

// The argument checks the two raster entries share, before any HIP call: ANERF_EINVAL naming the argument.
int raster_check(const char* who, const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                 int32_t width, int32_t height, const float* attrs, int32_t n_channels, const float* background,
                 const int32_t* face_ids, const float* depth, const float* bary, const float* image, const void* ws,
                 size_t ws_bytes, RasterPlan* pl) {
    if (width < 1 || width > MAX_DIM)
        return failf(ANERF_EINVAL, "%s: width %d must be in [1, %d]", who, (int)width, MAX_DIM);
    if (height < 1 || height > MAX_DIM)
        return failf(ANERF_EINVAL, "%s: height %d must be in [1, %d]", who, (int)height, MAX_DIM);
    if (!raster_plan(n_vertices, n_tri, width, height, pl))
        return failf(ANERF_EINVAL, "%s: n_vertices %lld / n_tri %lld must be in [0, 2^31)", who, (long long)n_vertices,
                     (long long)n_tri);
    if (n_channels < 0 || n_channels > MAX_CH)
        return failf(ANERF_EINVAL, "%s: n_channels %d must be in [0, %d]", who, (int)n_channels, MAX_CH);
    if (n_vertices > 0 && !vertices) return failf(ANERF_EINVAL, "%s: NULL vertices", who);
    if (n_tri > 0 && !triangles) return failf(ANERF_EINVAL, "%s: NULL triangles", who);
    if (!face_ids) return failf(ANERF_EINVAL, "%s: NULL face_ids", who);
    if (!depth) return failf(ANERF_EINVAL, "%s: NULL depth", who);
    if (!bary) return failf(ANERF_EINVAL, "%s: NULL bary", who);
    // (attrs [n_vertices][n_channels]: without vertices there is no extent, and an empty tensor's pointer is NULL)
    if (n_channels > 0 && n_vertices > 0 && !attrs) return failf(ANERF_EINVAL, "%s: NULL attrs", who);
    if (n_channels > 0 && !background) return failf(ANERF_EINVAL, "%s: NULL background", who);
    if (n_channels > 0 && !image) return failf(ANERF_EINVAL, "%s: NULL image", who);
    char sizer[64];
    snprintf(sizer, sizeof sizer, "%s_workspace", who);
    return check_workspace(who, ws, ws_bytes, pl->bytes, 8, ANERF_EINVAL, sizer);
}

Scene raster_scene(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                   const float* matrix, int32_t width, int32_t height) {
    Scene sc;
    sc.pos = vertices;
    sc.tri = triangles;
    sc.nv = (int)n_vertices;
    sc.nt = n_vertices > 0 ? (long long)n_tri : 0;
    sc.width = width;
    sc.height = height;
    for (int k = 0; k < 12; ++k) sc.A[k] = matrix[k];
    return sc;
}

int large_blocks(long long nt) {
    const long long want = nt * LARGE_SPLIT;  // no more workgroups than the list can use
    return (int)(want < LARGE_BLOCKS ? want : LARGE_BLOCKS);
}

}  // namespace

extern "C" {

size_t anerf_mesh_vertex_normals_workspace(int64_t n_vertices, int64_t n_tri) {
    if (n_vertices < 0 || n_tri < 0 || n_vertices > MAXN || n_tri > MAXN) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_vertex_normals_workspace: counts must be in [0, 2^31)");
        return 0;
    }
    return (size_t)(n_vertices > 0 ? n_vertices : 1) * 3 * sizeof(long long);  // the accumulators (never 0)
}

int anerf_mesh_vertex_normals(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                              float* normals, void* ws, size_t ws_bytes, void* stream) {
    if (n_vertices < 0 || n_tri < 0 || n_vertices > MAXN || n_tri > MAXN)
        return failf(ANERF_EINVAL, "anerf_mesh_vertex_normals: n_vertices %lld / n_tri %lld must be in [0, 2^31)",
                     (long long)n_vertices, (long long)n_tri);
    if (n_vertices > 0 && !vertices)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_vertex_normals: NULL vertices");
    if (n_vertices > 0 && !normals)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_vertex_normals: NULL normals");
    if (n_tri > 0 && !triangles)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_vertex_normals: NULL triangles");
    const int rc = check_workspace("anerf_mesh_vertex_normals", ws, ws_bytes,
                                   anerf_mesh_vertex_normals_workspace(n_vertices, n_tri), 8, ANERF_EINVAL,
                                   "anerf_mesh_vertex_normals_workspace");
    if (rc != ANERF_OK) return rc;
    if (n_vertices == 0) return ANERF_OK;
    hipStream_t s = (hipStream_t)stream;
    const int nv = (int)n_vertices;
    long long* acc = (long long*)ws;
    hipLaunchKernelGGL(nrm_zero_kernel, dim3(blocks_for(3ll * nv)), dim3(NTHR), 0, s, acc, 3ll * nv);
    if (n_tri > 0)
        hipLaunchKernelGGL(nrm_face_kernel, dim3(blocks_for(n_tri)), dim3(NTHR), 0, s, vertices, nv, triangles,
                           (long long)n_tri, acc);
    hipLaunchKernelGGL(nrm_vertex_kernel, dim3(blocks_for(nv)), dim3(NTHR), 0, s, (const long long*)acc, nv, normals);
    return launched("anerf_mesh_vertex_normals");
}

size_t anerf_mesh_raster_workspace(int64_t n_vertices, int64_t n_tri, int32_t width, int32_t height) {
    RasterPlan pl;
    if (!raster_plan(n_vertices, n_tri, width, height, &pl)) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_raster_workspace: counts must be in [0, 2^31), width and "
                                          "height in [1, 16384]");
        return 0;
    }
    return pl.bytes;
}

int anerf_mesh_raster(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                      const float* transform, int32_t width, int32_t height, const float* attrs, int32_t n_channels,
                      const float* background, int32_t* face_ids, float* depth, float* bary, float* image, void* ws,
                      size_t ws_bytes, void* stream) {
    RasterPlan pl;
    if (!transform) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_raster: NULL transform");
    const int rc = raster_check("anerf_mesh_raster", vertices, n_vertices, triangles, n_tri, width, height, attrs,
                                n_channels, background, face_ids, depth, bary, image, ws, ws_bytes, &pl);
    if (rc != ANERF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Scene sc = raster_scene(vertices, n_vertices, triangles, n_tri, transform, width, height);
    Channels bg = {};
    for (int c = 0; c < n_channels; ++c) bg.bg[c] = background[c];
    unsigned long long* keys = (unsigned long long*)ws;
    int* n_large = (int*)((char*)ws + pl.off_count);
    int* large = (int*)((char*)ws + pl.off_list);
    const long long npix = (long long)width * height;
    hipLaunchKernelGGL(clear_kernel, dim3(blocks_for(npix)), dim3(NTHR), 0, s, keys, npix, n_large);
    if (sc.nt > 0) {
        hipLaunchKernelGGL(setup_kernel, dim3(blocks_for(sc.nt)), dim3(NTHR), 0, s, sc, keys, large, n_large);
        hipLaunchKernelGGL(large_kernel, dim3(large_blocks(sc.nt)), dim3(NTHR), 0, s, sc, keys, (const int*)large,
                           (const int*)n_large);
    }
    hipLaunchKernelGGL(resolve_kernel, dim3(blocks_for(npix)), dim3(NTHR), 0, s, sc,
                       (const unsigned long long*)keys, attrs, (int)n_channels, bg, face_ids, depth, bary, image);
    return launched("anerf_mesh_raster");
}

size_t anerf_mesh_raster_persp_workspace(int64_t n_vertices, int64_t n_tri, int32_t width, int32_t height) {
    RasterPlan pl;
    if (!raster_plan(n_vertices, n_tri, width, height, &pl)) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_raster_persp_workspace: counts must be in [0, 2^31), width and "
                                          "height in [1, 16384]");
        return 0;
    }
    return pl.bytes;
}

int anerf_mesh_raster_persp(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                            const float* view, const float* intrinsics, float near, float far, int32_t width,
                            int32_t height, const float* attrs, int32_t n_channels, const float* background,
                            int32_t* face_ids, float* depth, float* bary, float* image, void* ws, size_t ws_bytes,
                            void* stream) {
    RasterPlan pl;
    if (!view) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_raster_persp: NULL view");
    if (!intrinsics) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_raster_persp: NULL intrinsics");
    if (!(std::isfinite(near) && near > 0.f))
        return failf(ANERF_EINVAL, "anerf_mesh_raster_persp: near %g must be finite and > 0", (double)near);
    if (!(std::isfinite(far) && far >= near))
        return failf(ANERF_EINVAL, "anerf_mesh_raster_persp: far %g must be finite and >= near (%g)", (double)far,
                     (double)near);
    static const char* const names[4] = {"fx", "fy", "cx", "cy"};
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(intrinsics[k]))
            return failf(ANERF_EINVAL, "anerf_mesh_raster_persp: intrinsics %s is not finite", names[k]);
    for (int k = 0; k < 2; ++k)
        if (intrinsics[k] == 0.f)
            return failf(ANERF_EINVAL, "anerf_mesh_raster_persp: intrinsics %s must not be 0", names[k]);
    const int rc = raster_check("anerf_mesh_raster_persp", vertices, n_vertices, triangles, n_tri, width, height, attrs,
                                n_channels, background, face_ids, depth, bary, image, ws, ws_bytes, &pl);
    if (rc != ANERF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Scene sc = raster_scene(vertices, n_vertices, triangles, n_tri, view, width, height);
    const Lens ln = {intrinsics[0], intrinsics[1], intrinsics[2], intrinsics[3], near, far};
    Channels bg = {};
    for (int c = 0; c < n_channels; ++c) bg.bg[c] = background[c];
    unsigned long long* keys = (unsigned long long*)ws;
    int* n_large = (int*)((char*)ws + pl.off_count);
    int* large = (int*)((char*)ws + pl.off_list);
    const long long npix = (long long)width * height;
    hipLaunchKernelGGL(clear_kernel, dim3(blocks_for(npix)), dim3(NTHR), 0, s, keys, npix, n_large);
    if (sc.nt > 0) {
        hipLaunchKernelGGL(setup_persp_kernel, dim3(blocks_for(sc.nt)), dim3(NTHR), 0, s, sc, ln, keys, large, n_large);
        hipLaunchKernelGGL(large_persp_kernel, dim3(large_blocks(sc.nt)), dim3(NTHR), 0, s, sc, ln, keys,
                           (const int*)large, (const int*)n_large);
    }
    hipLaunchKernelGGL(resolve_persp_kernel, dim3(blocks_for(npix)), dim3(NTHR), 0, s, sc, ln,
                       (const unsigned long long*)keys, attrs, (int)n_channels, bg, face_ids, depth, bary, image);
    return launched("anerf_mesh_raster_persp");
}

}  // extern "C"

// anerf_iso.hip — the density grid's iso-surface as an indexed mesh, on the device (marching cubes).
//
// run_render.render_mesh (run_render.py:970-986) copies the fwd_type='mesh' grid to the host and runs
// mcubes.marching_cubes over it; here the grid stays in HBM and is streamed four times:
//
//   anerf_isosurface_count   count_kernel    per grid point: its 3 owned edges (to +axis 0, 1, 2) that change sign
//                                            and the triangles of its cell (case table), summed per block
//                            scan_kernel     exclusive scan of the block sums (one workgroup, 64-bit), the totals
//   anerf_isosurface_emit    vertex_kernel   the same classification, scanned within the block: each point's first
//                                            vertex id to the workspace, its vertices to the output
//                            triangle_kernel per cell: the case's triangles; the id of a vertex on an edge owned by
//                                            another corner q = that point's stored first id + the number of q's
//                                            crossing edges on lower axes (q's crossing mask recomputed)
//
//   anerf_isosurface_normals normal_kernel  the vertex pass again, writing each vertex's normal: the grid's gradient
//                                            (central differences, one-sided at the borders) interpolated along
//                                            the vertex's edge with the same t, normalised (contract: anerf.h)
//
// Order is part of the contract (anerf.h): vertices by (owner's linear index, axis), triangles by (cell's linear
// index, table order) -- count -> scan -> emit, no atomics, so two runs give identical arrays.  Every pass
// classifies through load() / inside() below on the same values (relu applied as the value is loaded), so the
// emit passes can never produce more than the count pass counted; all output stores are guarded by the
// capacities passed in all the same.
//
// The tiles, the block scan, scan_kernel, the base | counts head of the workspace and the host helpers are
// anerf_scan.hpp's, shared with anerf_mesh.hip.  A workgroup is 256 threads x 4 consecutive points (consecutive in
// the grid's last axis, so a wave reads 1 KB runs); the neighbour rows a cell needs (+1 in axis 0 / 1) are read
// through the cache.  The pass is bound by those reads (4 B per point per pass) and the 4 B per point of
// first-vertex ids.
#include "anerf_scan.hpp"

namespace {

#define ANERF_ISO_QUAL __device__ const
#include "anerf_iso_table.inc"

constexpr int ISO_FLAGS = ANERF_ISO_RELU | ANERF_ISO_FLIP;

struct Grid {
    const float* v;
    int n0, n1, n2;
    int s0, s1;  // strides of axes 0 and 1 (axis 2: 1)
    int n;       // n0 n1 n2 < 2^31
    float thr;
    int relu;
    int cells;   // every dimension >= 2; a grid without cells has no triangles and no vertices (anerf.h)
};

// The one load and the one predicate of every pass.  (v < 0 ? 0 : v keeps a NaN a NaN, as np.maximum does.)
__device__ __forceinline__ float load(const Grid& g, int idx) {
    const float v = g.v[idx];
    return (g.relu && v < 0.f) ? 0.f : v;
}
__device__ __forceinline__ bool inside(const Grid& g, float v) { return v >= g.thr; }  // (a NaN is outside)

struct Point {
    int i, j, k;   // grid coordinates
    float v0;      // value at the point
    float va[3];   // value at the +axis neighbour (valid where the edge exists)
    int vmask;     // bit a: the owned edge along axis a changes sign
    int ccase;     // the cell's case, 0 where the point has no cell
};

// Classify point p: its owned edges and, when `want_case`, its cell.
__device__ __forceinline__ Point classify(const Grid& g, int p, bool want_case) {
    Point r;
    r.i = p / g.s0;
    const int rem = p - r.i * g.s0;
    r.j = rem / g.s1;
    r.k = rem - r.j * g.s1;
    const bool h0 = g.cells && r.i + 1 < g.n0, h1 = g.cells && r.j + 1 < g.n1, h2 = g.cells && r.k + 1 < g.n2;
    r.v0 = load(g, p);
    const bool in0 = inside(g, r.v0);
    r.vmask = 0;
    r.ccase = 0;
    bool ia[3] = {false, false, false};
    if (h0) { r.va[0] = load(g, p + g.s0); ia[0] = inside(g, r.va[0]); r.vmask |= (ia[0] != in0) ? 1 : 0; }
    if (h1) { r.va[1] = load(g, p + g.s1); ia[1] = inside(g, r.va[1]); r.vmask |= (ia[1] != in0) ? 2 : 0; }
    if (h2) { r.va[2] = load(g, p + 1); ia[2] = inside(g, r.va[2]); r.vmask |= (ia[2] != in0) ? 4 : 0; }
    if (want_case && h0 && h1 && h2) {
        int c = (in0 ? 1 : 0) | (ia[0] ? 2 : 0) | (ia[1] ? 4 : 0) | (ia[2] ? 16 : 0);
        c |= inside(g, load(g, p + g.s0 + g.s1)) ? 8 : 0;
        c |= inside(g, load(g, p + g.s0 + 1)) ? 32 : 0;
        c |= inside(g, load(g, p + g.s1 + 1)) ? 64 : 0;
        c |= inside(g, load(g, p + g.s0 + g.s1 + 1)) ? 128 : 0;
        r.ccase = c;
    }
    return r;
}

// The crossing mask of point q's owned edges on axes below `axis` (the rank of edge (q, axis) among q's vertices).
__device__ __forceinline__ int lower_axis_crossings(const Grid& g, int q, int axis) {
    if (axis == 0) return 0;
    const int i = q / g.s0;
    const int rem = q - i * g.s0;
    const int j = rem / g.s1;
    const bool in0 = inside(g, load(g, q));
    int cnt = 0;
    if (i + 1 < g.n0) cnt += inside(g, load(g, q + g.s0)) != in0;
    if (axis == 2 && j + 1 < g.n1) cnt += inside(g, load(g, q + g.s1)) != in0;
    return cnt;
}

__global__ __launch_bounds__(NTHR) void count_kernel(Grid g, int* __restrict__ block_counts, int nblocks) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    int nv = 0, nt = 0;
    for (int it = 0; it < ITEMS; ++it) {
        const long long p = first + it;
        if (p < g.n) {
            const Point pt = classify(g, (int)p, true);
            nv += __popc(pt.vmask);
            nt += ANERF_ISO_NTRI[pt.ccase];
        }
    }
    int tv, tt;
    block_exclusive_scan(nv, lds, tv);
    block_exclusive_scan(nt, lds, tt);
    if (threadIdx.x == 0) {
        block_counts[blockIdx.x] = tv;
        block_counts[nblocks + blockIdx.x] = tt;
    }
}

// The prologue of the two vertex passes: the thread's ITEMS points from `first` on classified into pts (vmask 0 past
// the grid's end), their crossing edges counted and scanned over the workgroup.  Returns the thread's first vertex id.
// (g by value: the kernels then compile to the instructions of the prologue written out in each; by reference not.)
__device__ __forceinline__ long long classify_tile(Grid g, const long long* base, long long first, Point (&pts)[ITEMS],
                                                   int* lds) {
    int nv = 0;
    for (int it = 0; it < ITEMS; ++it) {
        pts[it].vmask = 0;
        if (first + it < g.n) {
            pts[it] = classify(g, (int)(first + it), false);
            nv += __popc(pts[it].vmask);
        }
    }
    int total;
    return base[blockIdx.x] + block_exclusive_scan(nv, lds, total);
}

__global__ __launch_bounds__(NTHR) void vertex_kernel(Grid g, const long long* __restrict__ base, int* __restrict__ first_id,
                                                      float* __restrict__ vertices, long long max_vertices) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    Point pts[ITEMS];
    long long id = classify_tile(g, base, first, pts, lds);
    for (int it = 0; it < ITEMS; ++it) {
        if (first + it >= g.n) break;
        const Point& pt = pts[it];
        first_id[first + it] = (int)id;  // (ids fit an int where the caller's capacities do, anerf.h)
        for (int a = 0; a < 3; ++a) {
            if (!((pt.vmask >> a) & 1)) continue;
            if (id < max_vertices) {
                const float t = (g.thr - pt.v0) / (pt.va[a] - pt.v0);
                float x = (float)pt.i, y = (float)pt.j, z = (float)pt.k;
                if (a == 0) x += t;
                if (a == 1) y += t;
                if (a == 2) z += t;
                float* o = vertices + id * 3;
                o[0] = x;
                o[1] = y;
                o[2] = z;
            }
            ++id;
        }
    }
}

// Central difference of the values along one axis at grid point idx (coordinate c of n >= 2 along the axis, stride
// st), one-sided in the first and the last row (anerf.h, "vertex normals"): no index leaves the grid.
__device__ __forceinline__ float grad_axis(const Grid& g, int idx, int c, int n, int st) {
    if (c == 0) return load(g, idx + st) - load(g, idx);
    if (c == n - 1) return load(g, idx) - load(g, idx - st);
    return (load(g, idx + st) - load(g, idx - st)) * 0.5f;
}

// vertex_kernel's ids through the same classify_tile (recomputed, not read: the pass needs the count pass's bases
// only), writing each vertex's normal instead of its position.
__global__ __launch_bounds__(NTHR) void normal_kernel(Grid g, const long long* __restrict__ base,
                                                      float* __restrict__ normals, long long max_vertices, int flip) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    Point pts[ITEMS];
    long long id = classify_tile(g, base, first, pts, lds);
    for (int it = 0; it < ITEMS; ++it) {
        if (first + it >= g.n) break;
        const Point& pt = pts[it];
        if (!pt.vmask) continue;
        const int p = (int)(first + it);
        const float g0[3] = {grad_axis(g, p, pt.i, g.n0, g.s0), grad_axis(g, p, pt.j, g.n1, g.s1),
                             grad_axis(g, p, pt.k, g.n2, 1)};
        for (int a = 0; a < 3; ++a) {
            if (!((pt.vmask >> a) & 1)) continue;
            if (id < max_vertices) {
                const float t = (g.thr - pt.v0) / (pt.va[a] - pt.v0);
                const int q = p + (a == 0 ? g.s0 : (a == 1 ? g.s1 : 1));
                const float g1[3] = {grad_axis(g, q, pt.i + (a == 0), g.n0, g.s0),
                                     grad_axis(g, q, pt.j + (a == 1), g.n1, g.s1),
                                     grad_axis(g, q, pt.k + (a == 2), g.n2, 1)};
                const float Gx = g0[0] + t * (g1[0] - g0[0]);
                const float Gy = g0[1] + t * (g1[1] - g0[1]);
                const float Gz = g0[2] + t * (g1[2] - g0[2]);
                const float s = (Gx * Gx + Gy * Gy) + Gz * Gz;
                float* o = normals + id * 3;
                if (s > 0.0f && s < __builtin_inff()) {  // (a zero or non-finite G: no normal)
                    const float len = sqrtf(s);
                    o[0] = (flip ? Gx : -Gx) / len;
                    o[1] = (flip ? Gy : -Gy) / len;
                    o[2] = (flip ? Gz : -Gz) / len;
                } else {
                    o[0] = o[1] = o[2] = 0.0f;
                }
            }
            ++id;
        }
    }
}

__global__ __launch_bounds__(NTHR) void triangle_kernel(Grid g, const long long* __restrict__ base_t,
                                                        const int* __restrict__ first_id, int* __restrict__ triangles,
                                                        long long max_triangles, int flip) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    int cases[ITEMS];
    int nt = 0;
    for (int it = 0; it < ITEMS; ++it) {
        cases[it] = 0;
        if (first + it < g.n) {
            cases[it] = classify(g, (int)(first + it), true).ccase;
            nt += ANERF_ISO_NTRI[cases[it]];
        }
    }
    int total;
    long long tid = base_t[blockIdx.x] + block_exclusive_scan(nt, lds, total);
    for (int it = 0; it < ITEMS; ++it) {
        const int c = cases[it];
        const int n = ANERF_ISO_NTRI[c];
        if (n == 0) continue;
        const int p = (int)(first + it);
        for (int t = 0; t < n; ++t, ++tid) {
            if (tid >= max_triangles) continue;
            int ids[3];
            for (int e = 0; e < 3; ++e) {
                const int edge = ANERF_ISO_TRI[c][3 * t + e];
                const int corner = ANERF_ISO_EDGE_CORNER[edge], axis = ANERF_ISO_EDGE_AXIS[edge];
                const int q = p + (corner & 1) * g.s0 + ((corner >> 1) & 1) * g.s1 + ((corner >> 2) & 1);
                ids[e] = first_id[q] + lower_axis_crossings(g, q, axis);
            }
            int* o = triangles + tid * 3;
            o[0] = ids[0];
            o[1] = flip ? ids[2] : ids[1];
            o[2] = flip ? ids[1] : ids[2];
        }
    }
}

// Workspace layout: the scan's base | block_counts (ScanSpace) | int first_id[n]
struct Plan {
    long long n;
    ScanSpace scan;
    size_t bytes;  // (first_id starts at scan.bytes)
};

bool plan(int32_t n0, int32_t n1, int32_t n2, Plan* pl) {
    if (n0 < 1 || n1 < 1 || n2 < 1) return false;
    const long long n = (long long)n0 * n1;  // (< 2^62)
    if (n >= (1ll << 31) || n * n2 >= (1ll << 31)) return false;
    pl->n = n * n2;
    pl->scan = scan_space(tiles_for(pl->n));
    pl->bytes = pl->scan.bytes + (size_t)pl->n * sizeof(int);
    return true;
}

// The checks every entry shares: ANERF_OK and the plan, or the failure as anerf_last_error() has it.
int check_common(const char* who, const float* grid, int32_t n0, int32_t n1, int32_t n2, int32_t flags, const void* ws,
                 size_t ws_bytes, Plan* pl) {
    if (!grid || !ws) return failf(ANERF_EINVAL, "%s: NULL grid or workspace", who);
    if (n0 < 1 || n1 < 1 || n2 < 1)
        return failf(ANERF_EINVAL, "%s: grid dimensions %d x %d x %d must be >= 1", who, n0, n1, n2);
    if (!plan(n0, n1, n2, pl))
        return failf(ANERF_EINVAL, "%s: %d x %d x %d grid points do not fit 31 bits", who, n0, n1, n2);
    if (flags & ~ISO_FLAGS)
        return failf(ANERF_EINVAL, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~ISO_FLAGS));
    return check_workspace(who, ws, ws_bytes, pl->bytes, 8, ANERF_EWORKSPACE, "anerf_isosurface_workspace");
}

Grid make_grid(const float* grid, int32_t n0, int32_t n1, int32_t n2, const Plan& pl, float threshold, int32_t flags) {
    Grid g;
    g.v = grid;
    g.n0 = n0;
    g.n1 = n1;
    g.n2 = n2;
    g.s0 = n1 * n2;
    g.s1 = n2;
    g.n = (int)pl.n;
    g.thr = threshold;
    g.relu = (flags & ANERF_ISO_RELU) ? 1 : 0;
    g.cells = (n0 > 1 && n1 > 1 && n2 > 1) ? 1 : 0;
    return g;
}

}  // namespace

extern "C" {

size_t anerf_isosurface_workspace(int32_t n0, int32_t n1, int32_t n2) {
    Plan pl;
    if (!plan(n0, n1, n2, &pl)) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_isosurface_workspace: dimensions must be >= 1 and n0 n1 n2 < 2^31");
        return 0;
    }
    return pl.bytes;
}

int anerf_isosurface_count(const float* grid, int32_t n0, int32_t n1, int32_t n2, float threshold, int32_t flags, void* ws,
                           size_t ws_bytes, int64_t* totals_dev, void* stream) {
    Plan pl;
    const int rc = check_common("anerf_isosurface_count", grid, n0, n1, n2, flags, ws, ws_bytes, &pl);
    if (rc != ANERF_OK) return rc;
    if (!totals_dev) return anerf_internal_fail(ANERF_EINVAL, "anerf_isosurface_count: NULL totals");
    const Grid g = make_grid(grid, n0, n1, n2, pl, threshold, flags);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(count_kernel, dim3(pl.scan.nblocks), dim3(NTHR), 0, s, g, pl.scan.counts(ws), pl.scan.nblocks);
    scan_block_sums(pl.scan, ws, totals_dev, s);
    return launched("anerf_isosurface_count");
}

int anerf_isosurface_emit(const float* grid, int32_t n0, int32_t n1, int32_t n2, float threshold, int32_t flags, void* ws,
                          size_t ws_bytes, float* vertices, int64_t max_vertices, int32_t* triangles,
                          int64_t max_triangles, void* stream) {
    Plan pl;
    const int rc = check_common("anerf_isosurface_emit", grid, n0, n1, n2, flags, ws, ws_bytes, &pl);
    if (rc != ANERF_OK) return rc;
    if (max_vertices < 0 || max_triangles < 0 || max_vertices > 0x7fffffffll || max_triangles > 0x7fffffffll)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_isosurface_emit: capacities must be in [0, 2^31)");
    if ((max_vertices > 0 && !vertices) || (max_triangles > 0 && !triangles))
        return anerf_internal_fail(ANERF_EINVAL, "anerf_isosurface_emit: NULL output with a non-zero capacity");
    const Grid g = make_grid(grid, n0, n1, n2, pl, threshold, flags);
    const long long* base = (const long long*)ws;
    int* first_id = (int*)((char*)ws + pl.scan.bytes);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vertex_kernel, dim3(pl.scan.nblocks), dim3(NTHR), 0, s, g, base, first_id, vertices,
                       (long long)max_vertices);
    if (max_triangles > 0)
        hipLaunchKernelGGL(triangle_kernel, dim3(pl.scan.nblocks), dim3(NTHR), 0, s, g, base + pl.scan.nblocks, first_id,
                           triangles, (long long)max_triangles, (flags & ANERF_ISO_FLIP) ? 1 : 0);
    return launched("anerf_isosurface_emit");
}

int anerf_isosurface_normals(const float* grid, int32_t n0, int32_t n1, int32_t n2, float threshold, int32_t flags,
                             const void* ws, size_t ws_bytes, float* normals, int64_t max_vertices, void* stream) {
    Plan pl;
    const int rc = check_common("anerf_isosurface_normals", grid, n0, n1, n2, flags, ws, ws_bytes, &pl);
    if (rc != ANERF_OK) return rc;
    if (max_vertices < 0 || max_vertices > 0x7fffffffll)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_isosurface_normals: the capacity must be in [0, 2^31)");
    if (max_vertices > 0 && !normals)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_isosurface_normals: NULL output with a non-zero capacity");
    if (max_vertices == 0) return ANERF_OK;
    const Grid g = make_grid(grid, n0, n1, n2, pl, threshold, flags);
    hipLaunchKernelGGL(normal_kernel, dim3(pl.scan.nblocks), dim3(NTHR), 0, (hipStream_t)stream, g,
                       (const long long*)ws, normals, (long long)max_vertices, (flags & ANERF_ISO_FLIP) ? 1 : 0);
    return launched("anerf_isosurface_normals");
}

}  // extern "C"

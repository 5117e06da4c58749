// anerf_simplify.hip — vertex clustering (Rossignac-Borrel) of an indexed triangle mesh, on the device.
//
// The vertices are snapped to a uniform grid of cells, every cell's vertices become one, and the triangles that
// collapse or become copies of one another are dropped.  The contract is in include/anerf.h (ABI 25): every decision
// is an integer one and every fp32 / fp64 operation is separately and correctly rounded, so the outputs are the same
// bits on every run and those of meshops.simplify_mesh_reference.
//
//   anerf_mesh_simplify_count  fill_kernel        the cell table = "no vertex", the long-row counter = 0
//                              key_kernel         per vertex: its cell; table[cell] = min(table[cell], v) (the cell's
//                                                 representative: its smallest member); the vertex's sums zeroed
//                              sum_kernel         per vertex: rep[v] = table[cell]; its fixed-point offsets in the
//                                                 cell and 1 added to the representative's 64-bit sums and count
//                              owner_count_kernel per triangle that neither leaves the mesh nor collapses: its owner,
//                                                 the smallest of its three representatives, counts one row entry
//                              (exclusive_scan)   the row offsets; the rows longer than SHORT_ROW listed
//                              fill_rows_kernel   the rows through per-owner cursors, in arrival order: an entry is
//                                                 ((mid << 32) | max of the representatives, the triangle's index)
//                              dedup_kernel       per triangle of a short row: it survives iff no entry of its row has
//                                                 the same key and a smaller index (reads only: no order shows)
//                              long_rows_kernel   per listed row: one workgroup sorts it by (key, index) with a bitonic
//                                                 network over global memory; the first of every run of a key survives
//                              out_count_kernel   per tile: the representatives | the surviving triangles
//                              (scan)             scan_kernel: the tile bases and the totals V', T'
//   anerf_mesh_simplify_emit   vertices_kernel    the representatives in ascending id: vertex_map, representatives,
//                                                 the positions from the sums
//                              members_kernel     vertex_map of every other vertex, from its representative's
//                              triangles_kernel   the surviving triangles, ids through vertex_map
//
// Two triangles have the same unordered set of NEW ids iff they have the same set of representatives (the map from
// representatives to new ids is one to one and monotone), so duplicates are decided before any new id exists, and both
// totals are known after one pass: one host read.  The table is written by the fill alone in one launch and by atomics
// alone in the next; the sums are zeroed by plain stores in key_kernel and added to in sum_kernel.  Contention on one
// address is a cell's population.  No kernel waits for another workgroup.
//
// Memory safety: a vertex whose cell is not inside the grid (a non-finite coordinate among them) gets rep -1, touches
// no table word and is never dereferenced; a triangle with an id outside [0, V) or a vertex without a cell is dropped
// before any of its ids is used as an index.  The emit pass reads rep and the flags from the workspace and guards
// every index it takes from them.
//
// The owner rows are built with the row toolkit of anerf_scan.hpp (exclusive_scan, take_slot, the long-row list and
// its walk, bitonic_sort on KeyIndexRow), which this unit shares with the adjacency of anerf_mesh.hip; the two output
// lists go through the header's count -> scan -> emit pattern (ScanSpace), as in anerf_iso.hip.
#include "anerf_scan.hpp"

namespace {

constexpr long long MAX_CELLS = 1ll << 26;  // include/anerf.h ANERF_SIMPLIFY_MAX_CELLS
constexpr int NO_VERTEX = 0x7fffffff;      // an empty cell of the table
constexpr int SHORT_ROW = 32;              // the entries up to which a row is searched by its triangles' own threads
constexpr float FIX = 1048576.f;           // 2^20: the fixed point of a vertex's offset in its cell

struct Grid {
    float o[3], cell;
    int n[3];
};

struct Cell {
    bool valid;
    int key;
    float c[3];
    long long fx[3];
};

// The contract's cell of vertex v: q = (p - o) / cell, c = floor(q), valid iff every q is finite and 0 <= c < n.
__device__ __forceinline__ Cell cell_of(const float* __restrict__ p, long long v, const Grid& g) {
    Cell r;
    r.valid = true;
    float q[3];
    for (int a = 0; a < 3; ++a) {
        q[a] = __fdiv_rn(p[3 * v + a] - g.o[a], g.cell);
        r.c[a] = floorf(q[a]);
        r.valid = r.valid && __builtin_isfinite(q[a]) && r.c[a] >= 0.f && r.c[a] < (float)g.n[a];
    }
    r.key = -1;
    for (int a = 0; a < 3; ++a) r.fx[a] = 0;
    if (r.valid) {
        r.key = ((int)r.c[0] * g.n[1] + (int)r.c[1]) * g.n[2] + (int)r.c[2];  // (below n0 n1 n2 <= 2^26)
        for (int a = 0; a < 3; ++a) r.fx[a] = (long long)rintf((q[a] - r.c[a]) * FIX);  // (q - c: exact, in [0, 1))
    }
    return r;
}

__global__ __launch_bounds__(NTHR) void fill_kernel(int* __restrict__ table, long long n_cells,
                                                    int* __restrict__ n_long) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i < n_cells) table[i] = NO_VERTEX;
    if (i == 0) *n_long = 0;
}

__global__ __launch_bounds__(NTHR) void key_kernel(const float* __restrict__ p, int nv, Grid g, int* table,
                                                   long long* __restrict__ sums, int* __restrict__ cnt,
                                                   int* __restrict__ row_cnt) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v >= nv) return;
    sums[3 * v] = sums[3 * v + 1] = sums[3 * v + 2] = 0;
    cnt[v] = 0;
    row_cnt[v] = 0;
    const Cell c = cell_of(p, v, g);
    if (c.valid) atomicMin(table + c.key, (int)v);
}

__global__ __launch_bounds__(NTHR) void sum_kernel(const float* __restrict__ p, int nv, Grid g,
                                                   const int* __restrict__ table, int* __restrict__ rep,
                                                   long long* sums, int* cnt) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v >= nv) return;
    const Cell c = cell_of(p, v, g);
    int r = c.valid ? table[c.key] : -1;
    if ((unsigned)r >= (unsigned)nv) r = -1;  // (cannot happen: this vertex itself was a candidate)
    rep[v] = r;
    if (r < 0) return;
    for (int a = 0; a < 3; ++a)
        atomicAdd((unsigned long long*)(sums + 3 * (long long)r + a), (unsigned long long)c.fx[a]);
    atomicAdd(cnt + r, 1);
}

// A triangle that stays: its ids lie in [0, nv), its vertices have cells, its three representatives differ.  owner:
// the smallest representative; key: (the middle one << 32) | the largest.
__device__ __forceinline__ bool triangle_row(const int* __restrict__ tri, long long i, int nv,
                                             const int* __restrict__ rep, int& owner, unsigned long long& key) {
    const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    if ((unsigned)a >= (unsigned)nv || (unsigned)b >= (unsigned)nv || (unsigned)c >= (unsigned)nv) return false;
    const int ra = rep[a], rb = rep[b], rc = rep[c];
    if ((unsigned)ra >= (unsigned)nv || (unsigned)rb >= (unsigned)nv || (unsigned)rc >= (unsigned)nv) return false;
    if (ra == rb || rb == rc || ra == rc) return false;
    const int lo = min(ra, min(rb, rc)), hi = max(ra, max(rb, rc));
    const int mid = ra ^ rb ^ rc ^ lo ^ hi;
    owner = lo;
    key = ((unsigned long long)(unsigned)mid << 32) | (unsigned)hi;
    return true;
}

__global__ __launch_bounds__(NTHR) void owner_count_kernel(const int* __restrict__ tri, long long nt, int nv,
                                                           const int* __restrict__ rep, int* row_cnt) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= nt) return;
    int owner;
    unsigned long long key;
    if (triangle_row(tri, i, nv, rep, owner, key)) atomicAdd(row_cnt + owner, 1);
}

// Every entry takes a slot of its own in its owner's row (row_cnt: its cursor), in arrival order.
__global__ __launch_bounds__(NTHR) void fill_rows_kernel(const int* __restrict__ tri, long long nt, int nv,
                                                         const int* __restrict__ rep, int* row_cnt,
                                                         const int* __restrict__ row_off,
                                                         unsigned long long* __restrict__ keys,
                                                         int* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= nt) return;
    int owner;
    unsigned long long key;
    if (!triangle_row(tri, i, nv, rep, owner, key)) return;
    const int slot = take_slot(row_cnt, owner);
    if (slot < 0) return;  // (slot < the row's count: inside the row)
    const long long at = (long long)row_off[owner] + slot;
    if (at >= nt) return;
    keys[at] = key;
    idx[at] = (int)i;
}

// One thread per triangle: dropped (0) when it leaves the mesh or collapses; in a short row, kept iff no entry of the
// row has its key and a smaller index.  The triangles of long rows are flagged by long_rows_kernel.
__global__ __launch_bounds__(NTHR) void dedup_kernel(const int* __restrict__ tri, long long nt, int nv,
                                                     const int* __restrict__ rep, const int* __restrict__ row_off,
                                                     const unsigned long long* __restrict__ keys,
                                                     const int* __restrict__ idx, int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= nt) return;
    int owner;
    unsigned long long key;
    if (!triangle_row(tri, i, nv, rep, owner, key)) {
        flag[i] = 0;
        return;
    }
    const int b = row_off[owner], n = row_off[owner + 1] - b;
    if (n > SHORT_ROW) return;
    int keep = 1;
    for (int j = 0; j < n; ++j) {
        const long long at = (long long)b + j;
        if (at < 0 || at >= nt) break;
        if (keys[at] == key && idx[at] < (int)i) keep = 0;
    }
    flag[i] = keep;
}

// One workgroup per listed row (for_each_long_row): sorted by (key, index) in place over global memory by the bitonic
// network of anerf_scan.hpp, then the first entry of every run of a key -- its smallest index -- survives.
__global__ __launch_bounds__(NTHR) void long_rows_kernel(const int* __restrict__ row_off, unsigned long long* keys,
                                                         int* idx, int nv, long long nt,
                                                         const int* __restrict__ long_list,
                                                         const int* __restrict__ n_long, int* __restrict__ flag) {
    for_each_long_row(long_list, n_long, nv, [&](int v) {
        const long long b = row_off[v], e = row_off[v + 1];
        if (b < 0 || e > nt || e <= b) return;  // (uniform over the workgroup)
        const unsigned n = (unsigned)(e - b);
        unsigned long long* k = keys + b;
        int* x = idx + b;
        __syncthreads();
        bitonic_sort(KeyIndexRow{k, x}, n, padded_log2(n));
        __syncthreads();
        for (unsigned i = threadIdx.x; i < n; i += NTHR) {
            const int t = x[i];
            if ((unsigned)t < (unsigned)nt) flag[t] = (i == 0 || k[i - 1] != k[i]) ? 1 : 0;
        }
    });
}

__global__ __launch_bounds__(NTHR) void out_count_kernel(const int* __restrict__ rep, long long nv,
                                                         const int* __restrict__ flag, long long nt,
                                                         int* __restrict__ block_counts, int nblocks) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    int cv = 0, ct = 0;
    for (int it = 0; it < ITEMS; ++it) {
        const long long p = first + it;
        cv += (p < nv && rep[p] == (int)p) ? 1 : 0;
        ct += (p < nt && flag[p] != 0) ? 1 : 0;
    }
    int tv, tt;
    block_exclusive_scan(cv, lds, tv);
    block_exclusive_scan(ct, lds, tt);
    if (threadIdx.x == 0) {
        block_counts[blockIdx.x] = tv;
        block_counts[nblocks + blockIdx.x] = tt;
    }
}

// ------------------------------------------------------------------ emit
// The representatives in ascending id.  The new position of a cell: m = float(double(S) / double(n) 2^-20) per axis,
// p' = o + cell (float(c) + m), every operation separately rounded.
__global__ __launch_bounds__(NTHR) void vertices_kernel(const float* __restrict__ p, long long nv, Grid g,
                                                        const int* __restrict__ rep,
                                                        const long long* __restrict__ sums,
                                                        const int* __restrict__ cnt, const long long* __restrict__ base,
                                                        float* __restrict__ out, long long n_out,
                                                        int* __restrict__ vertex_map, int* __restrict__ reps_out) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    int r[ITEMS], n = 0;
    for (int it = 0; it < ITEMS; ++it) {
        r[it] = first + it < nv ? rep[first + it] : -1;
        n += r[it] == (int)(first + it) ? 1 : 0;
    }
    int total;
    long long id = base[blockIdx.x] + block_exclusive_scan(n, lds, total);
    for (int it = 0; it < ITEMS; ++it) {
        const long long v = first + it;
        if (v >= nv) break;
        if (r[it] != (int)v) {
            if ((unsigned)r[it] >= (unsigned)nv) vertex_map[v] = -1;  // (a member: members_kernel's)
            continue;
        }
        vertex_map[v] = (int)id;
        if (id < n_out) {
            reps_out[id] = (int)v;
            const Cell c = cell_of(p, v, g);
            const double members = (double)cnt[v];
            for (int a = 0; a < 3; ++a) {
                const float m = __double2float_rn(__ddiv_rn((double)sums[3 * v + a], members) * 0x1p-20);
                out[3 * id + a] = g.o[a] + g.cell * (c.c[a] + m);
            }
        }
        ++id;
    }
}

__global__ __launch_bounds__(NTHR) void members_kernel(const int* __restrict__ rep, int nv, int* vertex_map) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v >= nv) return;
    const int r = rep[v];
    if ((unsigned)r < (unsigned)nv && r != (int)v) vertex_map[v] = rep[r] == r ? vertex_map[r] : -1;
}

__global__ __launch_bounds__(NTHR) void triangles_kernel(const int* __restrict__ tri, long long nt, int nv,
                                                         const int* __restrict__ flag,
                                                         const long long* __restrict__ base_t,
                                                         const int* __restrict__ vertex_map, int* __restrict__ out,
                                                         long long n_out) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    bool k[ITEMS];
    int n = 0;
    for (int it = 0; it < ITEMS; ++it) {
        k[it] = first + it < nt && flag[first + it] != 0;
        n += k[it] ? 1 : 0;
    }
    int total;
    long long id = base_t[blockIdx.x] + block_exclusive_scan(n, lds, total);
    for (int it = 0; it < ITEMS; ++it) {
        if (!k[it]) continue;
        const int* s = tri + 3 * (first + it);
        const int a = s[0], b = s[1], c = s[2];
        if (id < n_out && (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv) {
            int* o = out + 3 * id;
            o[0] = vertex_map[a];
            o[1] = vertex_map[b];
            o[2] = vertex_map[c];
        }
        ++id;
    }
}

// ------------------------------------------------------------------ host
// Workspace: the scan of the outputs (base | block_counts over the tiles of max(V, T): emit finds it at ws itself) |
// sums[3 V] | keys[T]  (64-bit, then ints:) | table[cells] | rep[V] | cnt[V] | row_cnt[V] | row_off[V + 1] |
// long_list[V] | n_long | tiles (the scan of the rows', over the tiles of V) | flag[T] | idx[T]
struct Plan {
    ScanSpace out;
    size_t sums, keys, table, rep, cnt, row_cnt, row_off, long_list, n_long, tiles, flag, idx, bytes;
};

bool plan(int64_t nv, int64_t nt, int64_t cells, Plan* pl) {
    if (nv < 0 || nt < 0 || nv > MAXN || nt > MAXN || cells < 1 || cells > MAX_CELLS) return false;
    const int nb = tiles_for(nv > nt ? nv : nt);
    pl->out = scan_space(nb < 1 ? 1 : nb);  // (empty lists still get their totals written)
    const size_t V = (size_t)nv, T = (size_t)nt;
    size_t o = pl->out.bytes;
    pl->sums = o, o += 3 * V * sizeof(long long);
    pl->keys = o, o += T * sizeof(long long);
    pl->table = o, o += (size_t)cells * sizeof(int);
    pl->rep = o, o += V * sizeof(int);
    pl->cnt = o, o += V * sizeof(int);
    pl->row_cnt = o, o += V * sizeof(int);
    pl->row_off = o, o += (V + 1) * sizeof(int);
    pl->long_list = o, o += V * sizeof(int);
    pl->n_long = o, o += sizeof(int);
    pl->tiles = o, o += scan_ints((int)nv, false) * sizeof(int);
    pl->flag = o, o += T * sizeof(int);
    pl->idx = o, o += T * sizeof(int);
    pl->bytes = (o + 7) & ~(size_t)7;
    return true;
}

int check(const char* who, const float* vertices, int64_t nv, const int32_t* tri, int64_t nt, const float* origin,
          float cell, const int32_t* dims, const void* ws, size_t ws_bytes, Plan* pl, Grid* g) {
    if (nv < 0 || nt < 0 || nv > MAXN || nt > MAXN)
        return failf(ANERF_EINVAL, "%s: n_vertices %lld / n_tri %lld must be in [0, 2^31)", who, (long long)nv,
                     (long long)nt);
    if ((nv > 0 && !vertices) || (nt > 0 && !tri) || !origin || !dims || !ws)
        return failf(ANERF_EINVAL, "%s: NULL vertices, triangles, origin, dims or workspace", who);
    if (!(cell > 0.f) || !__builtin_isfinite(cell))
        return failf(ANERF_EINVAL, "%s: cell must be finite and > 0, got %g", who, (double)cell);
    if (!__builtin_isfinite(origin[0]) || !__builtin_isfinite(origin[1]) || !__builtin_isfinite(origin[2]))
        return failf(ANERF_EINVAL, "%s: origin must be finite", who);
    long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1 || dims[a] > MAX_CELLS) cells = -1;
        if (cells > 0) cells *= dims[a];
        if (cells > MAX_CELLS) cells = -1;
    }
    if (cells < 0)
        return failf(ANERF_EINVAL, "%s: dims (%d, %d, %d) must be >= 1 with a product in [1, 2^26] "
                     "(ANERF_SIMPLIFY_MAX_CELLS)", who, (int)dims[0], (int)dims[1], (int)dims[2]);
    plan(nv, nt, cells, pl);
    for (int a = 0; a < 3; ++a) {
        g->o[a] = origin[a];
        g->n[a] = dims[a];
    }
    g->cell = cell;
    return check_workspace(who, ws, ws_bytes, pl->bytes, 8, ANERF_EINVAL, "anerf_mesh_simplify_workspace");
}

}  // namespace

extern "C" {

size_t anerf_mesh_simplify_workspace(int64_t n_vertices, int64_t n_tri, int64_t n_cells) {
    Plan pl;
    if (!plan(n_vertices, n_tri, n_cells, &pl)) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_simplify_workspace: n_vertices and n_tri must be in [0, 2^31), "
                                          "n_cells in [1, 2^26] (ANERF_SIMPLIFY_MAX_CELLS)");
        return 0;
    }
    return pl.bytes;
}

int anerf_mesh_simplify_count(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                              const float* origin, float cell, const int32_t* dims, void* ws, size_t ws_bytes,
                              int64_t* totals_dev, void* stream) {
    Plan pl;
    Grid g;
    const int rc = check("anerf_mesh_simplify_count", vertices, n_vertices, triangles, n_tri, origin, cell, dims, ws,
                         ws_bytes, &pl, &g);
    if (rc != ANERF_OK) return rc;
    if (!totals_dev) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_simplify_count: NULL totals");
    hipStream_t s = (hipStream_t)stream;
    const int nv = (int)n_vertices;
    const long long nt = (long long)n_tri, cells = (long long)g.n[0] * g.n[1] * g.n[2];
    int *table = at<int>(ws, pl.table), *rep = at<int>(ws, pl.rep), *cnt = at<int>(ws, pl.cnt);
    int *row_cnt = at<int>(ws, pl.row_cnt), *row_off = at<int>(ws, pl.row_off);
    int *long_list = at<int>(ws, pl.long_list), *n_long = at<int>(ws, pl.n_long);
    int *flag = at<int>(ws, pl.flag), *idx = at<int>(ws, pl.idx);
    long long* sums = at<long long>(ws, pl.sums);
    unsigned long long* keys = at<unsigned long long>(ws, pl.keys);
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(cells)), dim3(NTHR), 0, s, table, cells, n_long);
    if (nv > 0) {
        hipLaunchKernelGGL(key_kernel, dim3(blocks_for(nv)), dim3(NTHR), 0, s, vertices, nv, g, table, sums, cnt,
                           row_cnt);
        hipLaunchKernelGGL(sum_kernel, dim3(blocks_for(nv)), dim3(NTHR), 0, s, vertices, nv, g, (const int*)table, rep,
                           sums, cnt);
    }
    if (nv > 0 && nt > 0) {
        hipLaunchKernelGGL(owner_count_kernel, dim3(blocks_for(nt)), dim3(NTHR), 0, s, triangles, nt, nv,
                           (const int*)rep, row_cnt);
        exclusive_scan<false, SHORT_ROW>(row_cnt, nv, row_off, at<int>(ws, pl.tiles), nullptr, long_list, n_long, s);
        hipLaunchKernelGGL(fill_rows_kernel, dim3(blocks_for(nt)), dim3(NTHR), 0, s, triangles, nt, nv, (const int*)rep,
                           row_cnt, (const int*)row_off, keys, idx);
    }
    if (nt > 0) {  // (without vertices every triangle leaves: the kernel touches no row)
        hipLaunchKernelGGL(dedup_kernel, dim3(blocks_for(nt)), dim3(NTHR), 0, s, triangles, nt, nv, (const int*)rep,
                           (const int*)row_off, (const unsigned long long*)keys, (const int*)idx, flag);
        if (nv > 0 && nt > SHORT_ROW)
            hipLaunchKernelGGL(long_rows_kernel, dim3(long_blocks(nt, SHORT_ROW)), dim3(NTHR), 0, s, (const int*)row_off,
                               keys, idx, nv, nt, (const int*)long_list, (const int*)n_long, flag);
    }
    hipLaunchKernelGGL(out_count_kernel, dim3(pl.out.nblocks), dim3(NTHR), 0, s, (const int*)rep, (long long)nv,
                       (const int*)flag, nt, pl.out.counts(ws), pl.out.nblocks);
    scan_block_sums(pl.out, ws, totals_dev, s);
    return launched("anerf_mesh_simplify_count");
}

int anerf_mesh_simplify_emit(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                             const float* origin, float cell, const int32_t* dims, const void* ws, size_t ws_bytes,
                             float* out_vertices, int64_t n_out_v, int32_t* out_triangles, int64_t n_out_t,
                             int32_t* vertex_map, int32_t* representatives, void* stream) {
    Plan pl;
    Grid g;
    const int rc = check("anerf_mesh_simplify_emit", vertices, n_vertices, triangles, n_tri, origin, cell, dims, ws,
                         ws_bytes, &pl, &g);
    if (rc != ANERF_OK) return rc;
    if (n_out_v < 0 || n_out_v > n_vertices || n_out_t < 0 || n_out_t > n_tri)
        return failf(ANERF_EINVAL, "anerf_mesh_simplify_emit: n_out_v %lld / n_out_t %lld are not the counted totals "
                     "(at most n_vertices %lld / n_tri %lld)", (long long)n_out_v, (long long)n_out_t,
                     (long long)n_vertices, (long long)n_tri);
    if ((n_vertices > 0 && !vertex_map) || (n_out_v > 0 && (!out_vertices || !representatives)) ||
        (n_out_t > 0 && !out_triangles))
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_simplify_emit: NULL output with a non-zero extent");
    hipStream_t s = (hipStream_t)stream;
    const int nv = (int)n_vertices;
    const long long nt = (long long)n_tri;
    const long long* base = (const long long*)ws;
    const int* rep = at<const int>(ws, pl.rep);
    if (nv > 0) {
        hipLaunchKernelGGL(vertices_kernel, dim3(tiles_for(nv)), dim3(NTHR), 0, s, vertices, (long long)nv, g, rep,
                           (const long long*)at<const long long>(ws, pl.sums), at<const int>(ws, pl.cnt), base,
                           out_vertices, (long long)n_out_v, vertex_map, representatives);
        hipLaunchKernelGGL(members_kernel, dim3(blocks_for(nv)), dim3(NTHR), 0, s, rep, nv, vertex_map);
    }
    if (nv > 0 && nt > 0 && n_out_t > 0)
        hipLaunchKernelGGL(triangles_kernel, dim3(tiles_for(nt)), dim3(NTHR), 0, s, triangles, nt, nv,
                           at<const int>(ws, pl.flag), base + pl.out.nblocks, (const int*)vertex_map, out_triangles,
                           (long long)n_out_t);
    return launched("anerf_mesh_simplify_emit");
}

}  // extern "C"

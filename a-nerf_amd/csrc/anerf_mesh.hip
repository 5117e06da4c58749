// anerf_mesh.hip — connected components of an indexed triangle mesh and its stable compaction, its vertex adjacency
// (CSR) and Laplacian / Taubin smoothing over it, on the device.
//
// The iso-surface of a noisy density (anerf_iso.hip) is the body plus detached blobs and closed cavity surfaces;
// the reference leaves them to trimesh's split() on the host.  Here the triangle list stays in HBM:
//
//   anerf_mesh_components     init_kernel      parent[v] = v, the tallies and the component counter zeroed
//                             seed_kernel      per triangle: parent[v] = min(parent[v], the triangle's smallest id) --
//                                              a first forest of short trees (the smallest smaller neighbour)
//                             hook_kernel      per triangle (a, b, c): unite(a, b), unite(b, c) -- a lock-free
//                                              union-find, the larger root hooked under the smaller
//                             flatten_kernel   per vertex: root[v] = its tree's root, vert_count[root] += 1, the roots
//                                              counted (separate launch: the kernel boundary publishes the hooks);
//                                              the tallies are summed per wave, then per workgroup, before one add
//                             tri_tally_kernel per triangle: tri_count[root[first vertex]] += 1
//   anerf_mesh_compact_count  count_kernel     per block: the kept vertices and surviving triangles of its tile
//                             scan_kernel      exclusive scan of the block sums (one workgroup, 64-bit), the totals
//   anerf_mesh_compact_emit   vertex_kernel    the same flags scanned within the block: vertex_map, kept
//                             triangle_kernel  the surviving triangles, ids through vertex_map (separate launch)
//
//   anerf_mesh_adjacency_count  adj_count_kernel   per triangle: the pairs it lists, counted per vertex (int atomics)
//                             (exclusive_scan)   the raw row offsets; the rows of more than 64 raw entries listed
//                             adj_fill_kernel    the raw rows through per-vertex cursors, in arrival order
//                             adj_rows_kernel    per vertex: a row of <= 64 raw entries sorted by its thread, the
//                                                distinct count and the boundary flag from its runs
//                             adj_long_rows_kernel   per listed row: one workgroup, a bitonic network (LDS or global)
//                             (exclusive_scan)   the distinct counts -> offsets, the totals
//   anerf_mesh_adjacency_emit   adj_emit_kernel, adj_emit_long_kernel   the distinct entries of the sorted rows
//   anerf_mesh_smooth         smooth_step_kernel per vertex: one Jacobi step over its CSR row; one launch per step
// (the adjacency's contract and the reason for the launch per step: further down and DESIGN.md)
//
// The union-find's invariants, from the end of seed_kernel on (DESIGN.md has the termination argument; the seed only
// has to leave a forest with parent[x] <= x whose trees lie inside components -- it may drop an edge it saw, since
// hook_kernel unites the ends of every edge again):
//   (1) parent[x] <= x always, and a slot only ever decreases: a root slot (parent[x] == x) changes once, by the
//       compare-and-swap that hooks it under a smaller id; a non-root slot by atomicMin to a higher ancestor;
//   (2) every value a slot ever held is an ancestor of x from then on (hooks add edges above roots only, compression
//       replaces a parent by a higher ancestor), so a STALE read of a parent still yields an ancestor -- it costs
//       steps, never correctness.  hook_kernel reads parents with relaxed agent-scope atomic loads all the same
//       (they skip the CU's L1, which another CU's stores never refresh), and the one decision that must be fresh,
//       "x is still a root", is taken by the compare-and-swap itself, which returns the slot's current value when
//       it fails.
// No thread waits for another: a failed compare-and-swap means another thread hooked that root (progress), and the
// loser continues from the value the failure returned; every round of a walk moves to a strictly smaller id.
// Every component ends as one tree whose edges lead to strictly smaller ids, so its root is its smallest vertex id
// whatever the schedule: the outputs are deterministic (the tallies are integer atomics).
//
// Compaction keeps both outputs in their original relative order: count -> scan -> emit without atomics, the
// pattern of anerf_scan.hpp (256 threads x 4 consecutive items per workgroup), whose tiles, block scan, scan_kernel,
// workspace layout and host helpers this unit shares with anerf_iso.hip.  The adjacency's rows are built with the row
// toolkit of the same header (exclusive_scan, take_slot, the long-row list and its walk, bitonic_sort), which this
// unit shares with anerf_simplify.hip; its own are the pairs, the short rows' insertion sort, LDS_ROW and the emit.
#include "anerf_scan.hpp"

namespace {

constexpr int TALLY_THR = 1024;  // threads per workgroup of the two tallying kernels
constexpr int TALLY_WAVES = TALLY_THR / 64;

__device__ __forceinline__ int ld_parent(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of v's tree, for a launch in which no hook runs (flatten_kernel: one thread per vertex).  The thread
// walks up through the ancestors' CURRENT parents and publishes every ancestor it reaches in its own slot (by
// atomicMin, so that invariant (1) holds under races).  Ancestors have smaller ids, so their threads run at the
// same time or earlier and publish their own progress: the hops double in length (pointer jumping), about
// log2(depth) of them instead of depth.  Each hop moves to a strictly smaller id: at most v of them in any case.
// Whether p is a root is asked with a plain load first, which the CU's L1 may serve: the roots are final in that
// launch and the L1 holds nothing older than its start, so "parent[p] == p" is true wherever it is read from -- and
// for the one big component of a body mesh every walk ends on that same word, which the L1s share out.  A parent
// to walk on is read at agent scope, to see the other walkers' progress.
__device__ __forceinline__ int find_root(int* parent, int v) {
    int p = ld_parent(parent + v);
    if (p == v) return v;
    while (parent[p] != p) {
        p = ld_parent(parent + p);  // (p is no root: its parent is smaller)
        __hip_atomic_fetch_min(parent + v, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return p;
}

// Link the trees of a and b (Rem's walk): of the two, the larger id moves up to its parent, until they meet -- at
// their lowest common ancestor, since both ancestor chains descend and share their tail, so neither can step past
// it -- or until the larger is a root, which is then hooked under the other (smaller; root or not, it lies in the
// other tree).  Two vertices of one tree never touch the root unless it is their meeting point: in the one big
// component of a body mesh nearly every walk would otherwise end on the same word.  A node that moves twice in
// a row is pointed at its grandparent on the way (path splitting, by atomicMin).
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    int p = -1;  // parent[a] where already read, else -1
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
            p = -1;
        }
        if (p < 0) p = ld_parent(parent + a);
        if (p == a) {  // a root, as far as that read knows: the compare-and-swap decides
            if (__hip_atomic_compare_exchange_strong(parent + a, &p, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                return;
            // another thread hooked a under p < a (the fresh value): go on from there
        } else if (p > b) {  // a's parent moves next as well
            const int gp = ld_parent(parent + p);
            if (gp != p) __hip_atomic_fetch_min(parent + a, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a = p;
            p = gp;  // (gp == p: a root, handled in the next round)
            continue;
        }
        a = p;
        p = -1;
    }
}

__global__ __launch_bounds__(NTHR) void init_kernel(int* __restrict__ parent, int* __restrict__ tri_count,
                                                    int* __restrict__ vert_count, int nv,
                                                    unsigned long long* __restrict__ n_components) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v < nv) {
        parent[v] = (int)v;
        tri_count[v] = 0;
        vert_count[v] = 0;
    }
    if (v == 0) *n_components = 0ull;
}

// Without it every vertex starts as a root and the first hooks, all racing, chain neighbouring ids one by one
// (trees thousands deep on a marching-cubes mesh, whose ids follow the grid); the smallest smaller neighbour is a
// whole grid slice of ids lower.
__global__ __launch_bounds__(NTHR) void seed_kernel(const int* __restrict__ tri, long long nt, int nv, int* parent) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= nt) return;
    const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    if (!in_range(a, b, c, nv)) return;
    const int m = min(a, min(b, c));
    if (a != m) __hip_atomic_fetch_min(parent + a, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b != m) __hip_atomic_fetch_min(parent + b, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c != m) __hip_atomic_fetch_min(parent + c, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(NTHR) void hook_kernel(const int* __restrict__ tri, long long nt, int nv, int* parent) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= nt) return;
    const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    if (!in_range(a, b, c, nv)) return;  // (a bad list cannot write out of bounds)
    unite(parent, a, b);
    unite(parent, b, c);
}

// counts[key] += 1 for every thread with key >= 0, all threads of the workgroup calling.  Each wave sums its lanes
// per distinct key (one round per key: a wave of consecutive vertices or triangles lies in one or two components);
// the sums of the waves' first keys are merged over the workgroup before one add goes out, the others are added
// by the wave.  Adds to one address are served one after the other, so a thread-per-item add would queue up
// behind the big component's counter.
__device__ __forceinline__ void block_tally(int* counts, int key, int* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long todo = __ballot(key >= 0);
    int k0 = -1, n0 = 0;
    while (todo) {  // (wave-uniform)
        const int lead = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, lead);
        const unsigned long long same = __ballot(key == k);
        if (k0 < 0) {
            k0 = k;
            n0 = __popcll(same);
        } else if (lane == lead) {
            atomicAdd(counts + k, __popcll(same));
        }
        todo &= ~same;
    }
    if (lane == 0) {
        lds[wave] = k0;
        lds[TALLY_WAVES + wave] = n0;
    }
    __syncthreads();
    if (threadIdx.x < TALLY_WAVES) {  // thread w: wave w's first key, added by the first wave that has it
        const int k = lds[threadIdx.x];
        bool first = true;
        int sum = 0;
        for (int u = 0; u < TALLY_WAVES; ++u) {
            if (lds[u] != k) continue;
            if (u < (int)threadIdx.x) first = false;
            sum += lds[TALLY_WAVES + u];
        }
        if (k >= 0 && first) atomicAdd(counts + k, sum);
    }
}

__global__ __launch_bounds__(TALLY_THR) void flatten_kernel(int* parent, int nv, int* __restrict__ root,
                                                            int* vert_count, unsigned long long* n_components) {
    __shared__ int lds[2 * TALLY_WAVES];
    const long long v = (long long)blockIdx.x * TALLY_THR + threadIdx.x;
    int r = -1;
    if (v < nv) {
        r = find_root(parent, (int)v);  // (no hook runs any more: r is final)
        root[v] = r;
    }
    block_tally(vert_count, r, lds);
    const unsigned long long roots = __ballot(r >= 0 && r == (int)v);
    if ((threadIdx.x & 63) == 0 && roots) atomicAdd(n_components, (unsigned long long)__popcll(roots));
}

__global__ __launch_bounds__(TALLY_THR) void tri_tally_kernel(const int* __restrict__ tri, long long nt, int nv,
                                                              const int* __restrict__ root, int* tri_count) {
    __shared__ int lds[2 * TALLY_WAVES];
    const long long i = (long long)blockIdx.x * TALLY_THR + threadIdx.x;
    int r = -1;
    if (i < nt) {
        const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
        if (in_range(a, b, c, nv)) r = root[a];
    }
    block_tally(tri_count, r, lds);
}

// ------------------------------------------------------------------ compaction
struct Lists {
    const unsigned char* keep;
    const int* tri;
    long long nv, nt;
};

__device__ __forceinline__ bool vertex_kept(const Lists& l, long long p) { return p < l.nv && l.keep[p] != 0; }
__device__ __forceinline__ bool triangle_kept(const Lists& l, long long p) {
    if (p >= l.nt) return false;
    const int a = l.tri[3 * p], b = l.tri[3 * p + 1], c = l.tri[3 * p + 2];
    if (!in_range(a, b, c, (int)l.nv)) return false;
    return l.keep[a] != 0 && l.keep[b] != 0 && l.keep[c] != 0;
}

__global__ __launch_bounds__(NTHR) void count_kernel(Lists l, int* __restrict__ block_counts, int nblocks) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    int nv = 0, nt = 0;
    for (int it = 0; it < ITEMS; ++it) {
        nv += vertex_kept(l, first + it) ? 1 : 0;
        nt += triangle_kept(l, first + it) ? 1 : 0;
    }
    int tv, tt;
    block_exclusive_scan(nv, lds, tv);
    block_exclusive_scan(nt, lds, tt);
    if (threadIdx.x == 0) {
        block_counts[blockIdx.x] = tv;
        block_counts[nblocks + blockIdx.x] = tt;
    }
}

__global__ __launch_bounds__(NTHR) void vertex_kernel(Lists l, const long long* __restrict__ base,
                                                      int* __restrict__ vertex_map, int* __restrict__ kept,
                                                      long long max_kept) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    bool k[ITEMS];
    int n = 0;
    for (int it = 0; it < ITEMS; ++it) {
        k[it] = vertex_kept(l, first + it);
        n += k[it] ? 1 : 0;
    }
    int total;
    long long id = base[blockIdx.x] + block_exclusive_scan(n, lds, total);
    for (int it = 0; it < ITEMS; ++it) {
        const long long p = first + it;
        if (p >= l.nv) break;
        vertex_map[p] = k[it] ? (int)id : -1;
        if (k[it]) {
            if (id < max_kept) kept[id] = (int)p;
            ++id;
        }
    }
}

__global__ __launch_bounds__(NTHR) void triangle_kernel(Lists l, const long long* __restrict__ base_t,
                                                        const int* __restrict__ vertex_map, int* __restrict__ out,
                                                        long long max_triangles) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    bool k[ITEMS];
    int n = 0;
    for (int it = 0; it < ITEMS; ++it) {
        k[it] = triangle_kept(l, first + it);
        n += k[it] ? 1 : 0;
    }
    int total;
    long long id = base_t[blockIdx.x] + block_exclusive_scan(n, lds, total);
    for (int it = 0; it < ITEMS; ++it) {
        if (!k[it]) continue;
        if (id < max_triangles) {
            const int* s = l.tri + 3 * (first + it);
            int* o = out + 3 * id;
            o[0] = vertex_map[s[0]];
            o[1] = vertex_map[s[1]];
            o[2] = vertex_map[s[2]];
        }
        ++id;
    }
}

// The compaction's workspace is the scan's base | block_counts and nothing more: its plan is the ScanSpace.
bool plan(int64_t nv, int64_t nt, ScanSpace* pl) {
    if (nv < 0 || nt < 0 || nv > MAXN || nt > MAXN) return false;
    const int nblocks = tiles_for(nv > nt ? nv : nt);
    *pl = scan_space(nblocks < 1 ? 1 : nblocks);  // (empty lists still get their totals written)
    return true;
}

int check_compact(const char* who, const uint8_t* keep, int64_t nv, const int32_t* tri, int64_t nt, const void* ws,
                  size_t ws_bytes, ScanSpace* pl) {
    if (!plan(nv, nt, pl))
        return failf(ANERF_EINVAL, "%s: n_vertices %lld / n_tri %lld must be in [0, 2^31)", who, (long long)nv,
                     (long long)nt);
    if ((nv > 0 && !keep) || (nt > 0 && !tri) || !ws)
        return failf(ANERF_EINVAL, "%s: NULL keep, triangles or workspace", who);
    return check_workspace(who, ws, ws_bytes, pl->bytes, 8, ANERF_EINVAL, "anerf_mesh_compact_workspace");
}

// ------------------------------------------------------------------ vertex adjacency (CSR)
constexpr int SHORT_ROW = 64;         // the raw entries one thread sorts at most; longer rows go to a workgroup
constexpr int LDS_ROW = 8192;         // the padded length up to which a long row's network runs over LDS (32 KB)

// Workspace, in ints; everything whose size depends on V alone comes first, so that anerf_mesh_adjacency_emit
// finds it without the triangle count:
//   raw_off[V + 1] | cnt[V] | long_list[V] | n_long | tiles[3 nb] (both scans') | raw[6 T]
// cnt holds the listed pairs per vertex (count), counts down to 0 as the cursor of the fill, then holds the
// distinct degree (the row kernels), which the second scan turns into `offsets`.
struct AdjPlan {
    size_t raw_off, cnt, long_list, n_long, tiles, raw;  // offsets in ints
};

bool adj_plan(int64_t nv, AdjPlan* pl) {
    if (nv < 0 || nv > MAXN) return false;
    size_t o = 0;
    pl->raw_off = o, o += (size_t)nv + 1;
    pl->cnt = o, o += (size_t)nv;
    pl->long_list = o, o += (size_t)nv;
    pl->n_long = o, o += 1;
    pl->tiles = o, o += scan_ints((int)nv, true);  // (no vertices: offsets[0] and the totals are still written)
    pl->raw = o;
    return true;
}

__global__ __launch_bounds__(NTHR) void adj_zero_kernel(int* __restrict__ cnt, int nv, int* __restrict__ n_long) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v < nv) cnt[v] = 0;
    if (v == 0) *n_long = 0;
}

// The pairs a triangle lists, per first end: (a,b) (a,c) | (b,a) (b,c) | (c,a) (c,b), equal ends dropped.
__global__ __launch_bounds__(NTHR) void adj_count_kernel(const int* __restrict__ tri, long long nt, int nv, int* cnt) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= nt) return;
    const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    if (!in_range(a, b, c, nv)) return;
    const int na = (a != b) + (a != c), nb = (b != a) + (b != c), nc = (c != a) + (c != b);
    if (na) atomicAdd(cnt + a, na);
    if (nb) atomicAdd(cnt + b, nb);
    if (nc) atomicAdd(cnt + c, nc);
}

// Every listed pair takes a slot of its own in row x (cnt: its cursor), in arrival order (sorted afterwards).
__device__ __forceinline__ void adj_put(int* cnt, const int* __restrict__ raw_off, int* __restrict__ raw, int x,
                                        int y) {
    if (x == y) return;
    const int slot = take_slot(cnt, x);
    if (slot >= 0) raw[raw_off[x] + slot] = y;  // (slot < the row's count: inside the row)
}

__global__ __launch_bounds__(NTHR) void adj_fill_kernel(const int* __restrict__ tri, long long nt, int nv, int* cnt,
                                                        const int* __restrict__ raw_off, int* __restrict__ raw) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= nt) return;
    const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    if (!in_range(a, b, c, nv)) return;
    adj_put(cnt, raw_off, raw, a, b);
    adj_put(cnt, raw_off, raw, a, c);
    adj_put(cnt, raw_off, raw, b, a);
    adj_put(cnt, raw_off, raw, b, c);
    adj_put(cnt, raw_off, raw, c, a);
    adj_put(cnt, raw_off, raw, c, b);
}

// One thread per vertex: a row of at most SHORT_ROW raw entries is sorted in place (insertion sort) and walked once
// for its distinct entries and for a run of length 1 (a pair listed once: a boundary edge); a longer row is on the
// list of adj_long_rows_kernel (the scan of the raw counts put it there).
__global__ __launch_bounds__(NTHR) void adj_rows_kernel(const int* __restrict__ raw_off, int* __restrict__ raw, int nv,
                                                        int* __restrict__ deg, unsigned char* __restrict__ boundary) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v >= nv) return;
    const int b = raw_off[v], n = raw_off[v + 1] - b;
    if (n > SHORT_ROW) return;
    int* r = raw + b;
    for (int i = 1; i < n; ++i) {
        const int x = r[i];
        int j = i;
        for (; j > 0 && r[j - 1] > x; --j) r[j] = r[j - 1];
        r[j] = x;
    }
    int d = 0, bnd = 0;
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && r[j] == r[i]) ++j;
        ++d;
        if (j - i == 1) bnd = 1;
        i = j;
    }
    deg[v] = d;
    boundary[v] = (unsigned char)bnd;
}

// One workgroup per listed row (for_each_long_row): sorted by the bitonic network of anerf_scan.hpp, over LDS where
// the padded row fits and in place over global memory where not; then the distinct count and the boundary flag from
// the sorted row, every thread looking at its entries' two neighbours.
__global__ __launch_bounds__(NTHR) void adj_long_rows_kernel(const int* __restrict__ raw_off, int* raw, int nv,
                                                             int* __restrict__ deg, unsigned char* __restrict__ boundary,
                                                             const int* __restrict__ long_list,
                                                             const int* __restrict__ n_long) {
    __shared__ int row[LDS_ROW];
    __shared__ int tally[2];
    for_each_long_row(long_list, n_long, nv, [&](int v) {
        const int b = raw_off[v];
        const unsigned n = (unsigned)max(raw_off[v + 1] - b, 0);
        int* g = raw + b;
        const int lp = padded_log2(n);
        const bool in_lds = (1u << lp) <= (unsigned)LDS_ROW;
        if (threadIdx.x == 0) tally[0] = tally[1] = 0;
        if (in_lds) {
            for (unsigned i = threadIdx.x; i < n; i += NTHR) row[i] = g[i];
            __syncthreads();
            bitonic_sort(IntRow{row}, n, lp);
            for (unsigned i = threadIdx.x; i < n; i += NTHR) g[i] = row[i];
        } else {
            __syncthreads();
            bitonic_sort(IntRow{g}, n, lp);
        }
        __syncthreads();  // (the row in global memory is complete for the whole workgroup)
        int d = 0, single = 0;
        for (unsigned i = threadIdx.x; i < n; i += NTHR) {
            const int x = g[i];
            const bool first = i == 0 || g[i - 1] != x, last = i + 1 == n || g[i + 1] != x;
            d += first ? 1 : 0;
            single |= (first && last) ? 1 : 0;
        }
        atomicAdd(&tally[0], d);
        atomicOr(&tally[1], single);
        __syncthreads();
        if (threadIdx.x == 0) {
            deg[v] = tally[0];
            boundary[v] = (unsigned char)tally[1];
        }
        __syncthreads();  // (row and tally are free for the next row)
    });
}

// A row of the emit pass: its bounds clamped to the part of the workspace that holds the raw rows (the emit entry
// does not know T; a workspace that is not the count pass's cannot make it read outside).
__device__ __forceinline__ int clamp_raw(int x, long long raw_cap) {
    return x < 0 ? 0 : (x > raw_cap ? (int)raw_cap : x);
}

// One thread per vertex: the distinct entries of a sorted short row, to neighbors[offsets[v] ...].
__global__ __launch_bounds__(NTHR) void adj_emit_kernel(const int* __restrict__ raw_off, const int* __restrict__ raw,
                                                        int nv, long long raw_cap, const int* __restrict__ offsets,
                                                        int* __restrict__ neighbors, long long max_neighbors) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v >= nv) return;
    const int b = clamp_raw(raw_off[v], raw_cap), n = clamp_raw(raw_off[v + 1], raw_cap) - b;
    if (n > SHORT_ROW) return;  // (adj_emit_long_kernel's)
    const int* r = raw + b;
    long long pos = offsets[v];
    const long long end = min((long long)offsets[v + 1], max_neighbors);
    int prev = 0;
    for (int i = 0; i < n; ++i) {
        const int x = r[i];
        if (i == 0 || x != prev) {
            if (pos >= 0 && pos < end) neighbors[pos] = x;
            ++pos;
        }
        prev = x;
    }
}

// One workgroup per listed long row: tiles of NTHR entries, the "first of its run" flags scanned within the tile.
__global__ __launch_bounds__(NTHR) void adj_emit_long_kernel(const int* __restrict__ raw_off,
                                                             const int* __restrict__ raw, int nv, long long raw_cap,
                                                             const int* __restrict__ long_list,
                                                             const int* __restrict__ n_long,
                                                             const int* __restrict__ offsets, int* __restrict__ neighbors,
                                                             long long max_neighbors) {
    __shared__ int lds[NTHR];
    for_each_long_row(long_list, n_long, nv, [&](int v) {
        const int b = clamp_raw(raw_off[v], raw_cap), n = clamp_raw(raw_off[v + 1], raw_cap) - b;
        const int* r = raw + b;
        const long long end = min((long long)offsets[v + 1], max_neighbors);
        long long carry = offsets[v];
        for (long long start = 0; start < n; start += NTHR) {
            const long long i = start + threadIdx.x;
            const bool first = i < n && (i == 0 || r[i] != r[i - 1]);
            int total;
            const long long pos = carry + block_exclusive_scan(first ? 1 : 0, lds, total);
            if (first && pos >= 0 && pos < end) neighbors[pos] = r[i];
            carry += total;
        }
    });
}

// ------------------------------------------------------------------ smoothing
// One Jacobi step p' = p + w (mean of the neighbours - p), one thread per vertex; the sum runs over the row in its
// stored (ascending) order, every operation separately rounded (-ffp-contract=off), the division correctly rounded.
// A bad CSR cannot make it read outside: row bounds are clamped to [0, ne], a neighbour outside [0, nv) is skipped
// and not counted.
__global__ __launch_bounds__(NTHR) void smooth_step_kernel(const float* __restrict__ p, int nv,
                                                           const int* __restrict__ offsets,
                                                           const int* __restrict__ neighbors, int ne,
                                                           const unsigned char* __restrict__ pinned, float w,
                                                           float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (v >= nv) return;
    const float x = p[3 * v], y = p[3 * v + 1], z = p[3 * v + 2];
    float ox = x, oy = y, oz = z;
    if (!(pinned && pinned[v])) {
        const int b = min(max(offsets[v], 0), ne), e = min(max(offsets[v + 1], 0), ne);
        float sx = 0.f, sy = 0.f, sz = 0.f;
        int d = 0;
        for (int k = b; k < e; ++k) {
            const int u = neighbors[k];
            if ((unsigned)u >= (unsigned)nv) continue;
            const float ux = p[3 * (long long)u], uy = p[3 * (long long)u + 1], uz = p[3 * (long long)u + 2];
            if (d == 0) {
                sx = ux, sy = uy, sz = uz;
            } else {
                sx = sx + ux, sy = sy + uy, sz = sz + uz;
            }
            ++d;
        }
        if (d > 0) {
            const float fd = (float)d;
            ox = x + w * (__fdiv_rn(sx, fd) - x);
            oy = y + w * (__fdiv_rn(sy, fd) - y);
            oz = z + w * (__fdiv_rn(sz, fd) - z);
        }
    }
    out[3 * v] = ox;
    out[3 * v + 1] = oy;
    out[3 * v + 2] = oz;
}

bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" {

size_t anerf_mesh_components_workspace(int64_t n_vertices, int64_t n_tri) {
    if (n_vertices < 0 || n_tri < 0 || n_vertices > MAXN || n_tri > MAXN) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_components_workspace: counts must be in [0, 2^31)");
        return 0;
    }
    return (size_t)n_vertices * sizeof(int);  // the parent array
}

int anerf_mesh_components(const int32_t* triangles, int64_t n_tri, int64_t n_vertices, int32_t* root,
                          int32_t* tri_count, int32_t* vert_count, int64_t* n_components, void* ws, size_t ws_bytes,
                          void* stream) {
    if (n_tri < 0 || n_vertices < 0 || n_tri > MAXN || n_vertices > MAXN)
        return failf(ANERF_EINVAL, "anerf_mesh_components: n_tri %lld / n_vertices %lld must be in [0, 2^31)",
                     (long long)n_tri, (long long)n_vertices);
    if (!n_components) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_components: NULL n_components");
    if (n_tri > 0 && !triangles) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_components: NULL triangles");
    if (n_vertices > 0 && (!root || !tri_count || !vert_count || !ws))
        return anerf_internal_fail(ANERF_EINVAL,
                                   "anerf_mesh_components: NULL root, tri_count, vert_count or workspace");
    const int rc = check_workspace("anerf_mesh_components", ws, ws_bytes, (size_t)n_vertices * sizeof(int), 4,
                                   ANERF_EINVAL, "anerf_mesh_components_workspace");
    if (rc != ANERF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int nv = (int)n_vertices;
    int* parent = (int*)ws;
    unsigned long long* nc = (unsigned long long*)n_components;
    const int vblocks = nv > 0 ? blocks_for(nv) : 1;  // (n_vertices == 0: the counter is still zeroed)
    hipLaunchKernelGGL(init_kernel, dim3(vblocks), dim3(NTHR), 0, s, parent, tri_count, vert_count, nv, nc);
    if (nv > 0) {
        if (n_tri > 0) {
            hipLaunchKernelGGL(seed_kernel, dim3(blocks_for(n_tri)), dim3(NTHR), 0, s, triangles, (long long)n_tri, nv,
                               parent);
            hipLaunchKernelGGL(hook_kernel, dim3(blocks_for(n_tri)), dim3(NTHR), 0, s, triangles, (long long)n_tri, nv,
                               parent);
        }
        hipLaunchKernelGGL(flatten_kernel, dim3(blocks_for(nv, TALLY_THR)), dim3(TALLY_THR), 0, s, parent, nv, root,
                           vert_count, nc);
        if (n_tri > 0)
            hipLaunchKernelGGL(tri_tally_kernel, dim3(blocks_for(n_tri, TALLY_THR)), dim3(TALLY_THR), 0, s, triangles,
                               (long long)n_tri, nv, (const int*)root, tri_count);
    }
    return launched("anerf_mesh_components");
}

size_t anerf_mesh_compact_workspace(int64_t n_vertices, int64_t n_tri) {
    ScanSpace pl;
    if (!plan(n_vertices, n_tri, &pl)) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_compact_workspace: counts must be in [0, 2^31)");
        return 0;
    }
    return pl.bytes;
}

int anerf_mesh_compact_count(const uint8_t* keep, int64_t n_vertices, const int32_t* triangles, int64_t n_tri, void* ws,
                             size_t ws_bytes, int64_t* totals_dev, void* stream) {
    ScanSpace pl;
    const int rc = check_compact("anerf_mesh_compact_count", keep, n_vertices, triangles, n_tri, ws, ws_bytes, &pl);
    if (rc != ANERF_OK) return rc;
    if (!totals_dev) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_compact_count: NULL totals");
    const Lists l = {keep, triangles, (long long)n_vertices, (long long)n_tri};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(count_kernel, dim3(pl.nblocks), dim3(NTHR), 0, s, l, pl.counts(ws), pl.nblocks);
    scan_block_sums(pl, ws, totals_dev, s);
    return launched("anerf_mesh_compact_count");
}

int anerf_mesh_compact_emit(const uint8_t* keep, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                            const void* ws, size_t ws_bytes, int32_t* vertex_map, int32_t* kept, int64_t max_kept,
                            int32_t* triangles_out, int64_t max_triangles, void* stream) {
    ScanSpace pl;
    const int rc = check_compact("anerf_mesh_compact_emit", keep, n_vertices, triangles, n_tri, ws, ws_bytes, &pl);
    if (rc != ANERF_OK) return rc;
    if (max_kept < 0 || max_triangles < 0 || max_kept > MAXN || max_triangles > MAXN)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_compact_emit: capacities must be in [0, 2^31)");
    if ((n_vertices > 0 && !vertex_map) || (max_kept > 0 && !kept) || (max_triangles > 0 && !triangles_out))
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_compact_emit: NULL output with a non-zero extent");
    const Lists l = {keep, triangles, (long long)n_vertices, (long long)n_tri};
    const long long* base = (const long long*)ws;
    hipStream_t s = (hipStream_t)stream;
    if (n_vertices > 0)
        hipLaunchKernelGGL(vertex_kernel, dim3(pl.nblocks), dim3(NTHR), 0, s, l, base, vertex_map, kept,
                           (long long)max_kept);
    if (n_tri > 0 && max_triangles > 0)
        hipLaunchKernelGGL(triangle_kernel, dim3(pl.nblocks), dim3(NTHR), 0, s, l, base + pl.nblocks,
                           (const int*)vertex_map, triangles_out, (long long)max_triangles);
    return launched("anerf_mesh_compact_emit");
}

size_t anerf_mesh_adjacency_workspace(int64_t n_vertices, int64_t n_tri) {
    AdjPlan pl;
    if (!adj_plan(n_vertices, &pl) || n_tri < 0 || n_tri > MAXN / 6) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_adjacency_workspace: n_vertices must be in [0, 2^31) and "
                                          "6 n_tri below 2^31");
        return 0;
    }
    return (pl.raw + (size_t)6 * (size_t)n_tri) * sizeof(int);
}

int anerf_mesh_adjacency_count(const int32_t* triangles, int64_t n_tri, int64_t n_vertices, void* ws, size_t ws_bytes,
                               int32_t* offsets, uint8_t* boundary, int64_t* totals_dev, void* stream) {
    AdjPlan pl;
    if (!adj_plan(n_vertices, &pl) || n_tri < 0 || n_tri > MAXN / 6)
        return failf(ANERF_EINVAL, "anerf_mesh_adjacency_count: n_vertices %lld must be in [0, 2^31) and 6 n_tri "
                     "(n_tri %lld) below 2^31", (long long)n_vertices, (long long)n_tri);
    if (!offsets || !totals_dev || !ws || (n_tri > 0 && !triangles) || (n_vertices > 0 && !boundary))
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_adjacency_count: NULL offsets, totals or workspace, or "
                                                 "NULL triangles or boundary with a non-zero extent");
    const int rc = check_workspace("anerf_mesh_adjacency_count", ws, ws_bytes,
                                   (pl.raw + (size_t)6 * (size_t)n_tri) * sizeof(int), 4, ANERF_EINVAL,
                                   "anerf_mesh_adjacency_workspace");
    if (rc != ANERF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int nv = (int)n_vertices;
    const long long nt = (long long)n_tri;
    int* w = (int*)ws;
    int *raw_off = w + pl.raw_off, *cnt = w + pl.cnt, *long_list = w + pl.long_list, *n_long = w + pl.n_long;
    int *tiles = w + pl.tiles, *raw = w + pl.raw;
    const bool pairs = nv > 0 && nt > 0;
    hipLaunchKernelGGL(adj_zero_kernel, dim3(nv > 0 ? blocks_for(nv) : 1), dim3(NTHR), 0, s, cnt, nv, n_long);
    if (pairs) hipLaunchKernelGGL(adj_count_kernel, dim3(blocks_for(nt)), dim3(NTHR), 0, s, triangles, nt, nv, cnt);
    exclusive_scan<false, SHORT_ROW>(cnt, nv, raw_off, tiles, nullptr, long_list, n_long, s);
    if (pairs)
        hipLaunchKernelGGL(adj_fill_kernel, dim3(blocks_for(nt)), dim3(NTHR), 0, s, triangles, nt, nv, cnt,
                           (const int*)raw_off, raw);
    if (nv > 0) {
        hipLaunchKernelGGL(adj_rows_kernel, dim3(blocks_for(nv)), dim3(NTHR), 0, s, (const int*)raw_off, raw, nv, cnt,
                           boundary);
        if (6 * nt > SHORT_ROW)
            hipLaunchKernelGGL(adj_long_rows_kernel, dim3(long_blocks(6 * nt, SHORT_ROW)), dim3(NTHR), 0, s,
                               (const int*)raw_off, raw, nv, cnt, boundary, (const int*)long_list, (const int*)n_long);
    }
    exclusive_scan<true, 0>(cnt, nv, offsets, tiles, (long long*)totals_dev, nullptr, nullptr, s);
    return launched("anerf_mesh_adjacency_count");
}

int anerf_mesh_adjacency_emit(int64_t n_vertices, void* ws, size_t ws_bytes, const int32_t* offsets,
                              int32_t* neighbors, int64_t max_neighbors, void* stream) {
    AdjPlan pl;
    if (!adj_plan(n_vertices, &pl) || max_neighbors < 0 || max_neighbors > MAXN)
        return failf(ANERF_EINVAL, "anerf_mesh_adjacency_emit: n_vertices %lld / max_neighbors %lld must be in "
                     "[0, 2^31)", (long long)n_vertices, (long long)max_neighbors);
    if (!offsets || !ws || (max_neighbors > 0 && !neighbors))
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_adjacency_emit: NULL offsets or workspace, or NULL "
                                                 "neighbors with a non-zero capacity");
    const int rc = check_workspace("anerf_mesh_adjacency_emit", ws, ws_bytes, pl.raw * sizeof(int), 4, ANERF_EINVAL,
                                   "anerf_mesh_adjacency_workspace", "at least ");
    if (rc != ANERF_OK) return rc;
    const int nv = (int)n_vertices;
    if (nv == 0 || max_neighbors == 0) return ANERF_OK;
    hipStream_t s = (hipStream_t)stream;
    const int* w = (const int*)ws;
    long long raw_cap = (long long)(ws_bytes / sizeof(int) - pl.raw);  // the raw rows the workspace can hold
    if (raw_cap > MAXN) raw_cap = MAXN;
    hipLaunchKernelGGL(adj_emit_kernel, dim3(blocks_for(nv)), dim3(NTHR), 0, s, w + pl.raw_off, w + pl.raw, nv, raw_cap,
                       offsets, neighbors, (long long)max_neighbors);
    if (raw_cap > SHORT_ROW)
        hipLaunchKernelGGL(adj_emit_long_kernel, dim3(long_blocks(raw_cap, SHORT_ROW)), dim3(NTHR), 0, s,
                           w + pl.raw_off, w + pl.raw, nv, raw_cap, w + pl.long_list, w + pl.n_long, offsets, neighbors,
                           (long long)max_neighbors);
    return launched("anerf_mesh_adjacency_emit");
}

int anerf_mesh_smooth(const float* positions, int64_t n_vertices, const int32_t* offsets, const int32_t* neighbors,
                      int64_t n_neighbors, const uint8_t* pinned, int32_t iterations, float lambda, float mu,
                      int32_t flags, float* out, float* scratch, void* stream) {
    if (n_vertices < 0 || n_vertices > MAXN || n_neighbors < 0 || n_neighbors > MAXN || iterations < 0 ||
        iterations > 0x3fffffff || (flags & ~ANERF_SMOOTH_TAUBIN))
        return failf(ANERF_EINVAL, "anerf_mesh_smooth: n_vertices %lld / n_neighbors %lld must be in [0, 2^31), "
                     "iterations %d in [0, 2^30), flags %d a combination of ANERF_SMOOTH_*", (long long)n_vertices,
                     (long long)n_neighbors, (int)iterations, (int)flags);
    const int steps = iterations * ((flags & ANERF_SMOOTH_TAUBIN) ? 2 : 1);
    if (n_vertices > 0 && (!positions || !out || !offsets || (steps > 1 && !scratch)))
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_smooth: NULL positions, out or offsets, or NULL scratch "
                                                 "with more than one step");
    if (n_neighbors > 0 && !neighbors)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_smooth: NULL neighbors with a non-zero extent");
    const size_t bytes = (size_t)n_vertices * 3 * sizeof(float);
    if (overlap(positions, out, bytes) || overlap(positions, scratch, bytes) || overlap(out, scratch, bytes))
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_smooth: positions, out and scratch must not overlap");
    if (n_vertices == 0) return ANERF_OK;
    hipStream_t s = (hipStream_t)stream;
    const int nv = (int)n_vertices;
    if (steps == 0) {
        const hipError_t e = hipMemcpyAsync(out, positions, bytes, hipMemcpyDeviceToDevice, s);
        return e == hipSuccess ? ANERF_OK : failf(ANERF_EHIP, "anerf_mesh_smooth: %s", hipGetErrorString(e));
    }
    // step i writes `out` when an even number of steps follows it: the last one always does
    const float* src = positions;
    for (int i = 0; i < steps; ++i) {
        float* dst = ((steps - 1 - i) & 1) ? scratch : out;
        const float w = ((flags & ANERF_SMOOTH_TAUBIN) && (i & 1)) ? mu : lambda;
        hipLaunchKernelGGL(smooth_step_kernel, dim3(blocks_for(nv)), dim3(NTHR), 0, s, src, nv, offsets, neighbors,
                           (int)n_neighbors, pinned, w, dst);
        src = dst;
    }
    return launched("anerf_mesh_smooth");
}

}  // extern "C"

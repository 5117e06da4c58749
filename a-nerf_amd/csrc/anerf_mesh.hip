// anerf_mesh.hip — connected components of an indexed triangle mesh and its stable compaction, on the device.
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
// pattern of anerf_iso.hip (256 threads x 4 consecutive items per workgroup).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/anerf.h"

int anerf_internal_fail(int code, const char* msg);  // anerf_render.hip: sets anerf_last_error()

namespace {

constexpr int NTHR = 256;           // threads per workgroup (4 waves of 64)
constexpr int TALLY_THR = 1024;     // threads per workgroup of the two tallying kernels
constexpr int TALLY_WAVES = TALLY_THR / 64;
constexpr int ITEMS = 4;            // consecutive items per thread (compaction)
constexpr int TILE = NTHR * ITEMS;  // items per workgroup (compaction)
constexpr long long MAXN = 0x7fffffffll;

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

__device__ __forceinline__ bool in_range(int a, int b, int c, int nv) {
    return (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv;
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

// Exclusive scan of one int per thread over the workgroup (NTHR threads); `total` is the workgroup's sum.
__device__ __forceinline__ int block_exclusive_scan(int x, int* lds, int& total) {
    const int t = threadIdx.x;
    __syncthreads();  // (lds may still be read by a previous call)
    lds[t] = x;
    __syncthreads();
    int acc = x;
    for (int d = 1; d < NTHR; d <<= 1) {
        const int y = t >= d ? lds[t - d] : 0;
        __syncthreads();
        acc += y;
        lds[t] = acc;
        __syncthreads();
    }
    total = lds[NTHR - 1];
    return acc - x;
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

// One workgroup: base[b] = sum of counts[< b] for the vertex and the triangle counts, tiles of NTHR with a carry.
__global__ __launch_bounds__(NTHR) void scan_kernel(const int* __restrict__ block_counts, long long* __restrict__ base,
                                                    int nblocks, long long* __restrict__ totals) {
    __shared__ int lds[NTHR];
    long long carry_v = 0, carry_t = 0;
    for (int start = 0; start < nblocks; start += NTHR) {
        const int b = start + threadIdx.x;
        const int cv = b < nblocks ? block_counts[b] : 0;
        const int ct = b < nblocks ? block_counts[nblocks + b] : 0;
        int tv, tt;  // (a tile sums at most NTHR * TILE: fits an int)
        const int ev = block_exclusive_scan(cv, lds, tv);
        const int et = block_exclusive_scan(ct, lds, tt);
        if (b < nblocks) {
            base[b] = carry_v + ev;
            base[nblocks + b] = carry_t + et;
        }
        carry_v += tv;
        carry_t += tt;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry_v;
        totals[1] = carry_t;
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

// Workspace of the compaction: long long base[2 nblocks] | int block_counts[2 nblocks]
struct Plan {
    int nblocks;
    size_t off_counts, bytes;
};

bool plan(int64_t nv, int64_t nt, Plan* pl) {
    if (nv < 0 || nt < 0 || nv > MAXN || nt > MAXN) return false;
    const long long n = nv > nt ? nv : nt;
    pl->nblocks = (int)((n + TILE - 1) / TILE);
    if (pl->nblocks < 1) pl->nblocks = 1;  // (empty lists still get their totals written)
    pl->off_counts = (size_t)pl->nblocks * 2 * sizeof(long long);
    pl->bytes = pl->off_counts + (size_t)pl->nblocks * 2 * sizeof(int);
    return true;
}

int check_compact(const char* who, const uint8_t* keep, int64_t nv, const int32_t* tri, int64_t nt, const void* ws,
                  size_t ws_bytes, Plan* pl) {
    char msg[256];
    if (!plan(nv, nt, pl)) {
        snprintf(msg, sizeof msg, "%s: n_vertices %lld / n_tri %lld must be in [0, 2^31)", who, (long long)nv,
                 (long long)nt);
        return anerf_internal_fail(ANERF_EINVAL, msg);
    }
    if ((nv > 0 && !keep) || (nt > 0 && !tri) || !ws) {
        snprintf(msg, sizeof msg, "%s: NULL keep, triangles or workspace", who);
        return anerf_internal_fail(ANERF_EINVAL, msg);
    }
    if ((uintptr_t)ws % 8) {
        snprintf(msg, sizeof msg, "%s: the workspace must be 8-byte aligned", who);
        return anerf_internal_fail(ANERF_EINVAL, msg);
    }
    if (ws_bytes < pl->bytes) {
        snprintf(msg, sizeof msg, "%s: workspace of %zu bytes, %zu needed (anerf_mesh_compact_workspace)", who,
                 ws_bytes, pl->bytes);
        return anerf_internal_fail(ANERF_EINVAL, msg);
    }
    return ANERF_OK;
}

int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return ANERF_OK;
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, hipGetErrorString(e));
    return anerf_internal_fail(ANERF_EHIP, msg);
}

int blocks_for(long long n, int threads = NTHR) { return (int)((n + threads - 1) / threads); }

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
    char msg[256];
    if (n_tri < 0 || n_vertices < 0 || n_tri > MAXN || n_vertices > MAXN) {
        snprintf(msg, sizeof msg, "anerf_mesh_components: n_tri %lld / n_vertices %lld must be in [0, 2^31)",
                 (long long)n_tri, (long long)n_vertices);
        return anerf_internal_fail(ANERF_EINVAL, msg);
    }
    if (!n_components) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_components: NULL n_components");
    if (n_tri > 0 && !triangles) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_components: NULL triangles");
    if (n_vertices > 0 && (!root || !tri_count || !vert_count || !ws))
        return anerf_internal_fail(ANERF_EINVAL,
                                   "anerf_mesh_components: NULL root, tri_count, vert_count or workspace");
    const size_t need = (size_t)n_vertices * sizeof(int);
    if (ws_bytes < need) {
        snprintf(msg, sizeof msg, "anerf_mesh_components: workspace of %zu bytes, %zu needed "
                 "(anerf_mesh_components_workspace)", ws_bytes, need);
        return anerf_internal_fail(ANERF_EINVAL, msg);
    }
    if ((uintptr_t)ws % 4)
        return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_components: the workspace must be 4-byte aligned");
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
    Plan pl;
    if (!plan(n_vertices, n_tri, &pl)) {
        anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_compact_workspace: counts must be in [0, 2^31)");
        return 0;
    }
    return pl.bytes;
}

int anerf_mesh_compact_count(const uint8_t* keep, int64_t n_vertices, const int32_t* triangles, int64_t n_tri, void* ws,
                             size_t ws_bytes, int64_t* totals_dev, void* stream) {
    Plan pl;
    const int rc = check_compact("anerf_mesh_compact_count", keep, n_vertices, triangles, n_tri, ws, ws_bytes, &pl);
    if (rc != ANERF_OK) return rc;
    if (!totals_dev) return anerf_internal_fail(ANERF_EINVAL, "anerf_mesh_compact_count: NULL totals");
    const Lists l = {keep, triangles, (long long)n_vertices, (long long)n_tri};
    long long* base = (long long*)ws;
    int* counts = (int*)((char*)ws + pl.off_counts);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(count_kernel, dim3(pl.nblocks), dim3(NTHR), 0, s, l, counts, pl.nblocks);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(NTHR), 0, s, counts, base, pl.nblocks, (long long*)totals_dev);
    return launched("anerf_mesh_compact_count");
}

int anerf_mesh_compact_emit(const uint8_t* keep, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                            const void* ws, size_t ws_bytes, int32_t* vertex_map, int32_t* kept, int64_t max_kept,
                            int32_t* triangles_out, int64_t max_triangles, void* stream) {
    Plan pl;
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

}  // extern "C"

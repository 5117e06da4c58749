// anerf_scan.hpp — what the mesh units (anerf_iso.hip, anerf_mesh.hip, anerf_raster.hip, anerf_simplify.hip) share.
//
// Count -> scan -> emit.  A pass that writes a variable number of outputs per item, in order and without atomics, runs
// in three steps over tiles of TILE = NTHR x ITEMS consecutive items, one workgroup each:
//   count   the unit's kernel: every thread counts its ITEMS items, block_exclusive_scan gives the tile's sum,
//           block_counts[tile] (two interleaved count arrays: vertices | triangles);
//   scan    scan_block_sums: one workgroup turns the tile sums into 64-bit bases and the two totals, which the host
//           reads to size the outputs;
//   emit    the unit's kernel: the same counts scanned within the tile, + base[tile] = each item's first output.
// The workspace of the pattern is ScanSpace (the iso-surface, the compaction, the simplification's outputs).
//
// Per-vertex rows (the adjacency of anerf_mesh.hip, the owner rows of anerf_simplify.hip): count per vertex ->
// exclusive_scan -> fill through take_slot -> sort or search each row, the long ones by one workgroup each:
//   exclusive_scan      out[0, n] of an int array in the same three steps on the same tiles (tile_sums_kernel,
//                       tile_bases_kernel, tile_scan_kernel); options: the 64-bit totals {sum, largest item}, the list
//                       of the rows above a threshold
//   take_slot           a row's next free slot from its count-down cursor
//   list_long_row, for_each_long_row, long_blocks   the list of the rows that get a workgroup, and the walk over it
//   bitonic_sort        the sorting network of one workgroup over a row (IntRow, KeyIndexRow), padded_log2
//
// Host helpers: failf, launched, check_workspace, at<T>, MAXN; on the device in_range.  Everything here sits in the
// unnamed namespace: each unit gets its own copy with internal linkage, no device symbol is exported, and a unit
// holds only the kernels it launches.  The host helpers report through anerf_last_error().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/anerf.h"

int anerf_internal_fail(int code, const char* msg);  // anerf_render.hip: sets anerf_last_error()

namespace {

constexpr int NTHR = 256;           // threads per workgroup (4 waves of 64)
constexpr int ITEMS = 4;            // consecutive items per thread
constexpr int TILE = NTHR * ITEMS;  // items per workgroup
constexpr long long MAXN = 0x7fffffffll;  // vertex and triangle counts lie in [0, 2^31)

inline int blocks_for(long long n, int threads = NTHR) { return (int)((n + threads - 1) / threads); }
inline int tiles_for(long long n) { return blocks_for(n, TILE); }

// A triangle whose three ids lie in [0, nv): the only kind a kernel takes an index from.
__device__ __forceinline__ bool in_range(int a, int b, int c, int nv) {
    return (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv;
}

// Exclusive scan of one int per thread over the workgroup (NTHR threads); `total` is the workgroup's sum.
// lds[NTHR]; safe to call back to back on the same lds.
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

// One workgroup: base[b] = sum of counts[< b] for the vertex and the triangle counts, tiles of NTHR with a carry.
__global__ __launch_bounds__(NTHR) void scan_kernel(const int* __restrict__ block_counts, long long* __restrict__ base,
                                                    int nblocks, long long* __restrict__ totals) {
    __shared__ int lds[NTHR];
    long long carry_v = 0, carry_t = 0;
    for (int start = 0; start < nblocks; start += NTHR) {
        const int b = start + threadIdx.x;
        const int cv = b < nblocks ? block_counts[b] : 0;
        const int ct = b < nblocks ? block_counts[nblocks + b] : 0;
        int tv, tt;  // (a block counts at most 5 per item, a cell's triangles: a tile sums at most NTHR * 5 * TILE)
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

// Workspace of the pattern: long long base[2 nblocks] | int block_counts[2 nblocks] | (the unit's own, from `bytes`)
struct ScanSpace {
    int nblocks;
    size_t off_counts, bytes;
    int* counts(void* ws) const { return (int*)((char*)ws + off_counts); }  // (base: ws itself)
};

inline ScanSpace scan_space(int nblocks) {
    ScanSpace sp;
    sp.nblocks = nblocks;
    sp.off_counts = (size_t)nblocks * 2 * sizeof(long long);
    sp.bytes = sp.off_counts + (size_t)nblocks * 2 * sizeof(int);
    return sp;
}

// The scan step, after the unit's count kernel on the same stream: bases into ws, the totals to totals_dev [2].
inline void scan_block_sums(const ScanSpace& sp, void* ws, int64_t* totals_dev, hipStream_t s) {
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(NTHR), 0, s, (const int*)sp.counts(ws), (long long*)ws, sp.nblocks,
                       (long long*)totals_dev);
}

// ------------------------------------------------------------------ per-vertex rows
constexpr int MAX_LONG_BLOCKS = 1024;  // workgroups of a long-row kernel (each strides over the list)

// The workgroups of a long-row kernel: no more rows than entries / (short_row + 1) can be long.
inline int long_blocks(long long entries, int short_row) {
    const long long rows = entries / (short_row + 1);
    return (int)(rows < 1 ? 1 : (rows > MAX_LONG_BLOCKS ? MAX_LONG_BLOCKS : rows));
}

// Row v goes to a workgroup.  The list has room for every vertex and each is listed at most once: the index stays
// below nv.  It fills in arrival order: each row is handled on its own, so the order does not show.
__device__ __forceinline__ void list_long_row(int* __restrict__ long_list, int* n_long, int v) {
    long_list[atomicAdd(n_long, 1)] = v;
}

// body(v) for the listed rows, by the whole workgroup, workgroup b taking entries b, b + gridDim.x, ...  The length is
// read from the device (no host read) and, like every entry, trusted only as far as [0, nv): a workspace that is not
// the count pass's cannot lead outside.  The bound and the skip are uniform over the workgroup, so body may use
// __syncthreads -- and must end on one if it leaves anything in LDS that the next row overwrites.
template <typename Body>
__device__ __forceinline__ void for_each_long_row(const int* __restrict__ long_list, const int* __restrict__ n_long,
                                                  int nv, Body body) {
    const int nl = min(*n_long, nv);
    for (int li = blockIdx.x; li < nl; li += gridDim.x) {
        const int v = long_list[li];
        if ((unsigned)v < (unsigned)nv) body(v);
    }
}

// cursor[x] starts as row x's count and counts down: every entry takes a slot of its own in its row, in arrival
// order.  A negative slot is none: the row is full (the cursor was not this fill's count).
__device__ __forceinline__ int take_slot(int* cursor, int x) { return atomicSub(cursor + x, 1) - 1; }

// Exclusive scan of in[0, n) into out[0, n], out[n] the sum (the callers keep it below 2^31), in the three steps of
// the pattern above: per-tile sums -> one workgroup scans them -> per-tile scan.  `tiles` is its workspace,
// scan_ints(n, TOTALS) ints.  TOTALS: totals[0] = the sum, totals[1] = the largest item (which rides along as a
// per-tile maximum), 64-bit, for the host.  LIST_ABOVE > 0: every row with more items than that is listed
// (list_long_row; n_long zeroed by the caller).
inline int scan_tiles(int n) { return n > 0 ? tiles_for(n) : 1; }  // (nothing to scan: out[0] is still written)
inline size_t scan_ints(int n, bool totals) { return (size_t)scan_tiles(n) * (totals ? 3 : 2); }

template <bool TOTALS>
__global__ __launch_bounds__(NTHR) void tile_sums_kernel(const int* __restrict__ in, int n, int* __restrict__ tile_sum,
                                                         int* __restrict__ tile_max) {
    __shared__ int lds[NTHR];
    __shared__ int mx;
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    int s = 0, m = 0;
    for (int it = 0; it < ITEMS; ++it) {
        if (first + it < n) {
            const int x = in[first + it];
            s += x;
            m = max(m, x);
        }
    }
    if (TOTALS && threadIdx.x == 0) mx = 0;
    int total;
    block_exclusive_scan(s, lds, total);  // (its barriers publish mx = 0)
    if (TOTALS) {
        atomicMax(&mx, m);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tile_sum[blockIdx.x] = total;
        if (TOTALS) tile_max[blockIdx.x] = mx;
    }
}

template <bool TOTALS>
__global__ __launch_bounds__(NTHR) void tile_bases_kernel(const int* __restrict__ tile_sum,
                                                          const int* __restrict__ tile_max, int nblocks,
                                                          int* __restrict__ base, int* __restrict__ last,
                                                          long long* __restrict__ totals) {
    __shared__ int lds[NTHR];
    __shared__ int mx;
    if (threadIdx.x == 0) mx = 0;
    __syncthreads();
    int carry = 0, m = 0;
    for (int start = 0; start < nblocks; start += NTHR) {
        const int b = start + threadIdx.x;
        const int c = b < nblocks ? tile_sum[b] : 0;
        if (TOTALS && b < nblocks) m = max(m, tile_max[b]);
        int total;
        const int e = block_exclusive_scan(c, lds, total);
        if (b < nblocks) base[b] = carry + e;
        carry += total;
    }
    if (TOTALS) {
        atomicMax(&mx, m);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *last = carry;
        if (TOTALS) {
            totals[0] = carry;
            totals[1] = mx;
        }
    }
}

template <int LIST_ABOVE>
__global__ __launch_bounds__(NTHR) void tile_scan_kernel(const int* __restrict__ in, int n, const int* __restrict__ base,
                                                         int* __restrict__ out, int* __restrict__ long_list,
                                                         int* n_long) {
    __shared__ int lds[NTHR];
    const long long first = (long long)blockIdx.x * TILE + threadIdx.x * ITEMS;
    int x[ITEMS], s = 0;
    for (int it = 0; it < ITEMS; ++it) {
        x[it] = first + it < n ? in[first + it] : 0;
        s += x[it];
    }
    int total;
    int e = base[blockIdx.x] + block_exclusive_scan(s, lds, total);
    for (int it = 0; it < ITEMS; ++it) {
        if (first + it >= n) break;
        out[first + it] = e;
        e += x[it];
        if (LIST_ABOVE > 0 && x[it] > LIST_ABOVE) list_long_row(long_list, n_long, (int)(first + it));
    }
}

template <bool TOTALS, int LIST_ABOVE>
void exclusive_scan(const int* in, int n, int* out, int* tiles, long long* totals, int* long_list, int* n_long,
                    hipStream_t s) {
    const int nb = scan_tiles(n);
    int *sum = tiles, *base = tiles + nb, *mx = tiles + 2 * (size_t)nb;  // (mx: with TOTALS only)
    hipLaunchKernelGGL(tile_sums_kernel<TOTALS>, dim3(nb), dim3(NTHR), 0, s, in, n, sum, mx);
    hipLaunchKernelGGL(tile_bases_kernel<TOTALS>, dim3(1), dim3(NTHR), 0, s, (const int*)sum, (const int*)mx, nb, base,
                       out + n, totals);
    if (n > 0)
        hipLaunchKernelGGL(tile_scan_kernel<LIST_ABOVE>, dim3(nb), dim3(NTHR), 0, s, in, n, (const int*)base, out,
                           long_list, n_long);
}

// Bitonic sorting network over a row of n entries by one workgroup, ascending, the row padded virtually to P = 2^lp
// >= n with +infinity: every compare-exchange (l, r), l < r, of this form of the network leaves the smaller at l, so
// an infinity at r >= n never moves and those pairs are skipped.  Stage s merges blocks of 2^s: pairs (i, block end
// - i) first, then halving strides.  Only __syncthreads between the stages (over global memory as well: one
// workgroup, one CU); the caller's barrier comes before (the row is complete) and after (it is sorted for every
// thread).  lp = padded_log2(n) <= 31; every loop is bounded by P.
// A Row is what the network compares and exchanges: load(i), store(i, entry), the entries ordered by <.
struct IntRow {  // ints, in LDS or in global memory
    int* a;
    __device__ int load(unsigned i) const { return a[i]; }
    __device__ void store(unsigned i, int x) const { a[i] = x; }
};

struct KeyIndex {
    unsigned long long key;
    int index;
    __device__ bool operator<(const KeyIndex& o) const { return key < o.key || (key == o.key && index < o.index); }
};

struct KeyIndexRow {  // (key, index) pairs in two arrays, ordered by key, then index
    unsigned long long* k;
    int* x;
    __device__ KeyIndex load(unsigned i) const { return {k[i], x[i]}; }
    __device__ void store(unsigned i, const KeyIndex& e) const { k[i] = e.key, x[i] = e.index; }
};

__device__ __forceinline__ int padded_log2(unsigned n) {
    int lp = 0;
    while (lp < 31 && (1u << lp) < n) ++lp;
    return lp;
}

template <typename Row>
__device__ __forceinline__ void compare_exchange(const Row& a, unsigned l, unsigned r, unsigned n) {
    if (r >= n) return;
    const auto x = a.load(l), y = a.load(r);
    if (y < x) {
        a.store(l, y);
        a.store(r, x);
    }
}

template <typename Row>
__device__ __forceinline__ void bitonic_sort(const Row& a, unsigned n, int lp) {
    const unsigned half = lp > 0 ? 1u << (lp - 1) : 0u;  // pairs per stage
    for (int s = 1; s <= lp; ++s) {
        const unsigned k = 1u << s, h = k >> 1;
        for (unsigned t = threadIdx.x; t < half; t += NTHR) {
            const unsigned first = (t >> (s - 1)) << s, in = t & (h - 1);
            compare_exchange(a, first + in, first + (k - 1 - in), n);
        }
        __syncthreads();
        for (int q = s - 2; q >= 0; --q) {
            const unsigned j = 1u << q;
            for (unsigned t = threadIdx.x; t < half; t += NTHR) {
                const unsigned l = ((t >> q) << (q + 1)) + (t & (j - 1));
                compare_exchange(a, l, l + j, n);
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ host helpers
// anerf_internal_fail with a formatted message (256 bytes, truncated); returns `code`.
__attribute__((format(printf, 2, 3))) inline int failf(int code, const char* fmt, ...) {
    char msg[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return anerf_internal_fail(code, msg);
}

// The end of an entry that launched kernels: ANERF_OK, or ANERF_EHIP with the launch error.
inline int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ANERF_OK : failf(ANERF_EHIP, "%s: %s", who, hipGetErrorString(e));
}

// An entry's workspace: there (unless it needs none), aligned to `align` bytes (4 or 8) and of at least `need` bytes,
// which `sizer`, the entry's _workspace function, returns.  A short one fails with `short_code`: ANERF_EWORKSPACE from
// the iso-surface entries, ANERF_EINVAL from the others.
inline int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need, int align, int short_code,
                           const char* sizer, const char* at_least = "") {
    if (!ws && need > 0) return failf(ANERF_EINVAL, "%s: NULL workspace", who);
    if ((uintptr_t)ws % (unsigned)align)
        return failf(ANERF_EINVAL, "%s: the workspace must be %d-byte aligned", who, align);
    if (ws_bytes < need)
        return failf(short_code, "%s: workspace of %zu bytes, %s%zu needed (%s)", who, ws_bytes, at_least, need, sizer);
    return ANERF_OK;
}

// The part of a workspace that starts `off` bytes in.
template <typename T>
T* at(const void* ws, size_t off) {
    return (T*)((char*)ws + off);
}

}  // namespace

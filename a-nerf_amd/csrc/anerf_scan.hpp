// anerf_scan.hpp — what the count -> scan -> emit passes of anerf_iso.hip and anerf_mesh.hip share.
//
// A pass that writes a variable number of outputs per item, in order and without atomics, runs in three steps over
// tiles of TILE = NTHR x ITEMS consecutive items, one workgroup each:
//   count   the unit's kernel: every thread counts its ITEMS items, block_exclusive_scan gives the tile's sum,
//           block_counts[tile] (two interleaved count arrays: vertices | triangles);
//   scan    scan_block_sums: one workgroup turns the tile sums into 64-bit bases and the two totals, which the host
//           reads to size the outputs;
//   emit    the unit's kernel: the same counts scanned within the tile, + base[tile] = each item's first output.
// The workspace of the pattern is ScanSpace.  Everything here sits in the unnamed namespace: each unit gets its own
// copy with internal linkage, no device symbol is exported.  The host helpers report through anerf_last_error().
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

inline int blocks_for(long long n, int threads = NTHR) { return (int)((n + threads - 1) / threads); }
inline int tiles_for(long long n) { return blocks_for(n, TILE); }

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

}  // namespace

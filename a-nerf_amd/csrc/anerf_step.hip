// anerf_step.hip — the tail of a training step: the image loss, the pose loss and the optimizer update.
//
// The reference's Trainer (core/trainer.py:319-483) runs these as dozens of small ATen launches with a host read per
// statistic and per parameter tensor; here each is a fixed, short launch sequence that never waits for the host:
//
//   anerf_train_loss            loss_kernel        per ray: both passes' (fine | coarse) terms, summed per block
//                               loss_final_kernel  one workgroup: the block sums in a fixed order, the 8 outputs
//   anerf_train_loss_backward   loss_bwd_kernel    per ray: g_rgb, g_acc of both passes, times the upstream scalar
//   anerf_pose_loss             pose_kernel        per (ray, joint): anchor, temporal and MPJPC terms, per block
//                               pose_final_kernel  one workgroup: the block sums, the 4 outputs
//   anerf_pose_loss_backward    pose_bwd_kernel    per (ray, joint): gradients to the rotations / bones and to kps
//   anerf_adam_step             adam_kernel        up to ADAM_MAX tensors per launch (the table travels by value), a
//                                                  workgroup per ADAM_CHUNK elements: torch.optim.Adam's update and the
//                                                  chunk's sum of squared gradients
//                               adam_norm_kernel   one workgroup: the chunk sums in a fixed order, total / avg norm
//
// These kernels are bound by launch latency, not by bandwidth or arithmetic (a training batch is a few thousand rays,
// the networks about a million parameters), so the sums and the loss arithmetic run in double: the results are the
// float64 values rounded once.  Every reduction has a fixed shape -- per thread in index order, an LDS tree per
// workgroup, one partial per workgroup in the workspace, a last workgroup that sums the partials in index order --
// so two runs give the same bits; there are no atomics.  The Adam update itself is fp32, in torch's operation order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/anerf.h"

int anerf_internal_fail(int code, const char* msg);  // anerf_render.hip: sets anerf_last_error()

namespace {

constexpr int NTHR = 256;  // threads per workgroup (4 waves of 64)
constexpr long long MAX_BLOCKS = 0x7fffffffll;
constexpr int HEAD = 16;   // doubles at the front of the loss workspaces: the final sums (read by the backward)

inline int launched(const char* fn) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return ANERF_OK;
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", fn, hipGetErrorString(e));
    return anerf_internal_fail(ANERF_EHIP, msg);
}

inline int fail(const char* fn, const char* what) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", fn, what);
    return anerf_internal_fail(ANERF_EINVAL, msg);
}

// The workgroup's sums of K values per thread: an LDS tree, the same pairs on every run.  lds [K * NTHR].
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* lds) {
    const int t = threadIdx.x;
    __syncthreads();  // (lds may still be read by a previous call)
    for (int k = 0; k < K; ++k) lds[k * NTHR + t] = v[k];
    __syncthreads();
    for (int s = NTHR / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < K; ++k) lds[k * NTHR + t] += lds[k * NTHR + t + s];
        __syncthreads();
    }
    for (int k = 0; k < K; ++k) v[k] = lds[k * NTHR];
}

// One workgroup: the sums over `nparts` partial rows of K doubles, thread t taking rows t, t + NTHR, ... in order.
template <int K>
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, long long nparts, double (&v)[K],
                                             double* lds) {
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (long long b = threadIdx.x; b < nparts; b += NTHR)
        for (int k = 0; k < K; ++k) v[k] += part[b * K + k];
    block_sum<K>(v, lds);
}

// ---------------------------------------------------------------------------------------------------------------------
// The image loss (Trainer._compute_nerf_loss, core/trainer.py:353-380)

struct LossArgs {
    const float *rgb, *acc, *rgb0, *acc0, *target, *bgs, *fgs;
    long long n;
    int kind, use_bg, reg;
    float beta, base_bg, coarse_weight, reg_coef;
};

constexpr int LK = 5;  // per pass: loss sum, squared-error sum, regulariser sum, regulariser count, acc sum

// loss and d loss / d (pred - target) of one element
__device__ __forceinline__ double elem_loss(int kind, double beta, double d, double& grad) {
    const double ad = fabs(d);
    if (kind == ANERF_LOSS_MSE) {
        grad = 2.0 * d;
        return d * d;
    }
    if (kind == ANERF_LOSS_L1 || beta <= 0.0) {  // (smooth_l1_loss with beta 0 is the L1 loss)
        grad = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
        return ad;
    }
    if (ad < beta) {
        grad = d / beta;
        return 0.5 * d * d / beta;
    }
    grad = d > 0.0 ? 1.0 : -1.0;
    return ad - 0.5 * beta;
}

// acc2bce's element and its derivative to the accumulated opacity (eps 1e-8)
__device__ __forceinline__ double bce(double x, double y, double& grad) {
    const double eps = 1e-8;
    grad = -(y / (x + eps) - (1.0 - y) / (1.0 - x + eps));
    return -(y * log(x + eps) + (1.0 - y) * log(1.0 - x + eps));
}

// One ray of one pass: its sums into s[LK] (when s) or its gradients (when g_rgb): scale_rgb on the loss term,
// scale_reg on the regulariser term.
__device__ __forceinline__ void loss_ray(const LossArgs& a, const float* __restrict__ rgb,
                                         const float* __restrict__ acc, long long i, double* s, float* g_rgb,
                                         float* g_acc, double scale_rgb, double scale_reg) {
    const double ac = acc[i];
    double ga = 0.0;
    for (int c = 0; c < 3; ++c) {
        double p = rgb[3 * i + c];
        double bg = 0.0;
        if (a.use_bg) {
            bg = a.bgs ? (double)a.bgs[3 * i + c] : (double)a.base_bg;
            p += (1.0 - ac) * bg;
        }
        const double d = p - (double)a.target[3 * i + c];
        double gr;
        const double l = elem_loss(a.kind, a.beta, d, gr);
        if (s) {
            s[0] += l;
            s[1] += d * d;
        } else {
            g_rgb[3 * i + c] = (float)(gr * scale_rgb);
            ga -= gr * scale_rgb * bg;
        }
    }
    if (a.reg == ANERF_REG_BCE) {
        const double y = a.fgs[i];
        if (y < 1.0) {  // (reduction 'off': the mean over y < 1)
            double gr;
            const double l = bce(ac, y, gr);
            if (s) {
                s[2] += l;
                s[3] += 1.0;
            } else {
                ga += gr * scale_reg;
            }
        }
    }
    if (s)
        s[4] += ac;
    else
        g_acc[i] = (float)ga;
}

__global__ __launch_bounds__(NTHR) void loss_kernel(LossArgs a, double* __restrict__ part) {
    __shared__ double lds[2 * LK * NTHR];
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    double s[2 * LK];
    for (int k = 0; k < 2 * LK; ++k) s[k] = 0.0;
    if (i < a.n) {
        loss_ray(a, a.rgb, a.acc, i, s, nullptr, nullptr, 0.0, 0.0);
        if (a.rgb0) loss_ray(a, a.rgb0, a.acc0, i, s + LK, nullptr, nullptr, 0.0, 0.0);
    }
    block_sum<2 * LK>(s, lds);
    if (threadIdx.x < 2 * LK) part[(long long)blockIdx.x * 2 * LK + threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(NTHR) void loss_final_kernel(LossArgs a, const double* __restrict__ part,
                                                          long long nparts, double* __restrict__ head,
                                                          float* __restrict__ out) {
    __shared__ double lds[2 * LK * NTHR];
    double s[2 * LK];
    sum_partials<2 * LK>(part, nparts, s, lds);
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 2 * LK; ++k) head[k] = s[k];
    const double n3 = 3.0 * (double)a.n, ln10 = log(10.0);
    const bool coarse = a.rgb0 != nullptr, reg = a.reg == ANERF_REG_BCE;
    const double rgb_loss = s[0] / n3;
    const double rgb_loss0 = coarse ? s[LK] / n3 * (double)a.coarse_weight : 0.0;
    // (no ray with fgs < 1: 0 / 0, a NaN, as torch's mean of an empty selection)
    const double reg_loss = reg ? s[2] / s[3] * (double)a.reg_coef : 0.0;
    const double reg_loss0 = reg && coarse ? s[LK + 2] / s[LK + 3] * (double)a.reg_coef : 0.0;
    out[0] = (float)rgb_loss;
    out[1] = (float)rgb_loss0;
    out[2] = (float)reg_loss;
    out[3] = (float)reg_loss0;
    out[4] = (float)(-10.0 * log(s[1] / n3) / ln10);
    out[5] = coarse ? (float)(-10.0 * log(s[LK + 1] / n3) / ln10) : 0.f;
    out[6] = (float)(s[4] / (double)a.n);
    out[7] = (float)(rgb_loss + reg_loss + rgb_loss0 + reg_loss0);  // (Trainer.compute_loss's order, :340-349)
}

__global__ __launch_bounds__(NTHR) void loss_bwd_kernel(LossArgs a, const double* __restrict__ head,
                                                        const float* __restrict__ upstream, float* __restrict__ g_rgb,
                                                        float* __restrict__ g_acc, float* __restrict__ g_rgb0,
                                                        float* __restrict__ g_acc0) {
    const long long i = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (i >= a.n) return;
    const double up = (double)upstream[0], n3 = 3.0 * (double)a.n;
    loss_ray(a, a.rgb, a.acc, i, nullptr, g_rgb, g_acc, up / n3, up * (double)a.reg_coef / head[3]);
    if (a.rgb0)
        loss_ray(a, a.rgb0, a.acc0, i, nullptr, g_rgb0, g_acc0, up * (double)a.coarse_weight / n3,
                 up * (double)a.reg_coef / head[LK + 3]);
}

int check_loss(const char* fn, const LossArgs& a) {
    if (!a.rgb || !a.acc || !a.target) return fail(fn, "rgb, acc and target must not be NULL");
    if ((a.rgb0 == nullptr) != (a.acc0 == nullptr)) return fail(fn, "rgb0 and acc0: both or neither");
    if (a.n < 1 || (a.n + NTHR - 1) / NTHR > MAX_BLOCKS) return fail(fn, "n must be in [1, 2^31 * 256)");
    if (a.kind != ANERF_LOSS_MSE && a.kind != ANERF_LOSS_L1 && a.kind != ANERF_LOSS_HUBER)
        return fail(fn, "unknown loss kind (ANERF_LOSS_MSE, _L1 or _HUBER)");
    if (a.kind == ANERF_LOSS_HUBER && !(a.beta >= 0.f)) return fail(fn, "the Huber beta must be >= 0");
    if (a.reg != ANERF_REG_NONE && a.reg != ANERF_REG_BCE) return fail(fn, "unknown regulariser (ANERF_REG_NONE or _BCE)");
    if (a.reg == ANERF_REG_BCE && !a.fgs) return fail(fn, "the BCE regulariser needs fgs");
    return ANERF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The pose loss (Trainer._compute_kp_loss, core/trainer.py:382-441)

struct PoseArgs {
    const float *cur, *anchor, *kps, *anchor_kps;
    const long long* kp_idx;
    const float *prev_cur, *next_cur, *prev_kps, *next_kps, *temp_val;  // all NULL without the temporal term
    long long n, n_poses;
    int nj, rot6d;
    float tol, coef, temp_coef, ext_scale;
};

constexpr int PK = 3;  // anchor-loss sum, temporal sum, per-joint change sum

// Component c of joint (i, j)'s rotation parameters in a per-ray tensor: the [:3, :2] block of a 3 x 3 rotation,
// row-major (--opt_rot6d), or an axis-angle bone.
__device__ __forceinline__ long long cur_at(const PoseArgs& a, long long ij, int c) {
    return a.rot6d ? ij * 9 + (c >> 1) * 3 + (c & 1) : ij * 3 + c;
}

// One (ray, joint): its sums into s[PK] (when s) or its gradients, scaled by the three factors.
__device__ __forceinline__ void pose_item(const PoseArgs& a, long long ij, double* s, float* g_cur, float* g_kps,
                                          double scale_kp, double scale_temp) {
    const long long i = ij / a.nj;
    const int j = (int)(ij - i * a.nj);
    const int nc = a.rot6d ? 6 : 3;
    const long long f = a.kp_idx[i];
    const bool ok = f >= 0 && f < a.n_poses;  // (an index outside the table reads nothing and poisons the sums)
    const bool temporal = a.prev_cur != nullptr;
    const double tv = temporal ? (double)a.temp_val[i] : 0.0;
    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nc; ++c) {
        const double b = a.cur[cur_at(a, ij, c)];
        if (j > 0) {  // (the root joint is excluded)
            const double diff = ok ? (double)a.anchor[(f * a.nj + j) * nc + c] - b : NAN;
            const double d = diff * diff;
            if (!(d <= (double)a.tol)) {  // (a NaN goes through, as torch's lerp of it)
                if (s) s[0] += d - (double)a.tol;
                g[c] -= 2.0 * diff * scale_kp;
            }
        }
        if (temporal) {
            const double v = (b - (double)a.prev_cur[cur_at(a, ij, c)]) - ((double)a.next_cur[cur_at(a, ij, c)] - b);
            if (s) s[1] += v * v * tv;
            g[c] += 4.0 * v * tv * scale_temp;
        }
    }
    if (g_cur) {
        if (a.rot6d) {
            for (int r = 0; r < 3; ++r) {
                g_cur[ij * 9 + r * 3 + 0] = (float)g[2 * r];
                g_cur[ij * 9 + r * 3 + 1] = (float)g[2 * r + 1];
                g_cur[ij * 9 + r * 3 + 2] = 0.f;
            }
        } else {
            for (int c = 0; c < 3; ++c) g_cur[ij * 3 + c] = (float)g[c];
        }
    }
    double dist2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double k = a.kps[ij * 3 + c];
        if (s) {
            const double e = ok ? (double)a.anchor_kps[(f * a.nj + j) * 3 + c] - k : NAN;
            dist2 += e * e;
        }
        double gk = 0.0;
        if (temporal) {
            const double u = (k - (double)a.prev_kps[ij * 3 + c]) - ((double)a.next_kps[ij * 3 + c] - k);
            if (s) s[1] += u * u * tv;
            gk = 4.0 * u * tv * scale_temp;
        }
        if (g_kps) g_kps[ij * 3 + c] = (float)gk;
    }
    if (s) s[2] += sqrt(dist2);
}

__global__ __launch_bounds__(NTHR) void pose_kernel(PoseArgs a, double* __restrict__ part) {
    __shared__ double lds[PK * NTHR];
    const long long ij = (long long)blockIdx.x * NTHR + threadIdx.x;
    double s[PK] = {0.0, 0.0, 0.0};
    if (ij < a.n * a.nj) pose_item(a, ij, s, nullptr, nullptr, 0.0, 0.0);
    block_sum<PK>(s, lds);
    if (threadIdx.x < PK) part[(long long)blockIdx.x * PK + threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(NTHR) void pose_final_kernel(PoseArgs a, const double* __restrict__ part,
                                                          long long nparts, float* __restrict__ out) {
    __shared__ double lds[PK * NTHR];
    double s[PK];
    sum_partials<PK>(part, nparts, s, lds);
    if (threadIdx.x != 0) return;
    const double items = (double)a.n * (double)a.nj;
    const double kp_loss = s[0] / ((double)a.n * (double)(a.nj - 1)) * (double)a.coef;
    const double temp_loss = a.prev_cur ? s[1] / items * (double)a.temp_coef : 0.0;
    out[0] = (float)kp_loss;
    out[1] = (float)temp_loss;
    out[2] = (float)(s[2] / items / (double)a.ext_scale);
    out[3] = (float)(kp_loss + temp_loss);
}

__global__ __launch_bounds__(NTHR) void pose_bwd_kernel(PoseArgs a, const float* __restrict__ upstream,
                                                        float* __restrict__ g_cur, float* __restrict__ g_kps) {
    const long long ij = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (ij >= a.n * a.nj) return;
    const double up = (double)upstream[0], items = (double)a.n * (double)a.nj;
    pose_item(a, ij, nullptr, g_cur, g_kps, up * (double)a.coef / ((double)a.n * (double)(a.nj - 1)),
              up * (double)a.temp_coef / items);
}

int check_pose(const char* fn, const PoseArgs& a) {
    if (!a.cur || !a.anchor || !a.kps || !a.anchor_kps || !a.kp_idx)
        return fail(fn, "cur, anchor, kp_idx, kps and anchor_kps must not be NULL");
    const int nt = (a.prev_cur != nullptr) + (a.next_cur != nullptr) + (a.prev_kps != nullptr) +
                   (a.next_kps != nullptr) + (a.temp_val != nullptr);
    if (nt != 0 && nt != 5) return fail(fn, "the temporal term takes prev / next cur and kps and temp_val: all or none");
    if (a.n < 1 || a.n_poses < 1) return fail(fn, "n and n_poses must be >= 1");
    if (a.nj < 2 || a.nj > 4096) return fail(fn, "n_joints must be in [2, 4096] (the root joint carries no anchor loss)");
    // (n first: the product of a huge n would overflow before it could be refused)
    if (a.n > (1ll << 40) || (a.n * a.nj + NTHR - 1) / NTHR > MAX_BLOCKS) return fail(fn, "n * n_joints too large");
    return ANERF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Adam over a table of tensors (torch.optim.Adam's update, torch/optim/adam.py) with the gradients' sum of squares

constexpr int ADAM_MAX = 64;       // tensors per launch: the table is a kernel argument (2.8 KB of the 4 KB)
constexpr int ADAM_CHUNK = 2048;   // elements per workgroup: 2 float4 per thread

struct AdamTable {
    float* p[ADAM_MAX];
    const float* g[ADAM_MAX];
    float* m[ADAM_MAX];
    float* v[ADAM_MAX];
    long long numel[ADAM_MAX];
    int start[ADAM_MAX + 1];  // first workgroup of tensor k (start[count] = the launch's workgroups)
    int count;
};

struct AdamScalars {
    float b1w, beta2, b2w, bc2_sqrt, eps, neg_step_size, wd;
};

// torch's element update, operation by operation (exp_avg.lerp_, exp_avg_sq.mul_().addcmul_(), addcdiv_)
__device__ __forceinline__ void adam_elem(const AdamScalars& s, float& p, float g, float& m, float& v, double& sq) {
    sq += (double)g * (double)g;
    if (s.wd != 0.f) g = g + s.wd * p;
    m = m + s.b1w * (g - m);
    v = v * s.beta2 + (s.b2w * g) * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + s.neg_step_size * (m / denom);
}

__global__ __launch_bounds__(NTHR) void adam_kernel(AdamTable t, AdamScalars s, double* __restrict__ part) {
    __shared__ double lds[NTHR];
    int lo = 0, hi = t.count;  // the tensor of this workgroup: the last k with start[k] <= blockIdx.x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    float* __restrict__ p = t.p[lo];
    const float* __restrict__ g = t.g[lo];
    float* __restrict__ m = t.m[lo];
    float* __restrict__ v = t.v[lo];
    const long long numel = t.numel[lo];
    const long long first = (long long)((int)blockIdx.x - t.start[lo]) * ADAM_CHUNK;
    // a gradient that is a view (one layer's rows of a stacked weight gradient) is only 4-byte aligned
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    double sq[1] = {0.0};
    for (int it = 0; it < ADAM_CHUNK / (4 * NTHR); ++it) {
        const long long e = first + ((long long)it * NTHR + threadIdx.x) * 4;
        if (e >= numel) continue;
        if (vec && e + 4 <= numel) {
            float4 pp = *reinterpret_cast<const float4*>(p + e);
            const float4 gg = *reinterpret_cast<const float4*>(g + e);
            float4 mm = *reinterpret_cast<const float4*>(m + e);
            float4 vv = *reinterpret_cast<const float4*>(v + e);
            adam_elem(s, pp.x, gg.x, mm.x, vv.x, sq[0]);
            adam_elem(s, pp.y, gg.y, mm.y, vv.y, sq[0]);
            adam_elem(s, pp.z, gg.z, mm.z, vv.z, sq[0]);
            adam_elem(s, pp.w, gg.w, mm.w, vv.w, sq[0]);
            *reinterpret_cast<float4*>(p + e) = pp;
            *reinterpret_cast<float4*>(m + e) = mm;
            *reinterpret_cast<float4*>(v + e) = vv;
        } else {
            const long long end = e + 4 < numel ? e + 4 : numel;
            for (long long q = e; q < end; ++q) {
                float pp = p[q], mm = m[q], vv = v[q];
                adam_elem(s, pp, g[q], mm, vv, sq[0]);
                p[q] = pp;
                m[q] = mm;
                v[q] = vv;
            }
        }
    }
    block_sum<1>(sq, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = sq[0];
}

__global__ __launch_bounds__(NTHR) void adam_norm_kernel(const double* __restrict__ part, long long nparts,
                                                         int tensors, float* __restrict__ norms) {
    __shared__ double lds[NTHR];
    double s[1];
    sum_partials<1>(part, nparts, s, lds);
    if (threadIdx.x != 0) return;
    norms[0] = (float)sqrt(s[0]);                     // get_gradnorm's total_norm (core/trainer.py:191-203)
    norms[1] = (float)sqrt(s[0] / (double)tensors);   // and avg_norm
}

inline long long adam_blocks(int64_t numel) { return (numel + ADAM_CHUNK - 1) / ADAM_CHUNK; }

}  // namespace

extern "C" {

size_t anerf_train_loss_workspace(int64_t n) {
    if (n < 1 || (n + NTHR - 1) / NTHR > MAX_BLOCKS) {
        fail("anerf_train_loss_workspace", "n must be in [1, 2^31 * 256)");
        return 0;
    }
    return sizeof(double) * (HEAD + (size_t)((n + NTHR - 1) / NTHR) * 2 * LK);
}

int anerf_train_loss(const float* rgb, const float* acc, const float* rgb0, const float* acc0, const float* target,
                     const float* bgs, float base_bg, const float* fgs, int64_t n, int32_t loss_kind, float beta,
                     int32_t use_background, float coarse_weight, int32_t reg_kind, float reg_coef, float* out,
                     void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "anerf_train_loss";
    const LossArgs a{rgb, acc, rgb0, acc0, target, bgs, fgs, n, loss_kind, use_background != 0, reg_kind,
                     beta, base_bg, coarse_weight, reg_coef};
    if (const int rc = check_loss(fn, a)) return rc;
    if (!out || !workspace) return fail(fn, "out and workspace must not be NULL");
    if (((uintptr_t)workspace & 7) != 0) return fail(fn, "the workspace must be 8-byte aligned");
    if (workspace_bytes < anerf_train_loss_workspace(n))
        return anerf_internal_fail(ANERF_EWORKSPACE, "anerf_train_loss: workspace too small");
    const long long blocks = (n + NTHR - 1) / NTHR;
    double* head = (double*)workspace;
    double* part = head + HEAD;
    hipLaunchKernelGGL(loss_kernel, dim3((unsigned)blocks), dim3(NTHR), 0, (hipStream_t)stream, a, part);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(NTHR), 0, (hipStream_t)stream, a, part, blocks, head, out);
    return launched(fn);
}

int anerf_train_loss_backward(const float* rgb, const float* acc, const float* rgb0, const float* acc0,
                              const float* target, const float* bgs, float base_bg, const float* fgs, int64_t n,
                              int32_t loss_kind, float beta, int32_t use_background, float coarse_weight,
                              int32_t reg_kind, float reg_coef, const void* workspace, size_t workspace_bytes,
                              const float* upstream, float* g_rgb, float* g_acc, float* g_rgb0, float* g_acc0,
                              void* stream) {
    const char* fn = "anerf_train_loss_backward";
    const LossArgs a{rgb, acc, rgb0, acc0, target, bgs, fgs, n, loss_kind, use_background != 0, reg_kind,
                     beta, base_bg, coarse_weight, reg_coef};
    if (const int rc = check_loss(fn, a)) return rc;
    if (!workspace || !upstream || !g_rgb || !g_acc) return fail(fn, "workspace, upstream, g_rgb and g_acc must not be NULL");
    if (rgb0 && (!g_rgb0 || !g_acc0)) return fail(fn, "the coarse pair needs g_rgb0 and g_acc0");
    if (((uintptr_t)workspace & 7) != 0) return fail(fn, "the workspace must be 8-byte aligned");
    if (workspace_bytes < anerf_train_loss_workspace(n))
        return anerf_internal_fail(ANERF_EWORKSPACE, "anerf_train_loss_backward: workspace too small");
    const long long blocks = (n + NTHR - 1) / NTHR;
    hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)blocks), dim3(NTHR), 0, (hipStream_t)stream, a,
                       (const double*)workspace, upstream, g_rgb, g_acc, g_rgb0, g_acc0);
    return launched(fn);
}

size_t anerf_pose_loss_workspace(int64_t n, int32_t n_joints) {
    if (n < 1 || n > (1ll << 40) || n_joints < 2 || n_joints > 4096 || (n * n_joints + NTHR - 1) / NTHR > MAX_BLOCKS) {
        fail("anerf_pose_loss_workspace", "n >= 1, n_joints in [2, 4096], n * n_joints < 2^31 * 256");
        return 0;
    }
    return sizeof(double) * (size_t)((n * n_joints + NTHR - 1) / NTHR) * PK;
}

int anerf_pose_loss(const float* cur, int32_t rot6d, const float* anchor, const int64_t* kp_idx, int64_t n,
                    int32_t n_joints, int64_t n_poses, const float* kps, const float* anchor_kps,
                    const float* prev_cur, const float* next_cur, const float* prev_kps, const float* next_kps,
                    const float* temp_val, float tol, float coef, float temp_coef, float ext_scale, float* out,
                    void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "anerf_pose_loss";
    const PoseArgs a{cur, anchor, kps, anchor_kps, (const long long*)kp_idx, prev_cur, next_cur, prev_kps, next_kps,
                     temp_val, n, n_poses, n_joints, rot6d != 0, tol, coef, temp_coef, ext_scale};
    if (const int rc = check_pose(fn, a)) return rc;
    if (!out || !workspace) return fail(fn, "out and workspace must not be NULL");
    if (!(ext_scale > 0.f)) return fail(fn, "ext_scale must be > 0");
    if (((uintptr_t)workspace & 7) != 0) return fail(fn, "the workspace must be 8-byte aligned");
    if (workspace_bytes < anerf_pose_loss_workspace(n, n_joints))
        return anerf_internal_fail(ANERF_EWORKSPACE, "anerf_pose_loss: workspace too small");
    const long long blocks = (n * n_joints + NTHR - 1) / NTHR;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(pose_kernel, dim3((unsigned)blocks), dim3(NTHR), 0, (hipStream_t)stream, a, part);
    hipLaunchKernelGGL(pose_final_kernel, dim3(1), dim3(NTHR), 0, (hipStream_t)stream, a, part, blocks, out);
    return launched(fn);
}

int anerf_pose_loss_backward(const float* cur, int32_t rot6d, const float* anchor, const int64_t* kp_idx, int64_t n,
                             int32_t n_joints, int64_t n_poses, const float* kps, const float* prev_cur,
                             const float* next_cur, const float* prev_kps, const float* next_kps,
                             const float* temp_val, float tol, float coef, float temp_coef, const float* upstream,
                             float* g_cur, float* g_kps, void* stream) {
    const char* fn = "anerf_pose_loss_backward";
    // (the per-joint change has no gradient: the anchor keypoints are not read; kps stands in for the check)
    const PoseArgs a{cur, anchor, kps, kps, (const long long*)kp_idx, prev_cur, next_cur, prev_kps, next_kps,
                     temp_val, n, n_poses, n_joints, rot6d != 0, tol, coef, temp_coef, 1.f};
    if (const int rc = check_pose(fn, a)) return rc;
    if (!upstream || !g_cur) return fail(fn, "upstream and g_cur must not be NULL");
    if (prev_cur && !g_kps) return fail(fn, "the temporal term needs g_kps");
    const long long blocks = (n * n_joints + NTHR - 1) / NTHR;
    hipLaunchKernelGGL(pose_bwd_kernel, dim3((unsigned)blocks), dim3(NTHR), 0, (hipStream_t)stream, a, upstream,
                       g_cur, g_kps);
    return launched(fn);
}

size_t anerf_adam_step_workspace(const int64_t* numel, int32_t count) {
    const char* fn = "anerf_adam_step_workspace";
    if (!numel || count < 1) {
        fail(fn, "numel must not be NULL, count >= 1");
        return 0;
    }
    long long blocks = 0;
    for (int k = 0; k < count; ++k) {
        if (numel[k] < 1 || adam_blocks(numel[k]) > MAX_BLOCKS || (blocks += adam_blocks(numel[k])) > MAX_BLOCKS) {
            fail(fn, "every numel must be >= 1 and the table below 2^31 chunks of 2048 elements");
            return 0;
        }
    }
    return sizeof(double) * (size_t)blocks;
}

int anerf_adam_step(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                    const int64_t* numel, int32_t count, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int64_t step, int64_t chunk_base, int32_t norm_tensors, float* norms,
                    void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "anerf_adam_step";
    if (!params || !grads || !exp_avg || !exp_avg_sq || !numel || !workspace)
        return fail(fn, "params, grads, exp_avg, exp_avg_sq, numel and workspace must not be NULL");
    if (count < 1) return fail(fn, "count must be >= 1");
    if (step < 1) return fail(fn, "step must be >= 1 (the number of this update)");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) ||
        !(weight_decay >= 0.0))
        return fail(fn, "lr, eps, weight_decay >= 0 and betas in [0, 1)");
    if (chunk_base < 0 || chunk_base > MAX_BLOCKS) return fail(fn, "chunk_base must be >= 0");
    if (norms && norm_tensors < 1) return fail(fn, "norm_tensors must be >= 1 with norms");
    if (((uintptr_t)workspace & 7) != 0) return fail(fn, "the workspace must be 8-byte aligned");
    long long blocks = 0;
    for (int k = 0; k < count; ++k) {
        if (!params[k] || !grads[k] || !exp_avg[k] || !exp_avg_sq[k]) return fail(fn, "NULL tensor in the table");
        if ((((uintptr_t)params[k] | (uintptr_t)grads[k] | (uintptr_t)exp_avg[k] | (uintptr_t)exp_avg_sq[k]) & 3) != 0)
            return fail(fn, "tensors must be 4-byte aligned");
        if (numel[k] < 1 || adam_blocks(numel[k]) > MAX_BLOCKS || (blocks += adam_blocks(numel[k])) > MAX_BLOCKS)
            return fail(fn, "every numel must be >= 1 and the table below 2^31 chunks of 2048 elements");
    }
    if (chunk_base + blocks > MAX_BLOCKS) return fail(fn, "too many chunks");
    if (workspace_bytes < sizeof(double) * (size_t)(chunk_base + blocks))
        return anerf_internal_fail(ANERF_EWORKSPACE, "anerf_adam_step: workspace too small");
    // the scalars of torch's _single_tensor_adam / _multi_tensor_adam, in double as Python computes them
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    const AdamScalars s{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)std::sqrt(bc2), (float)eps,
                        (float)(-(lr / bc1)), (float)weight_decay};
    double* part = (double*)workspace + chunk_base;
    for (int k0 = 0; k0 < count; k0 += ADAM_MAX) {  // the table travels by value, ADAM_MAX tensors at a time
        AdamTable t;
        t.count = count - k0 < ADAM_MAX ? count - k0 : ADAM_MAX;
        int b = 0;
        for (int k = 0; k < ADAM_MAX; ++k) {
            const int src = k < t.count ? k0 + k : k0;  // (unused slots repeat the first: never selected)
            t.p[k] = (float*)params[src];
            t.g[k] = (const float*)grads[src];
            t.m[k] = (float*)exp_avg[src];
            t.v[k] = (float*)exp_avg_sq[src];
            t.numel[k] = numel[src];
            t.start[k] = b;
            if (k < t.count) b += (int)adam_blocks(numel[src]);
        }
        t.start[ADAM_MAX] = b;
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)b), dim3(NTHR), 0, (hipStream_t)stream, t, s, part);
        part += b;
    }
    if (norms)
        hipLaunchKernelGGL(adam_norm_kernel, dim3(1), dim3(NTHR), 0, (hipStream_t)stream,
                           (const double*)workspace, (long long)(chunk_base + blocks), norm_tensors, norms);
    return launched(fn);
}

}  // extern "C"

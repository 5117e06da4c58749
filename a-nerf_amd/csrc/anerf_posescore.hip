// anerf_posescore.hip — scoring of refined skeleton poses on the device: MPJPE, PA-MPJPE, PCK counts.
//
// The reference scores on the host (core/utils/evaluation_helpers.py:387-612): per frame the pose is downloaded and a
// NumPy port of MATLAB's `procrustes` runs one LAPACK SVD inside a Python loop, in float32.  Here the joints are scored
// where PoseOptLayer left them, in double, all frames in one call:
//
//   anerf_pose_scores   pose_score_kernel   a wavefront per frame, lane l holding joints l and l + 64: three butterflies
//                                           (10, 14 and 2 sums), the 3 x 3 SVD by one-sided Jacobi on every lane, the
//                                           frame's record of 25 doubles, its error planes and its aligned joints
//                       pose_total_kernel   twice: a workgroup per 32 frames -> its slot (frame counts, score sums,
//                                           per-joint sums and counts, threshold counts), then one last workgroup over
//                                           the slots in slot order -> totals [520]
//
// Everything after the widening of the inputs is double: d = 1 - trace^2 and Z - gt are cancellations that float32
// resolves to 4e-7 of the pose's extent at best (tests/golden/pose_scores.npz records the reference's own gap).  Every
// reduction has a fixed shape -- per lane in joint order, one __shfl_xor butterfly per wave, a serial loop per output
// element over a slot's frames and over the slots -- so two runs give the same bits and a frame's record does not
// depend on the other frames of the launch; there are no atomics and no data-dependent loops.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/anerf.h"

int anerf_internal_fail(int code, const char* msg);  // anerf_render.hip: sets anerf_last_error()

namespace {

constexpr int NTHR = 256;                 // threads per workgroup (4 waves of 64: 4 frames)
constexpr int WAVES = NTHR / 64;
constexpr int MAXJ = ANERF_POSE_MAX_JOINTS;
constexpr int PASSES = MAXJ / 64;         // joints per lane
constexpr int MAXT = ANERF_POSE_MAX_THRESHOLDS;
constexpr int NCOL = ANERF_POSE_FRAME_COLS;
constexpr int NTOT = ANERF_POSE_TOTALS;   // 8 + 3 x 128 + 2 x 64 words of 8 bytes
constexpr int SLOT_FRAMES = 32;           // frames per slot of the total kernel (2 x 32 x 128 doubles = 64 KB of LDS)
constexpr int SWEEPS = 10;                // Jacobi sweeps (3 rotations each); 3 x 3 in double converges in 5 or 6
constexpr double RANK_TOL = 1e-12;        // sigma_i <= RANK_TOL sigma_0: completed by cross products
constexpr double ZERO_SS = 1e-26;         // centred sum of squares <= ZERO_SS x the uncentred one: a zero norm
constexpr int T_JOINT = 8, T_COUNT = T_JOINT + 3 * MAXJ;
static_assert(T_COUNT + 2 * MAXT == NTOT, "layout of the totals");
static_assert(NCOL == 25, "layout of a frame's record");

struct ScoreArgs {
    const void* pred;
    const void* gt;
    const unsigned char* valid;
    double* frames;
    double* err;
    double* pa_err;
    float* aligned;
    int F, J, root, pred_f64, gt_f64, scaling, reflection;  // reflection: 0 best, 1 false, 2 true
    double pred_scale, gt_scale;
    unsigned long long sel[PASSES];  // bit l of sel[k]: joint l + 64 k is selected
};

struct TotalArgs {
    const double* frames;
    const double* err;
    const double* pa_err;
    const unsigned char* valid;
    double* slots;
    double* totals;
    int F, J, nt, nslots;
    unsigned long long sel[PASSES];
    double thr[MAXT];
};

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

// The wave's sums of N values per lane: one butterfly, after which every lane holds the same bits (a + b == b + a).
template <int N>
__device__ __forceinline__ void wave_sum(double (&v)[N]) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += __shfl_xor(v[k], m);
    }
}

__device__ __forceinline__ double load_scaled(const void* base, int f64, size_t at, double scale) {
    return (f64 ? ((const double*)base)[at] : (double)((const float*)base)[at]) * scale;
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// One rotation of the one-sided Jacobi: columns P and Q of G (and of V) are rotated until they are orthogonal.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&G)[3][3], double (&V)[3][3]) {
    const double alpha = G[0][P] * G[0][P] + G[1][P] * G[1][P] + G[2][P] * G[2][P];
    const double beta = G[0][Q] * G[0][Q] + G[1][Q] * G[1][Q] + G[2][Q] * G[2][Q];
    const double gamma = G[0][P] * G[0][Q] + G[1][P] * G[1][Q] + G[2][P] * G[2][Q];
    const bool on = fabs(gamma) > 0.0;
    const double zeta = (beta - alpha) / (2.0 * (on ? gamma : 1.0));
    double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));  // (zeta = inf: t = 0)
    t = on ? t : 0.0;
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double gp = G[r][P], gq = G[r][Q], vp = V[r][P], vq = V[r][Q];
        G[r][P] = c * gp - s * gq;
        G[r][Q] = s * gp + c * gq;
        V[r][P] = c * vp - s * vq;
        V[r][Q] = s * vp + c * vq;
    }
}

// Columns P < Q of G and V, and their squared norms, into descending order.
template <int P, int Q>
__device__ __forceinline__ void order_columns(double (&G)[3][3], double (&V)[3][3], double (&n2)[3]) {
    const bool sw = n2[P] < n2[Q];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double gp = G[r][P], gq = G[r][Q], vp = V[r][P], vq = V[r][Q];
        G[r][P] = sw ? gq : gp;
        G[r][Q] = sw ? gp : gq;
        V[r][P] = sw ? vq : vp;
        V[r][Q] = sw ? vp : vq;
    }
    const double a = n2[P], b = n2[Q];
    n2[P] = sw ? b : a;
    n2[Q] = sw ? a : b;
}

__device__ __forceinline__ double det3(const double (&M)[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// A = U diag(s) V^T with s descending, U and V orthogonal, a fixed number of operations: SWEEPS cyclic sweeps of the
// one-sided Jacobi on A's columns (which keeps the small singular values to their own relative accuracy), the columns
// ordered, U = G / s.  Where A has rank 2 or 1 the missing columns of U are completed by cross products to
// det U = det V; rank 0 gives U = V.
__device__ __forceinline__ void svd3(const double (&A)[3][3], double (&U)[3][3], double (&s)[3], double (&V)[3][3]) {
    double G[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            G[r][c] = A[r][c];
            V[r][c] = r == c ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {  // (a loop, not unrolled: the same trip count on every lane)
        jacobi_rotate<0, 1>(G, V);
        jacobi_rotate<0, 2>(G, V);
        jacobi_rotate<1, 2>(G, V);
    }
    double n2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) n2[c] = G[0][c] * G[0][c] + G[1][c] * G[1][c] + G[2][c] * G[2][c];
    order_columns<0, 1>(G, V, n2);
    order_columns<0, 2>(G, V, n2);
    order_columns<1, 2>(G, V, n2);
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = sqrt(n2[c]);
    const bool has0 = s[0] > 0.0;
    const bool has1 = has0 && s[1] > RANK_TOL * s[0];
    const bool has2 = has1 && s[2] > RANK_TOL * s[0];
    const double dv = det3(V) < 0.0 ? -1.0 : 1.0;
    double u0[3], u1[3], u2[3];
    const double i0 = 1.0 / (has0 ? s[0] : 1.0), i1 = 1.0 / (has1 ? s[1] : 1.0), i2 = 1.0 / (has2 ? s[2] : 1.0);
#pragma unroll
    for (int r = 0; r < 3; ++r) u0[r] = G[r][0] * i0;
    // a unit vector orthogonal to u0: the axis of u0's smallest component, less its part along u0
    const double a0 = fabs(u0[0]), a1 = fabs(u0[1]), a2 = fabs(u0[2]);
    const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    const double uk = k == 0 ? u0[0] : (k == 1 ? u0[1] : u0[2]);
    double w[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = (r == k ? 1.0 : 0.0) - uk * u0[r];
    const double wn = 1.0 / norm3(w[0], w[1], w[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] = has1 ? G[r][1] * i1 : w[r] * wn;
    const double x[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
    const double xn = 1.0 / norm3(x[0], x[1], x[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u2[r] = has2 ? G[r][2] * i2 : dv * x[r] * xn;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        U[r][0] = has0 ? u0[r] : V[r][0];
        U[r][1] = has0 ? u1[r] : V[r][1];
        U[r][2] = has0 ? u2[r] : V[r][2];
    }
}

// One frame per wavefront.  Lane l holds joints l and l + 64 (J <= 128); unselected or invalid joints add zeros.
__global__ __launch_bounds__(NTHR) void pose_score_kernel(ScoreArgs a) {
    const int lane = threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (f >= a.F) return;  // (the whole wave; the kernel has no barrier)
    const size_t fj = (size_t)f * (size_t)a.J;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    double p[PASSES][3], g[PASSES][3];
    bool on[PASSES], in[PASSES];
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        const int j = lane + 64 * k;
        in[k] = j < a.J;
        on[k] = in[k] && ((a.sel[k] >> lane) & 1ull) != 0 && (a.valid ? a.valid[fj + (in[k] ? j : 0)] != 0 : true);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[k][c] = in[k] ? load_scaled(a.pred, a.pred_f64, (fj + j) * 3 + c, a.pred_scale) : 0.0;
            g[k][c] = in[k] ? load_scaled(a.gt, a.gt_f64, (fj + j) * 3 + c, a.gt_scale) : 0.0;
        }
    }
    // the root joint (root < 0: none, the vectors are taken as they are)
    double pr[3] = {0.0, 0.0, 0.0}, gr[3] = {0.0, 0.0, 0.0};
    bool root_ok = true;
    if (a.root >= 0) {
        root_ok = a.valid ? a.valid[fj + a.root] != 0 : true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            pr[c] = load_scaled(a.pred, a.pred_f64, (fj + a.root) * 3 + c, a.pred_scale);
            gr[c] = load_scaled(a.gt, a.gt_f64, (fj + a.root) * 3 + c, a.gt_scale);
        }
    }

    // first butterfly: n, the centroids' sums, the error, the uncentred sums of squares
    double e[PASSES];
    double s1[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) s1[i] = 0.0;
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        e[k] = norm3(p[k][0] - g[k][0], p[k][1] - g[k][1], p[k][2] - g[k][2]);
        if (on[k]) {
            s1[0] += 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s1[1 + c] += p[k][c];
                s1[4 + c] += g[k][c];
            }
            s1[7] += e[k];
            s1[8] += p[k][0] * p[k][0] + p[k][1] * p[k][1] + p[k][2] * p[k][2];
            s1[9] += g[k][0] * g[k][0] + g[k][1] * g[k][1] + g[k][2] * g[k][2];
        }
    }
    wave_sum(s1);
    const double n = s1[0];
    double mp[3], mg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mp[c] = s1[1 + c] / n;
        mg[c] = s1[4 + c] / n;
    }

    // second butterfly: the centred sums of squares, A = X0^T Y0 (X = gt, Y = pred), the root-centred sums
    double s2[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) s2[i] = 0.0;
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        if (on[k]) {
            double y0[3], x0[3], yr[3], xr[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                y0[c] = p[k][c] - mp[c];
                x0[c] = g[k][c] - mg[c];
                yr[c] = p[k][c] - pr[c];
                xr[c] = g[k][c] - gr[c];
            }
            s2[0] += y0[0] * y0[0] + y0[1] * y0[1] + y0[2] * y0[2];
            s2[1] += x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) s2[2 + 3 * r + c] += x0[r] * y0[c];
            s2[11] += norm3(yr[0] - xr[0], yr[1] - xr[1], yr[2] - xr[2]);
            s2[12] += yr[0] * yr[0] + yr[1] * yr[1] + yr[2] * yr[2];
            s2[13] += yr[0] * xr[0] + yr[1] * xr[1] + yr[2] * xr[2];
        }
    }
    wave_sum(s2);
    const double ssY = s2[0], ssX = s2[1];
    const bool fit = n > 0.0 && ssY > ZERO_SS * s1[8] && ssX > ZERO_SS * s1[9];
    const double normY = sqrt(ssY), normX = sqrt(ssX);
    const double s_opt = root_ok ? s2[13] / s2[12] : nan;

    // the fit, the same on every lane
    double A[3][3], U[3][3], V[3][3], sv[3], T[3][3];
    const double inv = 1.0 / (fit ? normX * normY : 1.0);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r][c] = s2[2 + 3 * r + c] * inv;
    svd3(A, U, sv, V);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[r][c] = V[r][0] * U[c][0] + V[r][1] * U[c][1] + V[r][2] * U[c][2];
    if (a.reflection != 0) {
        const bool have = det3(T) < 0.0;
        if (have != (a.reflection == 2)) {  // (uniform over the wave)
            sv[2] = -sv[2];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) T[r][c] = V[r][0] * U[c][0] + V[r][1] * U[c][1] - V[r][2] * U[c][2];
        }
    }
    const double trace = sv[0] + sv[1] + sv[2];
    const double b = a.scaling ? trace * normX / normY : 1.0;
    const double d = a.scaling ? 1.0 - trace * trace : 1.0 + ssY / ssX - 2.0 * trace * normY / normX;
    double cv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) cv[c] = mg[c] - b * (mp[0] * T[0][c] + mp[1] * T[1][c] + mp[2] * T[2][c]);

    // third butterfly: the scaled and the aligned error; the per-joint outputs
    double s3[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        const int j = lane + 64 * k;
        double y0[3], z[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) y0[c] = p[k][c] - mp[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) z[c] = b * (y0[0] * T[0][c] + y0[1] * T[1][c] + y0[2] * T[2][c]) + mg[c];
        const double pe = norm3(z[0] - g[k][0], z[1] - g[k][1], z[2] - g[k][2]);
        const double ne = norm3(s_opt * (p[k][0] - pr[0]) - (g[k][0] - gr[0]), s_opt * (p[k][1] - pr[1]) - (g[k][1] - gr[1]),
                                s_opt * (p[k][2] - pr[2]) - (g[k][2] - gr[2]));
        if (on[k]) {
            s3[0] += ne;
            s3[1] += pe;
        }
        if (in[k]) {
            a.err[fj + j] = on[k] ? e[k] : 0.0;
            a.pa_err[fj + j] = on[k] ? (fit ? pe : nan) : 0.0;
            if (a.aligned) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.aligned[(fj + j) * 3 + c] = (float)(fit ? z[c] : nan);
            }
        }
    }
    wave_sum(s3);
    if (lane == 0) {
        double* rec = a.frames + (size_t)f * NCOL;
        rec[0] = n;
        rec[1] = s1[7] / n;
        rec[2] = root_ok ? s2[11] / n : nan;
        rec[3] = s3[0] / n;
        rec[4] = fit ? s3[1] / n : nan;
        rec[5] = fit ? d : nan;
        rec[6] = fit ? b : nan;
#pragma unroll
        for (int c = 0; c < 3; ++c) rec[7 + c] = fit ? sv[c] : nan;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) rec[10 + 3 * r + c] = fit ? T[r][c] : nan;
#pragma unroll
        for (int c = 0; c < 3; ++c) rec[19 + c] = fit ? cv[c] : nan;
        rec[22] = normX;
        rec[23] = normY;
        rec[24] = s_opt;
    }
}

// last == 0: a workgroup per SLOT_FRAMES frames.  The frames' error planes are staged in LDS (NaN where a pair does not
// count: an unselected or invalid joint, a frame without a fit), then every thread owns output elements of the slot and
// walks the staged pairs in (frame, joint) order.  last == 1: one workgroup, every thread owns elements of the totals
// and walks the slots in order.
__global__ __launch_bounds__(NTHR) void pose_total_kernel(TotalArgs a, int last) {
    extern __shared__ double lds[];  // [2][SLOT_FRAMES][J]
    const int t = threadIdx.x;
    if (last) {
        for (int i = t; i < NTOT; i += NTHR) {
            if (i >= T_COUNT) {
                long long s = 0;
                for (int b = 0; b < a.nslots; ++b) s += ((const long long*)a.slots)[(size_t)b * NTOT + i];
                ((long long*)a.totals)[i] = s;
            } else {
                double s = 0.0;
                for (int b = 0; b < a.nslots; ++b) s += a.slots[(size_t)b * NTOT + i];
                a.totals[i] = s;
            }
        }
        return;
    }
    const long long f0 = (long long)blockIdx.x * SLOT_FRAMES;
    const int nf = (int)(a.F - f0 < SLOT_FRAMES ? a.F - f0 : SLOT_FRAMES);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double* e_lds = lds;
    double* pa_lds = lds + SLOT_FRAMES * a.J;
    for (int i = t; i < nf * a.J; i += NTHR) {
        const int fl = i / a.J, j = i % a.J;
        const size_t at = (size_t)(f0 + fl) * (size_t)a.J + j;
        const bool counted = a.frames[(size_t)(f0 + fl) * NCOL + 4] == a.frames[(size_t)(f0 + fl) * NCOL + 4];
        const bool on = counted && ((a.sel[j >> 6] >> (j & 63)) & 1ull) != 0 && (a.valid ? a.valid[at] != 0 : true);
        e_lds[i] = on ? a.err[at] : nan;
        pa_lds[i] = on ? a.pa_err[at] : nan;
    }
    __syncthreads();
    double* slot = a.slots + (size_t)blockIdx.x * NTOT;
    // the frame counts and the scores' sums: n_scored, n_root, n_scaled, mpjpe, mpjpe_root, n_mpjpe, pa_mpjpe
    if (t < 8) {
        double s = 0.0;
        for (int fl = 0; fl < nf; ++fl) {
            const double* rec = a.frames + (size_t)(f0 + fl) * NCOL;
            const bool counted = rec[4] == rec[4];
            const bool root = counted && rec[2] == rec[2], scaled = counted && rec[3] == rec[3];
            double v = 0.0;
            if (t == 0) v = counted ? 1.0 : 0.0;
            if (t == 1) v = root ? 1.0 : 0.0;
            if (t == 2) v = scaled ? 1.0 : 0.0;
            if (t == 3) v = counted ? rec[1] : 0.0;
            if (t == 4) v = root ? rec[2] : 0.0;
            if (t == 5) v = scaled ? rec[3] : 0.0;
            if (t == 6) v = counted ? rec[4] : 0.0;
            s += v;
        }
        slot[t] = s;
    }
    // per joint: the sums of err and pa_err and the count of pairs (threads 0 .. 3 J)
    for (int i = t; i < 3 * MAXJ; i += NTHR) {
        const int which = i / MAXJ, j = i % MAXJ;
        double s = 0.0;
        if (j < a.J) {
            const double* src = which == 1 ? pa_lds : e_lds;
            for (int fl = 0; fl < nf; ++fl) {
                const double v = src[fl * a.J + j];
                if (v == v) s += which == 2 ? 1.0 : v;
            }
        }
        slot[T_JOINT + i] = s;
    }
    // per threshold: the pairs with pa_err < t (first MAXT) and with err < t (second MAXT)
    if (t < 2 * MAXT) {
        const int which = t / MAXT, k = t % MAXT;
        long long c = 0;
        if (k < a.nt) {
            const double* src = which == 0 ? pa_lds : e_lds;
            const double thr = a.thr[k];
            for (int i = 0; i < nf * a.J; ++i) c += src[i] < thr ? 1 : 0;  // (NaN compares false)
        }
        ((long long*)slot)[T_COUNT + t] = c;
    }
}

inline long long slots_of(long long F) { return (F + SLOT_FRAMES - 1) / SLOT_FRAMES; }

inline size_t workspace_words(long long F, long long J) {
    const long long w = F * NCOL + 2 * F * J + slots_of(F) * NTOT;
    return (size_t)(w > 0 ? w : 1);
}

}  // namespace

extern "C" {

size_t anerf_pose_scores_workspace(int32_t n_frames, int32_t n_joints, int32_t n_thresholds) {
    if (n_frames < 0 || n_joints < 1 || n_joints > MAXJ || n_thresholds < 0 || n_thresholds > MAXT) {
        fail("anerf_pose_scores_workspace", "n_frames >= 0, n_joints in [1, 128], n_thresholds in [0, 64]");
        return 0;
    }
    return sizeof(double) * workspace_words(n_frames, n_joints);
}

int anerf_pose_scores(const void* pred, const void* gt, int32_t n_frames, int32_t n_joints, const int32_t* joint_idx,
                      int32_t n_selected, const uint8_t* valid, int32_t root, double pred_scale, double gt_scale,
                      int32_t flags, const double* thresholds, int32_t n_thresholds, double* totals, double* frames,
                      double* err, double* pa_err, float* aligned, void* workspace, size_t workspace_bytes,
                      void* stream) {
    const char* fn = "anerf_pose_scores";
    if (!pred || !gt) return fail(fn, "pred and gt must not be NULL");
    if (!totals) return fail(fn, "totals must not be NULL");
    if (n_frames < 0) return fail(fn, "n_frames must be >= 0");
    if (n_joints < 1 || n_joints > MAXJ) return fail(fn, "n_joints must be in [1, 128]");
    if (root < -1 || root >= n_joints) return fail(fn, "root must be a joint in [0, n_joints), or -1 for none");
    const int32_t known = ANERF_POSE_PRED_F64 | ANERF_POSE_GT_F64 | ANERF_POSE_NO_SCALING | ANERF_POSE_REFLECT_FALSE |
                          ANERF_POSE_REFLECT_TRUE;
    if (flags & ~known) return fail(fn, "unknown flag bits");
    if ((flags & ANERF_POSE_REFLECT_FALSE) && (flags & ANERF_POSE_REFLECT_TRUE))
        return fail(fn, "ANERF_POSE_REFLECT_FALSE and ANERF_POSE_REFLECT_TRUE exclude each other");
    if (!std::isfinite(pred_scale) || !std::isfinite(gt_scale)) return fail(fn, "pred_scale and gt_scale must be finite");
    if (n_thresholds < 0 || n_thresholds > MAXT) return fail(fn, "n_thresholds must be in [0, 64]");
    if (n_thresholds > 0 && !thresholds) return fail(fn, "thresholds must not be NULL with n_thresholds > 0");
    unsigned long long sel[PASSES] = {};
    if (joint_idx) {
        if (n_selected < 0 || n_selected > n_joints) return fail(fn, "n_selected must be in [0, n_joints]");
        for (int i = 0; i < n_selected; ++i) {
            const int32_t j = joint_idx[i];
            char msg[160];
            if (j < 0 || j >= n_joints) {
                snprintf(msg, sizeof msg, "joint_idx[%d] = %d is outside [0, %d)", i, j, n_joints);
                return fail(fn, msg);
            }
            if ((sel[j >> 6] >> (j & 63)) & 1ull) {
                snprintf(msg, sizeof msg, "joint_idx[%d] = %d is repeated", i, j);
                return fail(fn, msg);
            }
            sel[j >> 6] |= 1ull << (j & 63);
        }
    } else {
        for (int j = 0; j < n_joints; ++j) sel[j >> 6] |= 1ull << (j & 63);
    }
    if (!workspace) return fail(fn, "workspace must not be NULL");
    if (((uintptr_t)workspace & 7) != 0) return fail(fn, "the workspace must be 8-byte aligned");
    if (workspace_bytes < sizeof(double) * workspace_words(n_frames, n_joints))
        return anerf_internal_fail(ANERF_EWORKSPACE, "anerf_pose_scores: workspace too small");
    if (n_frames == 0) return ANERF_OK;

    const size_t F = (size_t)n_frames, J = (size_t)n_joints;
    double* ws = (double*)workspace;
    ScoreArgs s;
    s.pred = pred;
    s.gt = gt;
    s.valid = valid;
    s.frames = frames ? frames : ws;
    s.err = err ? err : ws + F * NCOL;
    s.pa_err = pa_err ? pa_err : ws + F * NCOL + F * J;
    s.aligned = aligned;
    s.F = n_frames;
    s.J = n_joints;
    s.root = root;
    s.pred_f64 = (flags & ANERF_POSE_PRED_F64) != 0;
    s.gt_f64 = (flags & ANERF_POSE_GT_F64) != 0;
    s.scaling = (flags & ANERF_POSE_NO_SCALING) == 0;
    s.reflection = (flags & ANERF_POSE_REFLECT_FALSE) ? 1 : ((flags & ANERF_POSE_REFLECT_TRUE) ? 2 : 0);
    s.pred_scale = pred_scale;
    s.gt_scale = gt_scale;
    TotalArgs t;
    t.frames = s.frames;
    t.err = s.err;
    t.pa_err = s.pa_err;
    t.valid = valid;
    t.slots = ws + F * NCOL + 2 * F * J;
    t.totals = totals;
    t.F = n_frames;
    t.J = n_joints;
    t.nt = n_thresholds;
    t.nslots = (int)slots_of(n_frames);
    for (int k = 0; k < PASSES; ++k) s.sel[k] = t.sel[k] = sel[k];
    for (int k = 0; k < MAXT; ++k) t.thr[k] = k < n_thresholds ? thresholds[k] : 0.0;
    const size_t lds = sizeof(double) * 2 * SLOT_FRAMES * J;  // <= 64 KB
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_score_kernel, dim3((unsigned)((F + WAVES - 1) / WAVES)), dim3(NTHR), 0, st, s);
    hipLaunchKernelGGL(pose_total_kernel, dim3((unsigned)t.nslots), dim3(NTHR), lds, st, t, 0);
    hipLaunchKernelGGL(pose_total_kernel, dim3(1), dim3(NTHR), 0, st, t, 1);
    return launched(fn);
}

}  // extern "C"

// anerf_eval.hip — scoring of rendered frames on the device: squared error and SSIM, summed per frame.
//
// The reference scores on the host (core/utils/evaluation_helpers.py:257-385, run_render.py:883-968): every frame is
// downloaded and a CPU SSIM runs over it.  Here one launch scores up to EVAL_MAX frames of one size where they lie:
//
//   anerf_eval_frames   eval_kernel        a workgroup per TW x TH tile of a frame: the tile and its 5-pixel halo staged
//                                          in LDS as fp32, per channel the horizontal 11-tap pass of the five moment
//                                          planes (x, y, xx, yy, xy) into LDS in double, the vertical pass from LDS,
//                                          the SSIM map, and the tile's nine sums into its workspace slot
//                       eval_final_kernel  a workgroup per frame: the frame's slots in tile order -> sums [F][9]
//
// SSIM per pixel is a cancellation: sigma^2 = E[x^2] - mu^2 with C2 = 9e-4 (data_range 1) under differences of numbers
// near 1, where fp32 moments are off by up to 2.7e-4 per pixel (tests/test_eval_host.py).  So the moments, the map
// and the sums are double (the inputs widen exactly); the map output is the double value rounded once.  Every
// reduction has a fixed shape -- per thread in pixel order, an LDS tree per workgroup, one slot per (frame, tile), a
// last workgroup per frame over its slots in tile order -- so two runs give the same bits and a frame's sums do not
// depend on the other frames of the launch; there are no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/anerf.h"

int anerf_internal_fail(int code, const char* msg);  // anerf_render.hip: sets anerf_last_error()

namespace {

constexpr int NTHR = 256;       // threads per workgroup (4 waves of 64)
constexpr int TW = 32, TH = 16; // output tile
constexpr int RAD = 5, WIN = 11;  // the 11-tap window
constexpr int SW = TW + 2 * RAD, SH = TH + 2 * RAD;  // staged tile: 42 x 26
constexpr int NS = 9;           // { n, sum se, sum ssim } x { rectangle, rectangle x mask, rectangle x box }
constexpr int NM = 5;           // moment planes
constexpr int EVAL_MAX = 64;    // frames per launch (their rectangles travel by value)
constexpr int MAX_DIM = 1 << 15;

// LDS: 2 x 26 x 42 x 3 floats (26,208 B) + 5 x 26 x 32 doubles (33,280 B) = 59,488 B, two workgroups per CU's 160 KB
static_assert(NS * NTHR <= NM * SH * TW, "the moment planes double as the reduction's scratch");

struct EvalArgs {
    const float* pred;
    const void* gt;
    const unsigned char* mask;
    float* map;
    double* part;
    int H, W, tiles_x, tiles, gt_u8, valid, has_box;
    double c1, c2;
    double g[WIN];
    int rect[EVAL_MAX][4];
    int box[EVAL_MAX][4];
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

// The workgroup's sums of NS values per thread: an LDS tree, the same pairs on every run.  lds [NS * NTHR].
__device__ __forceinline__ void block_sum(double (&v)[NS], double* lds) {
    const int t = threadIdx.x;
    __syncthreads();  // (lds still holds the last channel's planes)
    for (int k = 0; k < NS; ++k) lds[k * NTHR + t] = v[k];
    __syncthreads();
    for (int s = NTHR / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < NS; ++k) lds[k * NTHR + t] += lds[k * NTHR + t + s];
        __syncthreads();
    }
    for (int k = 0; k < NS; ++k) v[k] = lds[k * NTHR];
}

__global__ __launch_bounds__(NTHR) void eval_kernel(EvalArgs a) {
    __shared__ float in[2][SH][SW][3];
    __shared__ double hp[NM][SH][TW];
    const int t = threadIdx.x;
    const int f = blockIdx.y, tile = blockIdx.x;
    const int tx0 = (tile % a.tiles_x) * TW, ty0 = (tile / a.tiles_x) * TH;
    const int x0 = a.rect[f][0], y0 = a.rect[f][1], x1 = a.rect[f][2], y1 = a.rect[f][3];
    // the scored pixels: the rectangle, less the window's radius per side under border = valid
    const int shrink = a.valid ? RAD : 0;
    const int sx0 = x0 + shrink, sy0 = y0 + shrink, sx1 = x1 - shrink, sy1 = y1 - shrink;
    const size_t fbase = (size_t)f * (size_t)a.H * (size_t)a.W;
    double* slot = a.part + ((size_t)f * (size_t)a.tiles + (size_t)tile) * NS;
    const bool live = max(tx0, sx0) < min(tx0 + TW, sx1) && max(ty0, sy0) < min(ty0 + TH, sy1);
    if (!live) {  // (the whole workgroup: no scored pixel in this tile)
        if (a.map)
            for (int p = t; p < TW * TH; p += NTHR) {
                const int y = ty0 + p / TW, x = tx0 + p % TW;
                if (y < a.H && x < a.W) {
                    float* m = a.map + (fbase + (size_t)y * a.W + x) * 3;
                    m[0] = m[1] = m[2] = 0.f;
                }
            }
        if (t < NS) slot[t] = 0.0;
        return;
    }
    // stage the tile and its halo: zeros outside the rectangle (which lies inside the frame)
    for (int i = t; i < SH * SW; i += NTHR) {
        const int r = i / SW, c = i % SW;
        const int y = ty0 - RAD + r, x = tx0 - RAD + c;
        float p[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
        if (x >= x0 && x < x1 && y >= y0 && y < y1) {
            const size_t at = (fbase + (size_t)y * a.W + x) * 3;
            for (int ch = 0; ch < 3; ++ch) {
                p[ch] = a.pred[at + ch];
                // a byte v is the fp32 that (v / 255.) rounds to, as the reference's `/ 255.` and astype(float32)
                q[ch] = a.gt_u8 ? (float)((double)((const unsigned char*)a.gt)[at + ch] / 255.0)
                                : ((const float*)a.gt)[at + ch];
            }
        }
        for (int ch = 0; ch < 3; ++ch) {
            in[0][r][c][ch] = p[ch];
            in[1][r][c][ch] = q[ch];
        }
    }
    double s[NS];
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        __syncthreads();  // (the staged tile is complete; the previous channel's planes are read)
        for (int i = t; i < SH * TW; i += NTHR) {
            const int r = i / TW, c = i % TW;
            double m[NM] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int k = 0; k < WIN; ++k) {
                const double x = in[0][r][c + k][ch], y = in[1][r][c + k][ch], w = a.g[k];
                m[0] += w * x;
                m[1] += w * y;
                m[2] += w * (x * x);
                m[3] += w * (y * y);
                m[4] += w * (x * y);
            }
            for (int j = 0; j < NM; ++j) hp[j][r][c] = m[j];
        }
        __syncthreads();
        for (int p = t; p < TW * TH; p += NTHR) {
            const int py = p / TW, px = p % TW;
            const int y = ty0 + py, x = tx0 + px;
            const bool scored = x >= sx0 && x < sx1 && y >= sy0 && y < sy1;
            double v = 0.0;
            if (scored) {
                double m[NM] = {0.0, 0.0, 0.0, 0.0, 0.0};
                for (int k = 0; k < WIN; ++k)
                    for (int j = 0; j < NM; ++j) m[j] += a.g[k] * hp[j][py + k][px];
                const double mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
                const double vx = m[2] - mxx, vy = m[3] - myy, vxy = m[4] - mxy;
                v = ((2.0 * mxy + a.c1) / (mxx + myy + a.c1)) * ((2.0 * vxy + a.c2) / (vx + vy + a.c2));
                const double d = (double)in[1][py + RAD][px + RAD][ch] - (double)in[0][py + RAD][px + RAD][ch];
                const double se = d * d;
                const size_t pix = fbase + (size_t)y * a.W + x;
                const bool wm = a.mask ? a.mask[pix] != 0 : true;
                const bool wb = a.has_box ? (x >= a.box[f][0] && x < a.box[f][2] && y >= a.box[f][1] && y < a.box[f][3])
                                          : true;
                const double one = ch == 0 ? 1.0 : 0.0;  // (n counts pixels)
                s[0] += one;
                s[1] += se;
                s[2] += v;
                if (wm) {
                    s[3] += one;
                    s[4] += se;
                    s[5] += v;
                }
                if (wb) {
                    s[6] += one;
                    s[7] += se;
                    s[8] += v;
                }
            }
            if (a.map && y < a.H && x < a.W) a.map[(fbase + (size_t)y * a.W + x) * 3 + ch] = (float)v;
        }
    }
    block_sum(s, &hp[0][0][0]);
    if (t < NS) slot[t] = s[t];
}

// One workgroup per frame: its tiles' slots, thread t taking slots t, t + NTHR, ... in order, then the tree.
__global__ __launch_bounds__(NTHR) void eval_final_kernel(const double* __restrict__ part, int tiles,
                                                          double* __restrict__ sums) {
    __shared__ double lds[NS * NTHR];
    const double* mine = part + (size_t)blockIdx.x * (size_t)tiles * NS;
    double s[NS];
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
    for (int b = threadIdx.x; b < tiles; b += NTHR)
        for (int k = 0; k < NS; ++k) s[k] += mine[(size_t)b * NS + k];
    block_sum(s, lds);
    if (threadIdx.x < NS) sums[(size_t)blockIdx.x * NS + threadIdx.x] = s[threadIdx.x];
}

inline long long tiles_of(int H, int W) { return (long long)((W + TW - 1) / TW) * ((H + TH - 1) / TH); }

int check_rects(const char* fn, const char* what, const int32_t* r, int n, int H, int W) {
    for (int f = 0; f < n; ++f) {
        const int32_t x0 = r[4 * f], y0 = r[4 * f + 1], x1 = r[4 * f + 2], y1 = r[4 * f + 3];
        if (x0 < 0 || y0 < 0 || x1 > W || y1 > H || x1 < x0 || y1 < y0 || x0 > W || y0 > H) {
            char msg[200];
            snprintf(msg, sizeof msg, "%s %d = (%d, %d, %d, %d) must satisfy 0 <= x0 <= x1 <= W = %d, 0 <= y0 <= y1 <= H = %d",
                     what, f, x0, y0, x1, y1, W, H);
            return fail(fn, msg);
        }
    }
    return ANERF_OK;
}

}  // namespace

extern "C" {

size_t anerf_eval_workspace(int32_t n_frames, int32_t H, int32_t W) {
    if (n_frames < 0 || H < 0 || W < 0 || H > MAX_DIM || W > MAX_DIM) {
        fail("anerf_eval_workspace", "n_frames >= 0, H and W in [0, 32768]");
        return 0;
    }
    const long long slots = (long long)n_frames * tiles_of(H, W);
    return sizeof(double) * NS * (size_t)(slots > 0 ? slots : 1);
}

int anerf_eval_frames(const float* pred, const void* gt, int32_t gt_uint8, const uint8_t* mask, const int32_t* rects,
                      const int32_t* boxes, int32_t n_frames, int32_t H, int32_t W, double data_range, int32_t border,
                      float* map, double* sums, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "anerf_eval_frames";
    if (!pred || !gt || !sums || !rects) return fail(fn, "pred, gt, rects and sums must not be NULL");
    if (n_frames < 0 || H < 0 || W < 0) return fail(fn, "n_frames, H and W must be >= 0");
    if (H > MAX_DIM || W > MAX_DIM) return fail(fn, "H and W must be <= 32768");
    if (border != ANERF_EVAL_SAME && border != ANERF_EVAL_VALID)
        return fail(fn, "unknown border (ANERF_EVAL_SAME or ANERF_EVAL_VALID)");
    if (!(data_range > 0.0) || !std::isfinite(data_range)) return fail(fn, "data_range must be > 0");
    if (const int rc = check_rects(fn, "rectangle", rects, n_frames, H, W)) return rc;
    if (boxes)
        if (const int rc = check_rects(fn, "box", boxes, n_frames, H, W)) return rc;
    if (!workspace) return fail(fn, "workspace must not be NULL");
    if (((uintptr_t)workspace & 7) != 0) return fail(fn, "the workspace must be 8-byte aligned");
    if (workspace_bytes < anerf_eval_workspace(n_frames, H, W))
        return anerf_internal_fail(ANERF_EWORKSPACE, "anerf_eval_frames: workspace too small");
    if (n_frames == 0) return ANERF_OK;
    const long long tiles = tiles_of(H, W);
    EvalArgs a;
    a.H = H;
    a.W = W;
    a.tiles_x = (W + TW - 1) / TW;
    a.tiles = (int)tiles;
    a.gt_u8 = gt_uint8 != 0;
    a.valid = border == ANERF_EVAL_VALID;
    a.has_box = boxes != nullptr;
    a.c1 = (0.01 * data_range) * (0.01 * data_range);
    a.c2 = (0.03 * data_range) * (0.03 * data_range);
    double gsum = 0.0;
    for (int k = 0; k < WIN; ++k) {
        a.g[k] = std::exp(-(double)((k - RAD) * (k - RAD)) / (2.0 * 1.5 * 1.5));
        gsum += a.g[k];
    }
    for (int k = 0; k < WIN; ++k) a.g[k] /= gsum;
    const size_t frame_px = (size_t)H * (size_t)W;
    for (int k0 = 0; k0 < n_frames && tiles > 0; k0 += EVAL_MAX) {  // the rectangles travel by value, EVAL_MAX at a time
        const int n = n_frames - k0 < EVAL_MAX ? n_frames - k0 : EVAL_MAX;
        a.pred = pred + (size_t)k0 * frame_px * 3;
        a.gt = a.gt_u8 ? (const void*)((const unsigned char*)gt + (size_t)k0 * frame_px * 3)
                       : (const void*)((const float*)gt + (size_t)k0 * frame_px * 3);
        a.mask = mask ? mask + (size_t)k0 * frame_px : nullptr;
        a.map = map ? map + (size_t)k0 * frame_px * 3 : nullptr;
        a.part = (double*)workspace + (size_t)k0 * (size_t)tiles * NS;
        for (int f = 0; f < EVAL_MAX; ++f)
            for (int c = 0; c < 4; ++c) {
                a.rect[f][c] = f < n ? rects[4 * (k0 + f) + c] : 0;
                a.box[f][c] = f < n && boxes ? boxes[4 * (k0 + f) + c] : 0;
            }
        hipLaunchKernelGGL(eval_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(NTHR), 0, (hipStream_t)stream, a);
    }
    hipLaunchKernelGGL(eval_final_kernel, dim3((unsigned)n_frames), dim3(NTHR), 0, (hipStream_t)stream,
                       (const double*)workspace, (int)tiles, sums);
    return launched(fn);
}

}  // extern "C"

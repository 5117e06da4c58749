// anerf_prep.hip — the pixel-level steps that make a dataset, on the device: mask morphology, skeleton segments,
// per-camera median backgrounds.
//
// Every loader of the reference runs them on the host with cv2 and NumPy before training can start (dilate_masks,
// core/load_surreal.py:50-59; get_mask, core/load_zju.py:53-63; create_kp_mask and draw_skeleton2d,
// core/utils/skeleton_utils.py:774-816 and :1363-1398; the median backgrounds of load_h36m.py:110 and
// load_zju.py:266-281).  Here the images stay where the dataset keeps them, as bytes in HBM:
//
//   anerf_mask_morph         morph_kernel    a workgroup per MW x MH tile of a mask: the tile and its halo staged in LDS
//                                            as bytes, the row pass (max / min over the clipped window) into LDS planes,
//                                            the column pass from them, the band rule and the OR with `other` at the store
//   anerf_draw_segments      segment_kernel  a workgroup per DW x DH tile of a frame: the frame's segments staged in LDS,
//                                            culled against the tile grown by ceil(w / 2) and compacted in index order;
//                                            a thread scans the survivors from the highest index down per pixel
//   anerf_background_median  median_kernel   a thread per (camera, pixel): a bisection on the value for the three
//                                            channels at once, eight counting passes over the camera's frames, one more
//                                            pass where the upper middle value differs from the lower
//
// Every decision is an integer decision (bytes, int32 counts, int64 products whose bounds anerf.h derives), no thread
// reads what another thread of the launch writes, and there are no atomics: the same bits on every run, and bit-identical
// to the NumPy checkers of a-nerf_amd/preprocess.py.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/anerf.h"

int anerf_internal_fail(int code, const char* msg);  // anerf_render.hip: sets anerf_last_error()

namespace {

constexpr int NTHR = 256;  // threads per workgroup (4 waves of 64)

// ---- morphology
constexpr int MW = 64, MH = 32;                   // output tile: a row of it is one wave's 64 bytes
constexpr int RMAX = ANERF_PREP_MAX_RADIUS;       // 32
constexpr int MSW = MW + 2 * RMAX, MSH = MH + 2 * RMAX;  // staged tile at the largest halo: 128 x 96
// LDS: 96 x 128 bytes staged (12,288 B) + 3 planes of 96 x 64 bytes (18,432 B) = 30,720 B, five workgroups per CU

// ---- segments
constexpr int DW = 32, DH = 16;  // output tile: 512 pixels, two per thread
constexpr int BMAX = ANERF_PREP_MAX_SEGMENTS;  // 128
constexpr int CMAX = ANERF_PREP_MAX_COORD;     // 8192

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

struct MorphArgs {
    const unsigned char* src;
    const unsigned char* other;
    unsigned char* dst;
    int H, W, tiles_x, tiles, erode, radius, band;
};

__global__ __launch_bounds__(NTHR) void morph_kernel(MorphArgs a) {
    __shared__ unsigned char in[MSH][MSW];
    __shared__ unsigned char pa[MSH][MW], pd[MSH][MW], pe[MSH][MW];  // op at radius; dilate, erode at band
    const int t = threadIdx.x;
    const int n = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int tx0 = (tile % a.tiles_x) * MW, ty0 = (tile / a.tiles_x) * MH;
    const int R = a.radius > a.band ? a.radius : a.band;  // the halo in use (<= RMAX)
    const int sw = MW + 2 * R, sh = MH + 2 * R;
    const size_t base = (size_t)n * (size_t)a.H * (size_t)a.W;
    // stage the tile and its halo (positions outside the mask are never read: the windows below are clipped to it)
    for (int i = t; i < sh * sw; i += NTHR) {
        const int r = i / sw, c = i % sw;
        const int y = ty0 - R + r, x = tx0 - R + c;
        unsigned char v = 0;
        if (x >= 0 && x < a.W && y >= 0 && y < a.H) v = a.src[base + (size_t)y * a.W + x];
        in[r][c] = v;
    }
    __syncthreads();
    // rows: for every staged row of the mask, the window [x - r, x + r] cut to [0, W)
    for (int i = t; i < sh * MW; i += NTHR) {
        const int r = i / MW, c = i % MW;
        const int y = ty0 - R + r, x = tx0 + c;
        if (y < 0 || y >= a.H || x >= a.W) continue;
        const int off = R - tx0;  // staged column of mask column 0
        {
            const int x0 = max(0, x - a.radius), x1 = min(a.W - 1, x + a.radius);
            int v = in[r][x0 + off];
            if (a.erode)
                for (int k = x0 + 1; k <= x1; ++k) v = min(v, (int)in[r][k + off]);
            else
                for (int k = x0 + 1; k <= x1; ++k) v = max(v, (int)in[r][k + off]);
            pa[r][c] = (unsigned char)v;
        }
        if (a.band > 0) {
            const int x0 = max(0, x - a.band), x1 = min(a.W - 1, x + a.band);
            int hi = in[r][x0 + off], lo = hi;
            for (int k = x0 + 1; k <= x1; ++k) {
                const int v = in[r][k + off];
                hi = max(hi, v);
                lo = min(lo, v);
            }
            pd[r][c] = (unsigned char)hi;
            pe[r][c] = (unsigned char)lo;
        }
    }
    __syncthreads();
    // columns: the window [y - r, y + r] cut to [0, H), then the band rule and the OR
    for (int p = t; p < MW * MH; p += NTHR) {
        const int py = p / MW, px = p % MW;
        const int y = ty0 + py, x = tx0 + px;
        if (y >= a.H || x >= a.W) continue;
        const int off = R - ty0;  // staged row of mask row 0
        const int y0 = max(0, y - a.radius), y1 = min(a.H - 1, y + a.radius);
        int v = pa[y0 + off][px];
        if (a.erode)
            for (int k = y0 + 1; k <= y1; ++k) v = min(v, (int)pa[k + off][px]);
        else
            for (int k = y0 + 1; k <= y1; ++k) v = max(v, (int)pa[k + off][px]);
        if (a.band > 0) {
            const int b0 = max(0, y - a.band), b1 = min(a.H - 1, y + a.band);
            int hi = pd[b0 + off][px], lo = pe[b0 + off][px];
            for (int k = b0 + 1; k <= b1; ++k) {
                hi = max(hi, (int)pd[k + off][px]);
                lo = min(lo, (int)pe[k + off][px]);
            }
            if (hi - lo == 1) v = 0;  // (uint8)(dilated - eroded) == 1: dilated >= eroded, so no wrap
        }
        const size_t at = base + (size_t)y * a.W + x;
        if (a.other) v = (v != 0 || a.other[at] != 0) ? 1 : 0;
        a.dst[at] = (unsigned char)v;
    }
}

struct SegArgs {
    const int* segs;
    const unsigned char* colors;
    unsigned char* mask;
    unsigned char* frames;
    int H, W, tiles_x, tiles, n_segs, w2, half;  // w2 = width^2, half = ceil(width / 2)
};

// Is the integer pixel centre (cx, cy) within width / 2 of the closed segment (px, py)-(qx, qy)?  Exact in int64:
// every coordinate difference is at most 2^14 in magnitude (anerf.h), so |t|, |d|^2 <= 2^29, |cross| < 2^29, the
// left sides stay under 2^60 and w^2 |d|^2 under 2^53.
__device__ __forceinline__ bool covers(int px, int py, int qx, int qy, int cx, int cy, long long w2) {
    const long long dx = qx - px, dy = qy - py, ex = cx - px, ey = cy - py;
    const long long t = ex * dx + ey * dy, dd = dx * dx + dy * dy;
    if (t <= 0) return 4 * (ex * ex + ey * ey) <= w2;
    if (t >= dd) {
        const long long fx = cx - qx, fy = cy - qy;
        return 4 * (fx * fx + fy * fy) <= w2;
    }
    const long long cr = dx * ey - dy * ex;
    return 4 * cr * cr <= w2 * dd;
}

__global__ __launch_bounds__(NTHR) void segment_kernel(SegArgs a) {
    __shared__ int seg[BMAX][4];
    __shared__ int list[BMAX];
    __shared__ int wcnt[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int f = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int tx0 = (tile % a.tiles_x) * DW, ty0 = (tile / a.tiles_x) * DH;
    // stage and cull: thread b takes segment b (waves 0 and 1 hold the BMAX = 128 of them)
    bool alive = false;
    if (t < a.n_segs) {
        const int* s = a.segs + ((size_t)f * a.n_segs + t) * 4;
        const int px = s[0], py = s[1], qx = s[2], qy = s[3];
        seg[t][0] = px;
        seg[t][1] = py;
        seg[t][2] = qx;
        seg[t][3] = qy;
        const bool in_range = px >= -CMAX && px <= CMAX && py >= -CMAX && py <= CMAX && qx >= -CMAX && qx <= CMAX &&
                              qy >= -CMAX && qy <= CMAX;  // (a segment with an endpoint outside is dropped)
        alive = in_range && min(px, qx) - a.half <= tx0 + DW - 1 && max(px, qx) + a.half >= tx0 &&
                min(py, qy) - a.half <= ty0 + DH - 1 && max(py, qy) + a.half >= ty0;
    }
    const unsigned long long m = __ballot(alive);
    if (lane == 0 && wave < 2) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (alive) list[(wave ? wcnt[0] : 0) + __popcll(m & ((1ull << lane) - 1ull))] = t;  // ascending segment index
    __syncthreads();
    const int n_alive = wcnt[0] + wcnt[1];
    const size_t fbase = (size_t)f * (size_t)a.H * (size_t)a.W;
    for (int p = t; p < DW * DH; p += NTHR) {
        const int y = ty0 + p / DW, x = tx0 + p % DW;
        if (y >= a.H || x >= a.W) continue;
        int hit = -1;
        for (int k = n_alive - 1; k >= 0; --k) {  // the highest index wins: later joints paint over earlier ones
            const int b = list[k];
            if (covers(seg[b][0], seg[b][1], seg[b][2], seg[b][3], x, y, a.w2)) {
                hit = b;
                break;
            }
        }
        const size_t at = fbase + (size_t)y * a.W + x;
        if (a.mask) a.mask[at] = hit >= 0 ? 1 : 0;
        if (a.frames && hit >= 0) {
            unsigned char* o = a.frames + at * 3;
            const unsigned char* c = a.colors + hit * 3;
            o[0] = c[0];
            o[1] = c[1];
            o[2] = c[2];
        }
    }
}

// One thread per (camera, pixel).  The rank-k value of the taken frames is the smallest v with #{value <= v} > k; the
// bisection on v takes eight passes whatever the data, with all three channels (and, in the first pass, the number
// of frames taken) counted in the same pass.  int32 counters: a camera has at most ANERF_PREP_MAX_CAMERA_FRAMES.
__global__ __launch_bounds__(NTHR) void median_kernel(const unsigned char* __restrict__ imgs,
                                                      const unsigned char* __restrict__ masks, size_t n_pixels,
                                                      const int* __restrict__ order, const int* __restrict__ cam_start,
                                                      unsigned char* __restrict__ bkgds, int* __restrict__ counts) {
    const size_t p = (size_t)blockIdx.x * NTHR + threadIdx.x;
    if (p >= n_pixels) return;
    const int cam = blockIdx.y;
    const int i0 = cam_start[cam], i1 = cam_start[cam + 1];
    int lo[3] = {0, 0, 0}, hi[3] = {255, 255, 255}, chi[3] = {-1, -1, -1};  // chi: #{value <= hi}, -1: all taken
    int n = 0;
    for (int pass = 0; pass < 8; ++pass) {
        const int mid[3] = {(lo[0] + hi[0]) >> 1, (lo[1] + hi[1]) >> 1, (lo[2] + hi[2]) >> 1};
        int c[3] = {0, 0, 0}, taken = 0;
        for (int i = i0; i < i1; ++i) {
            const size_t at = (size_t)order[i] * n_pixels + p;
            if (masks && masks[at] != 0) continue;
            const unsigned char* v = imgs + at * 3;
            ++taken;
            c[0] += v[0] <= mid[0];
            c[1] += v[1] <= mid[1];
            c[2] += v[2] <= mid[2];
        }
        if (pass == 0) n = taken;
        const int k = (n - 1) >> 1;  // the lower middle rank (n == 0: the result is set below)
        for (int ch = 0; ch < 3; ++ch) {
            if (c[ch] > k) {
                hi[ch] = mid[ch];
                chi[ch] = c[ch];
            } else {
                lo[ch] = mid[ch] + 1;
            }
        }
    }
    // lo == hi: the lower middle value.  The upper middle value (rank n / 2) is the same unless n is even and exactly
    // n / 2 values are <= it; then it is the smallest value above, found in one more pass
    int up[3] = {lo[0], lo[1], lo[2]};
    bool more = false, need[3];
    for (int ch = 0; ch < 3; ++ch) {
        const int below = chi[ch] < 0 ? n : chi[ch];
        need[ch] = n > 0 && below <= (n >> 1);
        if (need[ch]) up[ch] = 255;
        more = more || need[ch];
    }
    if (more) {
        for (int i = i0; i < i1; ++i) {
            const size_t at = (size_t)order[i] * n_pixels + p;
            if (masks && masks[at] != 0) continue;
            const unsigned char* v = imgs + at * 3;
            for (int ch = 0; ch < 3; ++ch)
                if (need[ch] && v[ch] > lo[ch] && v[ch] < up[ch]) up[ch] = v[ch];
        }
    }
    unsigned char* o = bkgds + ((size_t)cam * n_pixels + p) * 3;
    for (int ch = 0; ch < 3; ++ch) o[ch] = n > 0 ? (unsigned char)((lo[ch] + up[ch]) >> 1) : 0;
    if (counts) counts[(size_t)cam * n_pixels + p] = n;
}

}  // namespace

extern "C" {

int anerf_mask_morph(const uint8_t* src, uint8_t* dst, int64_t n_masks, int32_t H, int32_t W, int32_t op,
                     int32_t radius, int32_t band, const uint8_t* other, void* stream) {
    const char* fn = "anerf_mask_morph";
    if (!src || !dst) return fail(fn, "src and dst must not be NULL");
    if (src == dst) return fail(fn, "dst must not be src (a tile reads its neighbours' pixels)");
    if (op != ANERF_MORPH_DILATE && op != ANERF_MORPH_ERODE)
        return fail(fn, "unknown operation (ANERF_MORPH_DILATE or ANERF_MORPH_ERODE)");
    if (n_masks < 0) return fail(fn, "n_masks must be >= 0");
    if (H < 1 || W < 1 || H > ANERF_PREP_MAX_DIM || W > ANERF_PREP_MAX_DIM) return fail(fn, "H and W must be in [1, 32768]");
    if (radius < 0 || radius > RMAX) return fail(fn, "radius must be in [0, 32]");
    if (band < 0 || band > RMAX) return fail(fn, "band must be in [0, 32]");
    if (band > 0 && op != ANERF_MORPH_DILATE) return fail(fn, "the band is cleared from a dilation: op must be ANERF_MORPH_DILATE");
    const long long tiles_x = (W + MW - 1) / MW, tiles = tiles_x * ((H + MH - 1) / MH);
    if (tiles * n_masks > 0x7fffffffLL) return fail(fn, "n_masks x tiles must be below 2^31");
    if (n_masks == 0) return ANERF_OK;
    MorphArgs a;
    a.src = src;
    a.other = other;
    a.dst = dst;
    a.H = H;
    a.W = W;
    a.tiles_x = (int)tiles_x;
    a.tiles = (int)tiles;
    a.erode = op == ANERF_MORPH_ERODE;
    a.radius = radius;
    a.band = band;
    hipLaunchKernelGGL(morph_kernel, dim3((unsigned)(tiles * n_masks)), dim3(NTHR), 0, (hipStream_t)stream, a);
    return launched(fn);
}

int anerf_draw_segments(const int32_t* segs, int32_t n_frames, int32_t n_segs, int32_t H, int32_t W, int32_t width,
                        const uint8_t* colors, uint8_t* mask, uint8_t* frames, void* stream) {
    const char* fn = "anerf_draw_segments";
    if (!mask && !frames) return fail(fn, "one of mask and frames must be given");
    if (frames && !colors) return fail(fn, "frames are painted with colors: colors must not be NULL");
    if (n_frames < 0) return fail(fn, "n_frames must be >= 0");
    if (n_segs < 0 || n_segs > BMAX) return fail(fn, "n_segs must be in [0, 128]");
    if (n_segs > 0 && !segs) return fail(fn, "segs must not be NULL");
    if (H < 1 || W < 1 || H > CMAX || W > CMAX) return fail(fn, "H and W must be in [1, 8192]");
    if (width < 1 || width > ANERF_PREP_MAX_WIDTH) return fail(fn, "width must be in [1, 4096]");
    const long long tiles_x = (W + DW - 1) / DW, tiles = tiles_x * ((H + DH - 1) / DH);
    if (tiles * n_frames > 0x7fffffffLL) return fail(fn, "n_frames x tiles must be below 2^31");
    if (n_frames == 0) return ANERF_OK;
    SegArgs a;
    a.segs = segs;
    a.colors = colors;
    a.mask = mask;
    a.frames = frames;
    a.H = H;
    a.W = W;
    a.tiles_x = (int)tiles_x;
    a.tiles = (int)tiles;
    a.n_segs = n_segs;
    a.w2 = width * width;
    a.half = (width + 1) / 2;
    hipLaunchKernelGGL(segment_kernel, dim3((unsigned)(tiles * n_frames)), dim3(NTHR), 0, (hipStream_t)stream, a);
    return launched(fn);
}

int anerf_background_median(const uint8_t* imgs, const uint8_t* masks, int64_t n_imgs, int64_t n_pixels,
                            const int32_t* order_host, const int32_t* cam_start_host, const int32_t* order,
                            const int32_t* cam_start, int32_t n_cams, uint8_t* bkgds, int32_t* counts, void* stream) {
    const char* fn = "anerf_background_median";
    if (!imgs || !bkgds) return fail(fn, "imgs and bkgds must not be NULL");
    if (!cam_start_host || !cam_start) return fail(fn, "cam_start must be given on the host and on the device");
    if (n_imgs < 0 || n_imgs > 0x7fffffffLL) return fail(fn, "n_imgs must be in [0, 2^31)");
    if (n_pixels < 1 || n_pixels > (int64_t)ANERF_PREP_MAX_DIM * ANERF_PREP_MAX_DIM)
        return fail(fn, "n_pixels must be in [1, 2^30]");
    if (n_cams < 0 || n_cams > 65535) return fail(fn, "n_cams must be in [0, 65535]");
    if (cam_start_host[0] != 0) return fail(fn, "cam_start[0] must be 0");
    for (int c = 0; c < n_cams; ++c) {
        const long long cnt = (long long)cam_start_host[c + 1] - cam_start_host[c];
        if (cnt < 0) return fail(fn, "cam_start must not decrease");
        if (cnt > ANERF_PREP_MAX_CAMERA_FRAMES) {
            char msg[160];
            snprintf(msg, sizeof msg, "camera %d lists %lld frames, the limit is %d (ANERF_PREP_MAX_CAMERA_FRAMES)", c, cnt,
                     ANERF_PREP_MAX_CAMERA_FRAMES);
            return fail(fn, msg);
        }
    }
    const int m = cam_start_host[n_cams];
    if (m > 0 && (!order_host || !order)) return fail(fn, "order must be given on the host and on the device");
    for (int i = 0; i < m; ++i)
        if (order_host[i] < 0 || order_host[i] >= n_imgs) {
            char msg[160];
            snprintf(msg, sizeof msg, "order[%d] = %d is outside [0, n_imgs = %lld)", i, order_host[i], (long long)n_imgs);
            return fail(fn, msg);
        }
    if (n_cams == 0) return ANERF_OK;
    const long long blocks = (n_pixels + NTHR - 1) / NTHR;
    hipLaunchKernelGGL(median_kernel, dim3((unsigned)blocks, (unsigned)n_cams), dim3(NTHR), 0, (hipStream_t)stream, imgs,
                       masks, (size_t)n_pixels, order, cam_start, bkgds, counts);
    return launched(fn);
}

}  // extern "C"
